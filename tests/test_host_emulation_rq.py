"""The host check of the rational quadratic gradient kernels as a test, without a GPU: cugp_amd/csrc/cov_device.h -- the text
kernels.hip compiles for gfx950 -- runs behind tools/host_emul.h as 256 host threads per workgroup in a stand-alone program
built with -fsanitize=address,undefined (tools/rq_host_check.cpp; nothing is loaded into Python, nothing preloaded), on
exact-size heap buffers with NaN where the kernels must not read.  k_trace<true, RQ> plain and over m targets and
k_predict_grad<true, RQ> are compared BIT FOR BIT with a plain loop in the same order of summation inside the program (a
mismatch is exit code 4), and with fp64 numpy by the script's own run().  The program is built once per module; the cases
are the script's whole list (npad 128 and 384; n = 65, 257; d = 3 and 17: one and two feature chunks; m = 3 and 17: across
the 16-target staging chunk; nt up to 129: beyond one test tile).  A case fails on a non-zero exit, on anything a sanitizer
writes to stderr, and on a result beyond its tolerance."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import host_check  # noqa: E402
import rq_host_check  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists(host_check.CLANG), reason="no host compiler at " + host_check.CLANG)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("rq"))
    return host_check.build("rq_host_check", tmp), tmp


def test_the_list_covers_the_kernels_and_sizes():
    C = rq_host_check.CASES
    assert {c[0] for c in C} == {"trace", "targets", "grad"}
    for kernel in ("trace", "targets", "grad"):
        assert {(c[1], c[2]) for c in C if c[0] == kernel} >= {(65, 3), (257, 17)}, kernel
        assert {c[2] for c in C if c[0] == kernel} == {3, 17}
    assert all((c[1] + 127) // 128 * 128 <= 384 for c in C)
    assert {c[4] for c in C if c[0] == "targets"} == {3, 17}
    assert max(c[4] for c in C if c[0] == "grad") > 128 and any(c[5] == 0 for c in C if c[0] == "grad")
    assert {c[3] for c in C} >= {0.4, -0.7, 2.0, 12.0}


@pytest.mark.parametrize("case", rq_host_check.CASES, ids=["%s-n%d-d%d-a%g-%d" % c[:5] for c in rq_host_check.CASES])
def test_kernel_equals_the_plain_loop_under_the_sanitizers(program, case):
    exe, tmp = program
    assert rq_host_check.run(exe, tmp, *case)
