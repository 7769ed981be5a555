"""The host check of the sparse-GP kernels as a test, without a GPU: cugp_amd/csrc/sparse_device.h and, as the handle's own y
runs it (p = 1), sparse_targets_device.h -- the text kernels.hip compiles for gfx950 -- run behind tools/host_emul.h as 256 host threads per workgroup in a stand-alone program built with
-fsanitize=address,undefined (tools/sparse_host_check.cpp; nothing is loaded into Python, nothing preloaded), on exact-size
heap buffers with NaN where the kernels must not read, and is compared with numpy by the script's own run(): the trace sums
of k_trace_cross<ARD, KIND> on a ragged chunk and on the square, k_sparse_finalize_targets' results, and the small passes around
the products.  The program is built once per module; the cases are the script's whole list (chunks of 44, 128, 1, 44, 1,
200 and 257 rows; M = 65, 128, 130, 64, 200 and 260 -- mpad 384 with five Gram partials --; SE, Matern 3/2, SE-ARD with two feature chunks, Matern-5/2-ARD).  A case fails on a
non-zero exit, on anything a sanitizer writes to stderr, and on a result beyond its tolerance."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import host_check  # noqa: E402
import sparse_host_check  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists(host_check.CLANG), reason="no host compiler at " + host_check.CLANG)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("sparse"))
    return host_check.build("sparse_host_check", tmp), tmp


def test_the_list_covers_the_shapes_and_families():
    import truth_sparse as ts
    fams = {ts.CASES[name][0] for name, _ in sparse_host_check.CASES}
    assert fams == {"se", "matern32", "ard", "matern52_ard"}
    ms = {ts.CASES[name][2] for name, _ in sparse_host_check.CASES}
    assert {65, 128, 130, 200} <= ms                        # identity padding, none, two tiles (ragged), two tiles
    assert {rows for _, rows in sparse_host_check.CASES} >= {None, 1, 200}
    # mpad 384 (three M tiles), 257 rows (three test tiles of the prediction), five Gram partials
    assert sparse_host_check.CASES_MPAD384 == (("se_n1300_m260_c0", 257, 5),) and ts.CASES["se_n1300_m260_c0"][2] == 260


@pytest.mark.parametrize("case", sparse_host_check.CASES + sparse_host_check.CASES_MPAD384, ids=lambda c: "-".join(str(v) for v in c))
def test_sparse(program, capfd, case):
    exe, tmp = program
    ok = sparse_host_check.run(exe, tmp, *case)
    line = capfd.readouterr().out
    print(line, end="")
    assert ok and "BAD" not in line and "FAILED" not in line, line
    assert line.rstrip().endswith("ok"), line
