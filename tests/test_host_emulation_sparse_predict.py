"""The host check of the sparse model's input-gradient pass as a test, without a GPU: cugp_amd/csrc/sparse_predict_device.h --
the text kernels.hip compiles for gfx950 -- runs behind tools/host_emul.h as 256 host threads per workgroup in a stand-alone
program built with -fsanitize=address,undefined (tools/sparse_joint_host_check.cpp; nothing is loaded into Python, nothing
preloaded), on heap buffers with NaN where the kernel must not read and a marker where it must not write, and is compared by
the script's own run(): bit for bit with a plain double loop and with numpy.  The program is built once per module; the cases
are the script's whole list (a ragged nt in two tiles at mpad 128 and at mpad 384, one row, no padding).  A case fails on a
non-zero exit, on anything a sanitizer writes to stderr, and on a result that differs."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import host_check  # noqa: E402
import sparse_joint_host_check  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists(host_check.CLANG), reason="no host compiler at " + host_check.CLANG)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("sparse_joint"))
    return host_check.build("sparse_joint_host_check", tmp), tmp


def test_the_list_covers_the_shapes():
    cases = sparse_joint_host_check.CASES
    assert {(m + 127) // 128 * 128 for _, m in cases} >= {128, 384}            # mpad 128 and 384
    assert any(nt % 128 and nt > 128 for nt, _ in cases)                       # a ragged nt beyond one tile
    assert any(m % 128 for _, m in cases) and any(m % 128 == 0 for _, m in cases)


@pytest.mark.parametrize("case", sparse_joint_host_check.CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_sparse_predict_diff(program, capfd, case):
    exe, tmp = program
    ok = sparse_joint_host_check.run(exe, tmp, *case)
    line = capfd.readouterr().out
    print(line, end="")
    assert ok and "BAD" not in line and "FAILED" not in line and "DIFFERENT" not in line, line
    assert line.rstrip().endswith("ok"), line
