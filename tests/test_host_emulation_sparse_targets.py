"""The host check of the multi-target sparse-GP kernels as a test, without a GPU: cugp_amd/csrc/sparse_targets_device.h -- the
text kernels.hip compiles for gfx950 -- runs behind tools/host_emul.h as 256 host threads per workgroup in a stand-alone
program built with -fsanitize=address,undefined (tools/sparse_targets_host_check.cpp; nothing is loaded into Python, nothing
preloaded), on exact-size heap buffers with NaN where the kernels must mask (rows beyond the chunk's count, columns beyond M;
the targets' buffers end at target p, so a read beyond it in the last group is a sanitizer report), and is compared BIT FOR
BIT with plain numpy loops in the kernels' stated order by the script's own run(): every target's slab shares, y_t'y_t and,
with p = 1 too, H, H2 and Bs in the one order that the handle's own y has as well.  The program
is built once per module; the cases are the script's whole list.  A case fails on a non-zero exit, on anything a sanitizer
writes to stderr, and on any differing bit."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import host_check  # noqa: E402
import sparse_targets_host_check  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists(host_check.CLANG), reason="no host compiler at " + host_check.CLANG)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("sparse_targets"))
    return host_check.build("sparse_targets_host_check", tmp), tmp


def test_the_list_covers_the_shapes():
    cases = sparse_targets_host_check.CASES
    assert {c[0] for c in cases} == {1, 3, 9, 17}                       # one target, one group, a second and a third of one target
    assert {(c[1] + 127) // 128 * 128 for c in cases} == {128, 256}     # mpad
    assert any(c[2] < c[3] for c in cases) and any(c[2] == c[3] for c in cases)      # a ragged chunk, a full one
    assert any(c[1] % 128 for c in cases) and any(c[1] % 128 == 0 for c in cases)    # columns to mask, none
    assert any(c[3] > 128 for c in cases)                               # more than one slab


@pytest.mark.parametrize("case", sparse_targets_host_check.CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_sparse_targets(program, capfd, case):
    exe, tmp = program
    ok = sparse_targets_host_check.run(exe, tmp, *case)
    line = capfd.readouterr().out
    print(line, end="")
    assert ok and "BAD" not in line and "FAILED" not in line and "NOT" not in line, line
    assert line.rstrip().endswith("ok"), line
