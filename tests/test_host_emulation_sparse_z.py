"""The host check of the inducing-input gradient's kernels as a test, without a GPU: cugp_amd/csrc/sparse_z_device.h -- the
text kernels.hip compiles for gfx950 -- runs behind tools/host_emul.h as 256 host threads per workgroup in a stand-alone
program built with -fsanitize=address,undefined (tools/sparse_z_host_check.cpp; nothing is loaded into Python, nothing
preloaded), on exact-size heap buffers with NaN where the kernels must not read, and is compared by the script's own run():
bit for bit with a plain double loop in the kernels' summation order, and with the formula in numpy.  The program is built
once per module; the cases are the script's whole list (a ragged chunk with the rank-one part and the square in every case;
d = 2, 3, 6 and 17; one and two row ranges per column tile, four on the square, ragged ranges of 5, 5, 4 and 5, 5, 5, 5, 2 tiles; SE, Matern 3/2 and 5/2, SE-ARD with two
feature chunks, Matern-5/2-ARD).  A case fails on a non-zero exit, on anything a sanitizer writes to stderr, and on a
result that differs."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import host_check  # noqa: E402
import sparse_z_host_check  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists(host_check.CLANG), reason="no host compiler at " + host_check.CLANG)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("sparse_z"))
    return host_check.build("sparse_z_host_check", tmp), tmp


def test_the_list_covers_the_shapes_and_families():
    import truth_sparse_z as tz
    cases = sparse_z_host_check.CASES
    assert {tz.CASES[c[0]][0] for c in cases} == {"se", "matern32", "matern52", "ard", "matern52_ard"}
    assert {tz.CASES[c[0]][3] for c in cases} >= {3, 17}                       # one feature chunk, two
    assert {c[2] for c in cases} >= {1, 2} and {c[3] for c in cases} >= {1, 2}  # one and two row ranges per column tile
    assert {c[1] for c in cases} >= {None, 1, 200}                              # ragged chunks; 200 rows: two tiles per range
    assert {tz.CASES[c[0]][2] for c in cases} >= {64, 65, 128, 130, 200}        # padding beyond column m, none, two column tiles
    # the default chunk's ragged row ranges: 14 tiles in 3 ranges (5, 5, 4); 22 in 5 (5, 5, 5, 5, 2) with six column tiles
    assert sparse_z_host_check.CASES_DEFAULT_CHUNK == (("se_n800_m65_d3_c0", None, 3, 1), ("se_n1300_m260_c0", None, 5, 3))
    assert tz.z_ranges(896, 128, 3) == [5, 5, 4] and tz.z_ranges(1408, 384, 6) == [5, 5, 5, 5, 2]


@pytest.mark.parametrize("case", sparse_z_host_check.CASES + sparse_z_host_check.CASES_DEFAULT_CHUNK, ids=lambda c: "-".join(str(v) for v in c))
def test_sparse_z(program, capfd, case):
    exe, tmp = program
    ok = sparse_z_host_check.run(exe, tmp, *case)
    line = capfd.readouterr().out
    print(line, end="")
    assert ok and "BAD" not in line and "FAILED" not in line and "DIFFERENT" not in line, line
    assert line.rstrip().endswith("ok"), line
