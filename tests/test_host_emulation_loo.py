"""The host check of the leave-one-out kernels as a test, without a GPU: cugp_amd/csrc/loo_device.h -- the text kernels.hip
compiles for gfx950 -- runs behind tools/host_emul.h as 256 host threads per workgroup in a stand-alone program built with
-fsanitize=address,undefined (tools/loo_host_check.cpp; nothing is loaded into Python, nothing preloaded), on exact-size
heap buffers with NaN where the kernels must not read, and is compared with numpy by the script's own run(): per-point
outputs, B and L_LOO to 4 ulp of scale, b and the gradient to 1e-13, the padding exact zeros.  The program is built once
per module; the cases are the script's whole list (npad 128, 256, 384; n = 1, 2, 63, 64, 65, 128, 129, 257, 300; SE,
Matern 5/2, SE-ARD, Matern-3/2-ARD).  A case fails on a non-zero exit, on anything a sanitizer writes to stderr, and on a result beyond its
tolerance."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import host_check  # noqa: E402
import loo_host_check  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists(host_check.CLANG), reason="no host compiler at " + host_check.CLANG)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("loo"))
    return host_check.build("loo_host_check", tmp), tmp


def test_the_list_covers_the_sizes_and_families():
    import truth_loo as tl
    sizes = set()
    for family, name, rows in loo_host_check.CASES:
        n = rows if rows is not None else len(tl.inputs(family, name)[1])
        sizes.add((n, (n + 127) // 128 * 128))
    assert {n for n, _ in sizes} == {1, 2, 63, 64, 65, 128, 129, 257, 300}
    small = {(f, rows) for f, _, rows in loo_host_check.CASES if rows is not None and rows <= 64}
    assert small == {("se", 1), ("se", 2), ("se", 63), ("se", 64), ("ard", 2), ("ard", 63), ("matern52", 2), ("matern52", 63)}
    assert {p for _, p in sizes} == {128, 256, 384}
    assert {f for f, _, _ in loo_host_check.CASES} == {"se", "matern52", "ard", "matern32_ard"}


@pytest.mark.parametrize("case", loo_host_check.CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_loo(program, capfd, case):
    exe, tmp = program
    ok = loo_host_check.run(exe, tmp, *case)
    line = capfd.readouterr().out
    print(line, end="")
    assert ok and "BAD" not in line and "FAILED" not in line, line
    assert line.rstrip().endswith("ok"), line
