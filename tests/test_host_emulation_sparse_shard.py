"""The host check of the sharded sparse model's kernels as a test, without a GPU: cugp_amd/csrc/sparse_shard_device.h -- the
text kernels.hip compiles for gfx950 -- runs behind tools/host_emul.h as 256 host threads per workgroup in a stand-alone
program built with -fsanitize=address,undefined (tools/sparse_shard_host_check.cpp; nothing is loaded into Python, nothing
preloaded), on exact-size heap buffers with NaN where the kernels must not read, and is compared by the script's own run()
bit for bit with plain loops: k_sparse_shard_reduce over gathered blocks whose shards interleave over the ranks and leave
slots empty -- what one GPU cannot run --, k_sparse_shard_sums below, at and beyond a wave's 64 lanes, and
k_sparse_finalize_sharded against k_sparse_finalize_targets' formulas at p = 1.  The program is built once per module.  A
case fails on a non-zero exit, on anything a sanitizer writes to stderr, and on a result that differs."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import host_check  # noqa: E402
import sparse_shard_host_check as shc  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists(host_check.CLANG), reason="no host compiler at " + host_check.CLANG)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("sparse_shard"))
    return host_check.build("sparse_shard_host_check", tmp), tmp


def test_the_list_covers_the_layouts():
    from cugp_amd.bcm import gather_row_index
    cases = shc.CASES
    assert {c[:3] for c in cases} >= {(5, 2, 3), (3, 1, 5), (1, 1, 1), (8, 8, 1), (9, 8, 2)}
    assert {c[3] for c in cases if c[:3] in ((5, 2, 3), (3, 1, 5))} == {128, 256}      # the slot's shape at both
    assert {c[5] for c in cases} >= {1, 63, 64, 65, 200}                                # nb_uf around a wave's 64 lanes
    assert {c[4] for c in cases} == {"P", "tail"} and {c[8] for c in cases} == {0, 1}
    for K, W, per in {c[:3] for c in cases}:                                            # the slot map is bcm.py's
        assert per * W >= K
        for k in range(K):
            r, s = shc.slot_of(k, W, per)
            assert r * per + s == gather_row_index(k, W, per)
    assert any(c[2] * c[1] > c[0] for c in cases)                                       # an empty slot
    with open(os.path.join(ROOT, "cugp_amd", "csrc", "handle.h")) as f:
        assert "constexpr int SHARD_HDR = %d;" % shc.HDR in f.read()


@pytest.mark.parametrize("case", shc.CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_sparse_shard(program, capfd, case):
    exe, tmp = program
    ok = shc.run(exe, tmp, *case)
    line = capfd.readouterr().out
    print(line, end="")
    assert ok and "BAD" not in line and "FAILED" not in line and "DIFFERENT" not in line, line
    assert line.rstrip().endswith("ok"), line
