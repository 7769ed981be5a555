"""The hand-over block of a lone handle (TUNE_PIPE_BLOCK, default by size: cugp_pipe_block_for) moves block boundaries
and with them summation orders in K^-1 and the gradient: every block size the rule can return is held to fp64
ROUNDING at 3200 rows (25 tiles: each of them leaves at least two blocks) against the committed extended-precision
truth -- the harness and the factors of tests/accuracy.py, the fixture of tests/golden/make_truth_n3200.py.  Equal
bits are NOT expected between block sizes.
"""
import sys

import pytest

import accuracy
import truth
from accuracy import Report
from conftest import GOLDEN
from cugp_amd import capi

sys.path.insert(0, GOLDEN)
import make_truth_n3200  # noqa: E402

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not truth.EXTENDED, reason="numpy.longdouble is not an extended-precision type here")]

PIPE_BLOCK = 3                                 # kernels.h TUNE_PIPE_BLOCK
NT_MAX = 160


def test_every_block_size_of_the_rule_at_3200_rows():
    import cugp_amd.gp as gp
    lib = capi.lib()
    sizes = sorted({lib.cugp_pipe_block_for(nt) for nt in range(1, NT_MAX + 1)})
    assert sizes and sizes[0] >= 1 and sizes[-1] <= 16, sizes
    X, y, Xt, cov, _ = make_truth_n3200.inputs()
    f = make_truth_n3200.load()                # a missing fixture fails, it does not skip
    assert (len(y) + 127) // 128 == 25

    def handle(w):
        g = gp.Covsum(*X.shape)
        g.set_tuning(PIPE_BLOCK, w)
        assert g.get_tuning(PIPE_BLOCK) == w
        g.set_loghyperparam(cov.hp)
        return g

    for w in sizes:
        accuracy.hold_fixture_case(Report("n3200_block%d" % w, cov), f, X, y, Xt, cov, lambda: handle(w))
