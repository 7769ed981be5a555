"""CPU check of the multi-target truth and yardstick (tests/truth_targets.py): an fp64 stand-in of exactly the fused
formulation -- LAPACK Cholesky, Z = Y T', A = Z T, W = m K^-1 - A'A -- stays within the families' existing factors at
the listed cases, with room (at most half the factor: the project's factor rule asks for no new one).  This pins the
truth, the yardstick and the case choice that tests/test_gpu_targets.py leans on, without a GPU.
The ratios are those of the BLAS this runs on."""
import numpy as np
import pytest

import truth
import truth_targets as tt

pytestmark = pytest.mark.skipif(not truth.EXTENDED, reason="numpy.longdouble is not an extended-precision type here")


def test_targets_are_nested_and_start_with_y():
    y = np.linspace(-1.0, 2.0, 65)
    Y3, Y17 = tt.targets(y, 3), tt.targets(y, 17)
    assert Y3.shape == (3, 65) and Y17.shape == (17, 65)
    assert np.array_equal(Y3[0], y) and np.array_equal(Y17[:3], Y3)


def test_truth_of_one_target_is_the_single_target_truth(oracle):
    c = tt.case(oracle, "se", "n65", 3)
    t, one = c["t"], tt.truth_of(c["t"], c["Y"][:1], c["Xt"])
    assert float(abs(one["ll"] - t.ll) / abs(t.ll)) < 1e-17
    assert float(np.max(np.abs(one["grad"] - t.grad)) / np.max(np.abs(t.grad))) < 1e-16
    assert float(np.max(np.abs(one["A"][0] - t.alpha)) / np.max(np.abs(t.alpha))) < 1e-17
    assert float(np.max(np.abs(one["mean"][:, 0] - t.predict(c["Xt"])[0]))) < 1e-17 * float(np.max(np.abs(one["mean"])))


@pytest.mark.parametrize("family, name, m", tt.STANDIN_CASES, ids=["%s-%s-m%d" % c for c in tt.STANDIN_CASES])
def test_standin_stays_within_the_family_factor(oracle, family, name, m):
    c = tt.case(oracle, family, name, m)
    r = tt.standin_ratios(c)
    print("STANDIN-TARGETS %-9s %-13s m %3d  " % (family, name, m) + "  ".join("%s %.2f" % kv for kv in r.items()))
    cov = c["cov"]
    for q in cov.quantities[:4] + ("mean",):          # the yardstick is sane (accuracy.assert_yardstick_is_sane's cap)
        assert c["noise"][q] <= truth.YARDSTICK_CAP * c["floor"][q] / truth.U4, (q, c["noise"][q])
    assert max(r.values()) <= cov.F, (r, cov.F)
