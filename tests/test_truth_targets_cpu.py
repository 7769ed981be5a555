"""CPU check of the multi-target truth and yardstick (tests/truth_targets.py): an fp64 stand-in of exactly the fused
formulation -- LAPACK Cholesky, Z = Y T', A = Z T, W = m K^-1 - A'A -- stays within the families' existing factors at
the listed cases, with room (at most half the factor: the project's factor rule asks for no new one).  This pins the
truth, the yardstick and the case choice that tests/test_gpu_targets.py leans on, without a GPU.
The same for the cases beyond one test tile (WIDE_CASES, held to half the factor; the subset yardstick against a wider one;
two mutations of the means' indexing that must leave the bound) and for targets set on a handle that cugp_append has grown
(standin_grown, held to half of truth_append.F_APPEND).
The ratios are those of the BLAS this runs on."""
import numpy as np
import pytest

import truth
import truth_append as ta
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


# ------------------------------------------------------------------ beyond one test tile
def yardstick_is_capped(c):
    for q in c["cov"].quantities[:4] + ("mean",):     # (a subset case: its own, smaller, yardsticks)
        assert c["noise"][q] <= truth.YARDSTICK_CAP * c["floor"][q] / truth.U4, (q, c["noise"][q])


@pytest.mark.parametrize("case", tt.WIDE_CASES, ids=[tt.wide_id(c) for c in tt.WIDE_CASES])
def test_wide_standin_stays_within_half_the_family_factor(oracle, case):
    """The wide cases of tests/test_gpu_targets.py: every held quantity of the stand-in within HALF the family's factor
    (LL, the gradient and LL_t do not depend on the test points; they are held again at these nt all the same)."""
    c = tt.wide_case(oracle, *case)
    r = tt.standin_ratios(c)
    print("STANDIN-TARGETS-WIDE %-9s %-9s m %3d nt %3d %-7s " % (case[:4] + ("subset" if case[4] else "",))
          + "  ".join("%s %.2f" % kv for kv in r.items()))
    assert set(r) == set(tt.held(c)) and (case[4] is None or set(r) == {"mean"})
    assert c["Xt"].shape[0] == case[3] and np.array_equal(c["Xt"][-2], c["X"][len(c["X"]) // 2])
    yardstick_is_capped(c)
    assert max(r.values()) <= c["cov"].F / 2, (r, c["cov"].F)


def test_subset_yardstick_is_no_larger_than_a_wider_one(oracle):
    """n515_d33, m = 65: the yardstick of the means over the subset (0, 1, 63, 64) against the one over eight targets that
    include them.  The evaluator runs target by target, so the second is a maximum over more columns of the same numbers."""
    case = [c for c in tt.WIDE_CASES if c[4]][0]
    family, name, m, nt, subset = case
    c = tt.wide_case(oracle, *case)
    eight = tuple(sorted(set(subset) | {2, 17, 33, 48}))
    assert len(eight) == 8 and max(eight) < m
    noise8, floor8 = tt.subset_yardstick(oracle, c, c["Y"], c["Xt"], eight)
    print("SUBSET-YARDSTICK %s mean: 4 targets %.3e (floor %.3e)  8 targets %.3e (floor %.3e)"
          % (name, c["noise"]["mean"], c["floor"]["mean"], noise8["mean"], floor8["mean"]))
    assert c["noise"]["mean"] <= noise8["mean"] and c["floor"]["mean"] <= floor8["mean"]


@pytest.mark.parametrize("mutate", ["drop_chunk2", "swap_tiles"])
def test_wide_mutations_leave_the_bound(oracle, mutate):
    """n515_d33 (npad 640: k chunks [0, 512) and [512, 640)), m = 65, nt = 129: the stand-in's means with the second k
    chunk dropped, and with the test rows [0, 64) and [64, 128) swapped.  Either leaves F yardsticks: the case has teeth
    for exactly the faults its grid can have."""
    case = [c for c in tt.WIDE_CASES if c[4]][0]
    c = tt.wide_case(oracle, *case)
    assert c["X"].shape[0] > 512
    r = tt.standin_ratios(c, mutate)
    print("MUTATION-TARGETS-WIDE %-12s mean ratio %.3g (F %d)" % (mutate, r["mean"], c["cov"].F))
    assert r["mean"] > c["cov"].F, (mutate, r)


# ------------------------------------------------------------------ targets on a grown handle
def test_grown_standin_stays_within_half_of_F_APPEND(oracle):
    """cugp_set_targets after cugp_append (tests/test_gpu_targets.py: test_targets_on_a_grown_handle): T, K^-1 and log|K|
    of truth_append.standin_append's bordering fed into the multi-target formulas, against the case on all rows."""
    (family, name, n0, chunks), m = tt.GROWN_CASE
    assert (family, name, n0, chunks) in ta.CASES
    c = tt.case(oracle, family, name, m)
    out = tt.standin_grown(c["cov"], c["X"], c["Y"], c["Xt"], n0, chunks)
    r = tt.ratios(c, *out[:4], A=out[4])
    print("STANDIN-TARGETS-GROWN %-9s %-9s m %3d  %d+%s  " % (family, name, m, n0, "+".join(map(str, chunks)))
          + "  ".join("%s %.2f" % kv for kv in r.items()))
    yardstick_is_capped(c)
    alpha = r.pop("alpha")
    assert max(r.values()) <= ta.F_APPEND[family] / 2, r
    assert alpha <= ta.F_SOLVE / 2, alpha
