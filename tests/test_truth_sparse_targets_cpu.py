"""The CPU counterpart of tests/test_gpu_sparse_targets.py: everything its accuracy bound rests on, without a GPU.

  - the truth's F (ONE N x N factor, a forward substitution per target) equals the sum of truth_sparse.Truth(...).F over the
    targets, and its F_t, gradient and means the per-target truths', on the two smallest cases
  - the truth's gradient (shared Kuu^-1 and Sigma^-1, beta_t per target, summed G) against longdouble central differences
    of the definition, in theta and in Z
  - the stand-in -- the fused formulation of include/cugp.h in cugp_sparse_plan's chunks -- within F_SPARSE_TARGETS
    (F_SPARSE_TARGETS_Z for gZ) of the yardstick, truth_sparse.computed_form per target summed in target order; the factors
    follow truth.factor_rule of the ratios measured here
  - two mutations leave the bound: H with p left out (I - B^-1 once), the rank-p part of the weights for target 0 only
"""
import numpy as np
import pytest

import truth
import truth_sparse as ts
import truth_sparse_targets as tst
import truth_sparse_z as tz

LD = truth.LD
pytestmark = pytest.mark.skipif(not truth.EXTENDED, reason="numpy.longdouble is not an extended-precision type here")
NAMES = [n for n, _ in tst.CASES]
SMALLEST = ["se_n128_m128", "se_n300_m65"]


def test_the_cases_are_the_issues():
    assert tst.CASES == (("se_n128_m128", 1), ("se_n300_m65", 3), ("se_n1300_m200", 17), ("ard_n300_m130_d17", 5),
                         ("matern32_ard_n1000_m130", 9), ("matern52_n800_m65_d3_c0", 2), ("se_n300_dup60", 3))
    assert all(n in ts.CASES for n in NAMES)
    Y3, Y17 = tst.targets("se_n300_m65", 3), tst.targets("se_n300_m65", 17)
    assert np.array_equal(Y17[:3], Y3) and np.array_equal(Y3[0], ts.inputs("se_n300_m65")[1])


@pytest.mark.parametrize("name", SMALLEST)
def test_truth_is_the_sum_of_the_single_target_truths(name):
    c = tst.case(name)
    X, Z, cov, t = c["X"], c["Z"], c["cov"], c["t"]
    F, g, gz = LD(0), 0, 0
    for k, y in enumerate(c["Y"]):
        one = ts.Truth(X, y, Z, cov)
        F, g, gz = F + one.F, g + one.grad, gz + tz.truth_gz(X, y, Z, cov)
        assert abs(one.F - t.F_each[k]) <= 1e-17 * abs(one.F)
        assert np.max(np.abs(one.predict(c["Xt"])[0] - c["tm"][k])) <= 1e-16 * np.max(np.abs(c["tm"]))
        assert np.max(np.abs(one.predict(c["Xt"])[1] - c["tv"])) <= 1e-17
    print("SUM %-16s F %.3e grad %.3e gZ %.3e" % (name, float(abs(F - t.F) / abs(F)),
                                                  float(np.max(np.abs(g - t.grad)) / np.max(np.abs(g))),
                                                  float(np.max(np.abs(gz - t.gz)) / np.max(np.abs(gz)))))
    assert F == t.F                                            # the same per-target values added in the same order
    assert np.max(np.abs(g - t.grad)) <= 1e-15 * np.max(np.abs(g))
    assert np.max(np.abs(gz - t.gz)) <= 1e-13 * np.max(np.abs(gz))      # (|gZ| is cancellation on se_n128_m128: Z is all the data)


@pytest.mark.parametrize("name", ["se_n300_m65", "ard_n300_m130_d17"])
def test_truth_gradient_against_central_differences(name):
    """test_truth_sparse_cpu's procedure on sum_t F_t (a whole factorisation per target and probe: N = 300 only)."""
    c = tst.case(name)
    X, Y, Z, cov, t = c["X"], c["Y"], c["Z"], c["cov"], c["t"]
    make = truth.FAMILIES[ts.CASES[name][0]][1]
    h = 1e-6
    worst = 0.0
    comps = range(len(cov.hp)) if len(cov.hp) == 3 else (0, len(cov.hp) - 3, len(cov.hp) - 2, len(cov.hp) - 1)
    for j in comps:
        f = []
        for sgn in (1, -1):
            cc = make(list(cov.hp))
            th = LD(cov.hp[j]) + sgn * LD(h)
            if hasattr(cc, "w") and j < len(cc.w):
                cc.w[j] = np.exp(-th)
            elif j == len(cov.hp) - 2:
                cc.sf2 = np.exp(2 * th)
            elif j == len(cov.hp) - 1:
                cc.sn2 = np.exp(2 * th)
            else:
                cc.l2 = np.exp(2 * th)
            f.append(tst.bound_sum_definition(X, Y, Z, cc))
        cd = -(f[0] - f[1]) / (2 * LD(h))
        worst = max(worst, float(abs(cd - t.grad[j]) / np.max(np.abs(t.grad))))
    # two entries of Z: the first point's first coordinate, the last point's last
    wz = 0.0
    for (j, k) in ((0, 0), (Z.shape[0] - 1, Z.shape[1] - 1)):
        f = []
        for sgn in (1, -1):
            Zl = Z.astype(LD)
            Zl[j, k] = Zl[j, k] + sgn * LD(h)
            F = LD(0)
            for y in Y:
                F = F + _bound_at(X, y, Zl, cov)
            f.append(F)
        cd = -(f[0] - f[1]) / (2 * LD(h))
        wz = max(wz, float(abs(cd - t.gz[j, k]) / np.max(np.abs(t.gz))))
    print("CD %-24s theta %.2e  Z %.2e" % (name, worst, wz))
    assert worst <= 1e-9 and wz <= 1e-8


def _bound_at(X, y, Zl, cov):
    """truth_sparse.bound_definition with Z already in longdouble (it casts through fp64, which would round the probe)."""
    Xl, yl = np.asarray(X, dtype=np.float64).astype(LD), np.asarray(y, dtype=np.float64).astype(LD)
    N, M = len(yl), len(Zl)
    Kuu = ts.kernel_parts(cov, Zl, Zl)[0]
    Kuu[np.arange(M), np.arange(M)] += LD(ts.JITTER)
    Kuf = ts.kernel_parts(cov, Zl, Xl)[0]
    A0 = truth._mm(truth.tri_inverse(truth.cholesky(Kuu)), Kuf)
    Qff = truth._mm(np.ascontiguousarray(A0.T), A0)
    Cm = Qff.copy()
    Cm[np.arange(N), np.arange(N)] += cov.sn2
    LC = truth.cholesky(Cm)
    z = ts.forward(LC, yl)
    return -N * ts.LOG2PI / 2 - np.log(np.diag(LC)).sum() - z @ z / 2 - (N * cov.sf2 - np.trace(Qff)) / (2 * cov.sn2)


_RATIOS = {}


def standin_ratios(name):
    if name not in _RATIOS:
        c = tst.case(name)
        _RATIOS[name] = tst.ratios(c, tst.standin(c["cov"], c["X"], c["Y"], c["Z"], c["Xt"], c["chunk"]))
    return _RATIOS[name]


@pytest.mark.parametrize("name", NAMES)
def test_standin_within_the_bound(name):
    c = tst.case(name)
    r = standin_ratios(name)
    print("STANDIN-TARGETS %-24s p %-2d " % (name, c["p"]) + "  ".join("%s %.2f" % kv for kv in r.items())
          + "  | yardstick " + " ".join("%s %.1e" % (q, max(c["noise"][q], c["floor"][q])) for q in r))
    for q, v in r.items():
        assert v <= tst.factor(c, q), (q, v)


def test_factors_follow_the_rule():
    worst, worst_z = {}, {}
    for name in NAMES:
        fam = ts.CASES[name][0]
        r = dict(standin_ratios(name))
        worst_z[fam] = max(worst_z.get(fam, 0.0), r.pop("gZ"))
        worst[fam] = max(worst.get(fam, 0.0), max(r.values()))
    for fam in worst:
        rule, rule_z = truth.factor_rule(worst[fam]), truth.factor_rule(worst_z[fam])
        print("F_SPARSE_TARGETS %-12s largest stand-in ratio %.2f (gZ %.2f)  factor_rule %d (gZ %d)  F_SPARSE %d  "
              "F_SPARSE_TARGETS %d  F_SPARSE_TARGETS_Z %d" % (fam, worst[fam], worst_z[fam], rule, rule_z, ts.F_SPARSE[fam],
                                                            tst.F_SPARSE_TARGETS[fam], tst.F_SPARSE_TARGETS_Z[fam]))
        assert rule <= tst.F_SPARSE_TARGETS[fam] and rule_z <= tst.F_SPARSE_TARGETS_Z[fam], (fam, worst[fam], worst_z[fam])
        assert tst.F_SPARSE_TARGETS[fam] >= ts.F_SPARSE[fam] and tst.F_SPARSE_TARGETS_Z[fam] >= tz.F_SPARSE_Z[fam]


@pytest.mark.parametrize("mutate", tst.MUTATIONS)
@pytest.mark.parametrize("name", ["se_n300_m65", "ard_n300_m130_d17"])
def test_mutations_leave_the_bound(name, mutate):
    """H with p left out and the rank-p part for target 0 only both move the gradient (and gZ) far beyond the bound."""
    c = tst.case(name)
    r = tst.ratios(c, tst.standin(c["cov"], c["X"], c["Y"], c["Z"], c["Xt"], c["chunk"], mutate=mutate))
    lead = c["cov"].quantities[1]
    print("MUTATION-TARGETS %-24s %-14s %s ratio %.3g  gZ ratio %.3g" % (name, mutate, lead, r[lead], r["gZ"]))
    assert r[lead] > 1000 * tst.F_SPARSE_TARGETS[c["family"]]
    assert r["gZ"] > 1000 * tst.F_SPARSE_TARGETS_Z[c["family"]]
    assert r[c["cov"].quantities[0]] <= tst.F_SPARSE_TARGETS[c["family"]]        # (F itself does not read them)
