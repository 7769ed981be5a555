"""CPU checks of the ARD x Matern truth (truth.Truth with truth_ard_matern.ARDMatern), of its yardstick, of the factor it is
held to (truth.F_ARD, unchanged) and of the K-entry bound -- everything tests/test_gpu_ard_matern.py leans on.

  1. the truth's gradient against a central difference of its LL in longdouble: the independent check of H;
  2. equal length scales reproduce truth.Matern's truth to longdouble rounding;
  3. the stand-in within the rule: truth.factor_rule(largest ratio) <= F_ARD over the case list, both kinds; 2 x the
     largest alpha / K^-1 ratio <= F_SOLVE; every yardstick sane;
  4. the kernels' per-entry arithmetic, restated in fp64 numpy, inside the derived K-entry bound, and its extremes;
  5. two mutations leave their bounds: Kf in place of H in g_c (the gradient's F_ARD yardsticks), the isotropic a with
     l^2 = 1 and the weights ignored (the K-entry bound).
"""
import numpy as np
import pytest

import accuracy
import truth
import truth_ard_matern as tam
import truth_matern as tm
from conftest import synth

pytestmark = pytest.mark.skipif(not truth.EXTENDED, reason="numpy.longdouble is not an extended-precision type here")

LD = truth.LD


@pytest.mark.parametrize("kind", tam.KINDS)
def test_gradient_is_the_derivative_of_ll(kind):
    """grad_k = d(-LL)/d theta_k by a central difference in longdouble, every one of the d + 2 components; step and
    tolerance as tests/test_truth_matern_cpu.py derives them (h = 2^-20, 100 (h^2 + eps_LD / h |LL| / max|g|))."""
    n, d = 40, 3
    X, y = synth(n, d=d, seed=n, scale=4.0)
    hp = [0.9, 0.3, 1.6, 0.3, -1.0]
    h = 2.0 ** -20
    t = truth.Truth(X, y, tam.ARDMatern(hp, kind))
    gs = np.max(np.abs(t.grad))
    tol = 100 * (h * h + truth.EPS_LD / h * float(abs(t.ll) / gs))
    for k in range(d + 2):
        lo, hi = list(hp), list(hp)
        lo[k], hi[k] = hp[k] - h, hp[k] + h
        num = (truth.Truth(X, y, tam.ARDMatern(lo, kind)).ll - truth.Truth(X, y, tam.ARDMatern(hi, kind)).ll) / (LD(hi[k]) - LD(lo[k]))
        err = float(abs(num - t.grad[k]) / gs)
        print("kind %d g%d: formula %.15g, central difference %.15g, |diff| / max|g| %.3e (tolerance %.3e)"
              % (kind, k, float(t.grad[k]), float(num), err, tol))
        assert err <= tol, (kind, k, err, tol)


@pytest.mark.parametrize("kind", tam.KINDS)
def test_equal_length_scales_are_the_isotropic_matern(kind):
    """theta_c = theta_0 for every c: the same model as truth.Matern at [theta_0, theta_f, theta_n].  LL, the signal and
    noise components, the prediction, and sum_c g_c = g0 (sum_c H u_c^2 = dk/dtheta_0), to longdouble rounding: the two
    differ in the order of weighting and summing (x w)^2 against x^2 / l^2 -- 1e3 eps_LD relative covers the ~n roundings
    per entry and the conditioning of the solve (n = 60, cond(K) ~ 1e3)."""
    n, d = 60, 3
    X, y = synth(n, d=d, seed=n, scale=4.0)
    Xt = synth(9, d=d, seed=7, scale=4.0)[0]
    iso = [0.9, 0.3, -1.0]
    ta = truth.Truth(X, y, tam.ARDMatern([iso[0]] * d + iso[1:], kind))
    ti = truth.Truth(X, y, truth.Matern(iso, kind))
    tol = 1e3 * truth.EPS_LD
    gs = np.max(np.abs(ti.grad))
    assert abs(ta.ll - ti.ll) <= tol * abs(ti.ll)
    assert abs(ta.grad[:d].sum() - ti.grad[0]) <= tol * gs
    assert np.all(np.abs(ta.grad[d:] - ti.grad[1:]) <= tol * gs)
    (ma, va), (mi, vi) = ta.predict(Xt), ti.predict(Xt)
    assert np.all(np.abs(ma - mi) <= tol * np.max(np.abs(mi))) and np.all(np.abs(va - vi) <= tol * (ti.sf2 + ti.sn2))


@pytest.fixture(scope="module")
def table(oracle):
    """Stand-in ratios and yardsticks of every case and kind -- computed once."""
    out = {}
    for name, kind in tam.CASES:
        c = out[name, kind] = tam.live(oracle, name, kind)
        ratio, rs = accuracy.standin_ratios(c)
        print("STANDIN-ARD-MATERN %-13s %-8s " % (name, tam.KIND_NAMES[kind])
              + "  ".join("%s %.2f" % kv for kv in list(ratio.items()) + list(rs.items()))
              + "  | yardstick " + " ".join("%s %.1e" % kv for kv in c["noise"].items()))
    return out


def test_case_list_is_ard_cases_at_both_kinds():
    assert tam.CASES == tuple((n, k) for n in truth.ARD_CASES for k in (truth.MATERN32, truth.MATERN52))
    for name, kind in tam.CASES:
        X, y, Xt, cov = tam.inputs(name, kind)
        Xa, ya, Xta, hpa = truth.ard_inputs(name)
        assert np.array_equal(X, Xa) and np.array_equal(y, ya) and np.array_equal(Xt, Xta) and cov.hp == hpa
        assert cov.kind == kind and cov.F == truth.F_ARD and cov.quantities == truth.QUANTITIES_ARD


def test_standin_within_the_rule(table):
    """The project's rule (docs/ACCURACY.md, "The bound") over the case list, both kinds, asks for no more than the
    existing F_ARD; F_SOLVE covers alpha and K^-1.  The ratios are those of the BLAS this runs on."""
    worst = max(max(accuracy.standin_ratios(c)[0].values()) for c in table.values())
    worst_solve = max(max(accuracy.standin_ratios(c)[1].values()) for c in table.values())
    rule = truth.factor_rule(worst)
    print("largest stand-in ratio %.2f -> factor by the rule %d (F_ARD %d); alpha / K^-1 %.2f (F_SOLVE %d)"
          % (worst, rule, truth.F_ARD, worst_solve, truth.F_SOLVE))
    assert rule <= truth.F_ARD, (worst, rule, truth.F_ARD)
    assert 2 * worst_solve <= truth.F_SOLVE, (worst_solve, truth.F_SOLVE)


def test_yardsticks_are_sane(table):
    for key, c in table.items():
        accuracy.assert_yardstick_is_sane(c, key)


@pytest.mark.parametrize("kind", tam.KINDS)
def test_fp64_entry_formula_inside_the_bound(kind):
    """truth_ard_matern.entry_fp64 on wsqdist64 (the kernels' order of operations) against the longdouble kernel function
    on every case's K and k_test, entry by entry, inside k_entry_bound (derived beside K_BOUND in truth_ard_matern.py:
    (7 + 1/2 (1 + a) (d + 14)) u and (10 + (1 + a) (d + 14)) u).  H is held to the same count (its polynomial has fewer
    roundings than Kf's)."""
    assert tam.K_BOUND == {tam.MATERN32: (7.0, 0.5, 14.0), tam.MATERN52: (10.0, 1.0, 14.0)}
    worst = worst_h = 0.0
    for name in truth.ARD_CASES:
        X, y, Xt, cov = tam.inputs(name, kind)
        c64 = cov.fp64()
        d = X.shape[1]
        for A in (X, Xt):
            tk, th = tam.parts(truth.wsqdist(A.astype(LD), X.astype(LD), cov.w), cov.sf2, kind)
            kf, hh = tam.entry_fp64(tam.wsqdist64(A, X, c64.w), float(c64.sf2), kind)
            bound = tam.k_entry_bound(tam.a_of(A, X, cov), d, kind)
            assert float(tk.min()) > 1e-290
            rk, rh = np.abs(kf.astype(LD) - tk) / tk, np.abs(hh.astype(LD) - th) / th
            worst, worst_h = max(worst, float(np.max(rk / bound))), max(worst_h, float(np.max(rh / bound)))
            assert np.all(rk <= bound) and np.all(rh <= bound), (name, kind, float(np.max(rk / bound)), float(np.max(rh / bound)))
            assert tam.entry_excess(kf, A, X, cov) <= 1.0
    print("kind %d: largest |fp64 entry - truth| / bound: Kf %.3f, H %.3f" % (kind, worst, worst_h))


@pytest.mark.parametrize("kind", tam.KINDS)
def test_fp64_entry_extremes(kind):
    """s = 0 gives sf2 exactly and H = 3 sf2 | RN(5/3) sf2; s = +inf and a finite a whose exp underflows give exactly 0 for
    both, no NaN."""
    sf2 = 1.37
    kf, hh = tam.entry_fp64(np.array([0.0, 1.0, 1e6, 1e300, np.inf]), sf2, kind)
    assert kf[0] == sf2 and hh[0] == sf2 * (3.0 if kind == tam.MATERN32 else tam.FIVE_THIRDS)
    assert 0 < kf[1] < sf2 and hh[1] > 0
    assert np.all(kf[2:] == 0.0) and np.all(hh[2:] == 0.0)
    assert not np.any(np.isnan(kf)) and not np.any(np.isnan(hh))


@pytest.mark.parametrize("kind", tam.KINDS)
def test_mutation_kf_for_h_leaves_the_gradient_bound(kind, oracle):
    """g_c = 1/2 sum W o Kf o u_c^2 (SE-ARD's form: Kf where H belongs) in the stand-in: some g_c leaves F_ARD yardsticks,
    while LL and the other components, which do not read H, stay inside."""
    c = tam.live(oracle, "n65_d2", kind)
    st = truth.standin(tam._Mutated(c["cov"].hp, kind, "kf_for_h"), c["X"], c["y"], c["Xt"])
    e = truth.errors(c["cov"], *st, c["t"].ll, c["t"].grad, c["tm"], c["tv"])
    r = {q: e[q] / max(c["noise"][q], c["floor"][q]) for q in c["cov"].quantities}
    print("kf_for_h kind %d: " % kind + "  ".join("%s %.3g" % kv for kv in r.items()))
    assert r["gc"] > truth.F_ARD
    assert all(r[q] <= truth.F_ARD for q in ("ll", "gf", "gn", "mean", "var"))


@pytest.mark.parametrize("kind", tam.KINDS)
def test_mutation_ignored_weights_leaves_the_entry_bound(kind):
    """The isotropic entry with l^2 = 1 on the UNWEIGHTED distance (truth_matern.entry_fp64: what a launch of the isotropic
    Matern kernels on an ARD handle would compute) leaves the K-entry bound."""
    X, y, Xt, cov = tam.inputs("n65_d2", kind)
    bad = tm.entry_fp64(tm.sqdist64(X, X), 1.0, float(cov.fp64().sf2), kind)[0]
    excess = tam.entry_excess(bad, X, X, cov)
    print("ignored weights kind %d: |entry - truth| / bound %.3g" % (kind, excess))
    assert excess > 1.0
