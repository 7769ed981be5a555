"""CPU checks of the rational quadratic truth (truth.Truth with truth_rq.RQ, ARD and tied), of its yardstick, of the factor
F_RQ and of the K-entry bound -- everything tests/test_gpu_rq.py leans on.

  1. the truth's gradient against a central difference of its own LL in longdouble, every component (alpha included);
  2. the tied gradient is the sum of the ARD gradient's length components at equal scales;
  3. theta_alpha = 30 against truth.ARD within a bound derived from s^2 / (8 alpha);
  4. the stand-in stays within F_RQ, F_RQ is what the rule gives, alpha / K^-1 stay under F_SOLVE; every yardstick sane;
  5. rq_entry's arithmetic, restated in fp64 numpy, inside the derived bound on every case, exact at s = 0;
  6. three mutations leave the bound: H := Kf, A without u / (1 + u), u := s / alpha.
"""
import numpy as np
import pytest

import accuracy
import truth
import truth_rq as trq
from conftest import synth

pytestmark = pytest.mark.skipif(not truth.EXTENDED, reason="numpy.longdouble is not an extended-precision type here")

LD = truth.LD


@pytest.mark.parametrize("tied", [False, True], ids=["ard", "tied"])
def test_gradient_is_the_derivative_of_ll(tied):
    """grad_k = d(-LL)/d theta_k by a central difference in longdouble; n = 40; step and tolerance as
    tests/test_truth_matern_cpu.py derives them (h = 2^-20, 100 (h^2 + eps_LD / h |LL| / max|g|))."""
    n, d = 40, 3
    X, y = synth(n, d=d, seed=n, scale=4.0)
    hp = [0.9, 0.4, 0.3, -1.0] if tied else [0.9, 0.3, 1.6, 0.4, 0.3, -1.0]
    h = 2.0 ** -20
    t = truth.Truth(X, y, trq.RQ(hp, tied))
    gs = np.max(np.abs(t.grad))
    tol = 100 * (h * h + truth.EPS_LD / h * float(abs(t.ll) / gs))
    assert len(t.grad) == len(hp)
    for k in range(len(hp)):
        lo, hi = list(hp), list(hp)
        lo[k], hi[k] = hp[k] - h, hp[k] + h
        num = (truth.Truth(X, y, trq.RQ(lo, tied)).ll - truth.Truth(X, y, trq.RQ(hi, tied)).ll) / (LD(hi[k]) - LD(lo[k]))
        err = float(abs(num - t.grad[k]) / gs)
        print("g%d: formula %.15g, central difference %.15g, |diff| / max|g| %.3e (tolerance %.3e)"
              % (k, float(t.grad[k]), float(num), err, tol))
        assert err <= tol, (k, err, tol)


def test_tied_gradient_is_the_sum_of_the_length_components():
    """Equal length scales: LL, the alpha, signal and noise components and the prediction are the ARD descriptor's (the
    same operations on the same numbers: exactly), g_0 its length components added in index order."""
    n, d = 60, 3
    X, y = synth(n, d=d, seed=n, scale=4.0)
    Xt = synth(9, d=d, seed=7, scale=4.0)[0]
    hp = [0.9, 0.4, 0.3, -1.0]
    tt = truth.Truth(X, y, trq.RQ(hp, tied=True))
    ta = truth.Truth(X, y, trq.RQ([hp[0]] * d + hp[1:]))
    s = ta.grad[0]
    for c in range(1, d):
        s = s + ta.grad[c]
    assert tt.ll == ta.ll and tt.grad[0] == s and np.array_equal(tt.grad[1:], ta.grad[d:])
    (mt, vt), (ma, va) = tt.predict(Xt), ta.predict(Xt)
    assert np.array_equal(mt, ma) and np.array_equal(vt, va)


def test_large_alpha_is_the_se_ard_kernel():
    """theta_alpha = 30: -alpha log1p(u) = -s/2 + s^2 / (8 alpha) - ..., an alternating series, so 0 <= log(Kf / K_SE) <=
    s^2 / (8 alpha) entry by entry (to longdouble rounding of the two exponents: 1e3 eps_LD covers it); H / Kf = 1 / (1 + u)
    and A -> -Kf s^2 / (8 alpha).  The issue's figure: the entries differ by 4e-14 of sf2 at most."""
    n, d = 60, 3
    X, y = synth(n, d=d, seed=n, scale=4.0)
    th = [0.9, 0.3, 1.6]
    rq = trq.RQ(th + [30.0, 0.3, -1.0])
    se = truth.ARD(th + [0.3, -1.0])
    Xl = X.astype(LD)
    S = truth.wsqdist(Xl, Xl, rq.w)
    Kf, H, A = trq.parts(S, rq.sf2, rq.alpha)
    Kse = se.k(Xl, Xl)
    bound = S * S / (8 * rq.alpha)
    lr = np.log(Kf / Kse)
    slack = 1e3 * truth.EPS_LD * (1 + S)
    assert np.all(lr >= -slack) and np.all(lr <= bound + slack)
    print("largest |Kf - K_SE| / sf2 %.3e (bound on the log ratio %.3e)" % (float(np.max(np.abs(Kf - Kse)) / rq.sf2), float(bound.max())))
    assert float(np.max(np.abs(Kf - Kse)) / rq.sf2) <= 1e-13
    assert np.all(np.abs(A + Kf * bound) <= Kf * bound * (S / rq.alpha) + 1e-30)       # next term of the series: O(u) relative
    t_rq, t_se = truth.Truth(X, y, rq), truth.Truth(X, y, se)
    cond = float(n * rq.sf2 / rq.sn2 + 1)
    assert abs(t_rq.ll - t_se.ll) <= 10 * cond * float(bound.max()) * n


@pytest.fixture(scope="module")
def table(oracle):
    """Stand-in ratios (the eight orderings) and yardsticks of every case of both forms -- computed once."""
    out = {}
    for family, name in trq.ALL_CASES:
        c = trq.live(oracle, family, name)
        r, rs = trq.standin_orderings(c), accuracy.standin_ratios(c)[1]
        out[family, name] = (c, r, rs)
        print("STANDIN-RQ %-7s %-14s " % (family, name) + "  ".join("%s %.2f" % kv for kv in list(r.items()) + list(rs.items()))
              + "  | yardstick " + " ".join("%s %.1e" % kv for kv in c["noise"].items()))
    return out


def test_case_lists():
    assert trq.RQ_CASES == ("n1_d2", "n2_d2", "n63_d2", "n64_d2", "n65_d2", "n257_d3", "n257_d3_shift", "n300_d17",
                            "n515_d33", "n515_dense", "n384_cond1e6", "n1025_dense")
    want = dict(n1_d2=0.4, n2_d2=0.4, n63_d2=0.4, n64_d2=0.4, n65_d2=0.4, n257_d3=-0.7, n257_d3_shift=12.0, n300_d17=2.0,
                n515_d33=-0.7, n515_dense=0.4, n384_cond1e6=0.4, n1025_dense=2.0)
    assert trq.THETA_ALPHA == want and trq.TIED_CASES == ("n65", "n257_d3", "n300_d17", "n384_cond1e6")
    for name in trq.RQ_CASES:
        X, y, Xt, cov = trq.inputs("rq_ard", name)
        Xa, ya, Xta, hpa = truth.ard_inputs(name)
        assert np.array_equal(X, Xa) and np.array_equal(y, ya) and np.array_equal(Xt, Xta)
        assert cov.hp == hpa[:-2] + [want[name]] + hpa[-2:] and not cov.tied and cov.F == trq.F_RQ
    for name in trq.TIED_CASES:
        X, y, Xt, cov = trq.inputs("rq", name)
        Xa, ya, Xta, hpa = truth.live_inputs(name)
        assert np.array_equal(X, Xa) and np.array_equal(y, ya) and cov.tied and cov.hp == [hpa[0], 0.4, hpa[1], hpa[2]]
    assert truth.FAMILIES["rq"][1]([0.1, 0.2, 0.3, 0.4]).tied and not truth.FAMILIES["rq_ard"][1]([0.1, 0.2, 0.3, 0.4]).tied


def test_no_case_is_left_out_and_yardsticks_are_sane(table):
    """Every case of both forms has yardsticks under truth.YARDSTICK_CAP (1e-9, test_truth_cpu.py's cap): cond(K) <= 1 + n
    sf2 / sn2 whatever alpha is."""
    assert set(table) == set(trq.ALL_CASES) and truth.YARDSTICK_CAP == 1e-9
    for key, (c, _, _) in table.items():
        accuracy.assert_yardstick_is_sane(c, key)


def test_standin_within_f_rq_and_f_rq_is_what_the_rule_gives(table):
    """The project's rule (docs/ACCURACY.md, "The bound"): F_RQ is the next power of two at or above twice the largest
    stand-in ratio as it was measured before the first GPU run (truth_rq.STANDIN_WORST); the stand-in of the BLAS this runs
    on asks for no more; alpha and K^-1 stay under F_SOLVE."""
    assert trq.F_RQ == truth.factor_rule(trq.STANDIN_WORST)
    worst = max(max(r.values()) for _, r, _ in table.values())
    worst_solve = max(max(rs.values()) for _, _, rs in table.values())
    print("largest stand-in ratio %.2f -> factor by the rule %d (F_RQ %d); alpha / K^-1 %.2f (F_SOLVE %d)"
          % (worst, truth.factor_rule(worst), trq.F_RQ, worst_solve, truth.F_SOLVE))
    assert all(max(r.values()) <= trq.F_RQ for _, r, _ in table.values())
    assert truth.factor_rule(worst) <= trq.F_RQ, (worst, trq.F_RQ)
    assert 2 * worst_solve <= truth.F_SOLVE, (worst_solve, truth.F_SOLVE)


def _entry_ratios(family, name, mutate=None):
    """Largest |entry_fp64 - truth| / bound of Kf, H and A over K and k_test of a case (mutate: on the fp64 side)."""
    X, y, Xt, cov = trq.inputs(family, name)
    d = X.shape[1]
    worst = np.zeros(3)
    for A in (X, Xt):
        S = truth.wsqdist(A.astype(LD), X.astype(LD), cov.weights(d))
        tk, th, ta = trq.parts(S, cov.sf2, cov.alpha)
        kf, hh, da = trq.entries_fp64(A, X, cov)
        if mutate == "kf_for_h":
            hh = kf
        elif mutate == "a_without_ratio":
            alpha, h2a = trq.host_shape(cov.hp[-3])
            u = trq.tam.wsqdist64(A, X, np.exp(-np.asarray([cov.hp[0 if cov.tied else c] for c in range(d)]))) * h2a
            da = kf * (alpha * (-np.log1p(u)))
        elif mutate == "u_s_over_alpha":
            alpha, h2a = trq.host_shape(cov.hp[-3])
            s = trq.tam.wsqdist64(A, X, np.exp(-np.asarray([cov.hp[0 if cov.tied else c] for c in range(d)])))
            kf, hh, da = trq.entry_fp64(s, float(cov.fp64().sf2), alpha, 2 * h2a)
        bk, bh, ba = trq.k_entry_bound(np.asarray(S / (2 * cov.alpha), dtype=np.float64), float(cov.alpha), d)
        assert float(tk.min()) > 1e-290
        with np.errstate(invalid="ignore", divide="ignore"):
            rk = np.abs(kf.astype(LD) - tk) / (tk * bk)
            rh = np.abs(hh.astype(LD) - th) / (th * bh)
            ea = np.abs(da.astype(LD) - ta)
            ra = np.where(ea == 0, LD(0), ea / (tk * cov.alpha * ba))
        worst = np.maximum(worst, [float(rk.max()), float(rh.max()), float(ra.max())])
        zero = np.asarray(S == 0)
        if mutate is None and zero.any():                          # a test point that is a training row; K's diagonal
            assert np.all(kf[zero] == np.float64(np.exp(2 * cov.hp[-2]))) and np.all(hh[zero] == kf[zero]) and np.all(da[zero] == 0.0)
    return worst


def test_fp64_entry_formula_inside_the_bound():
    """truth_rq.entry_fp64 on the kernels' weighted distance against the longdouble Kf, H and A on every case's K and k_test,
    entry by entry, inside k_entry_bound; exact values at s = 0."""
    worst = np.zeros(3)
    for family, name in trq.ALL_CASES:
        r = _entry_ratios(family, name)
        print("ENTRY %-7s %-14s |fp64 - truth| / bound: Kf %.3f  H %.3f  A %.3f" % (family, name, r[0], r[1], r[2]))
        assert np.all(r <= 1.0), (family, name, r)
        worst = np.maximum(worst, r)
    print("largest: Kf %.3f  H %.3f  A %.3f" % tuple(worst))


def test_fp64_entry_extremes():
    sf2 = 1.37
    alpha, h2a = trq.host_shape(0.4)
    kf, hh, da = trq.entry_fp64(np.array([0.0, 1.0, 1e6, 1e300]), sf2, alpha, h2a)
    assert kf[0] == sf2 and hh[0] == sf2 and da[0] == 0.0
    assert 0 < kf[1] < sf2 and 0 < hh[1] < kf[1] and da[1] < 0
    assert np.all(np.isfinite(kf)) and np.all(np.isfinite(hh)) and np.all(np.isfinite(da))
    alpha, h2a = trq.host_shape(800.0)                             # exp overflows: inf, and 0.5 / inf = 0
    assert alpha == np.inf and h2a == 0.0
    kf, hh, da = trq.entry_fp64(np.array([0.0, 1.0]), sf2, alpha, h2a)
    assert np.all(np.isnan(kf)) and np.all(np.isnan(hh)) and np.all(np.isnan(da))
    k30 = trq.entry_fp64(np.array([0.5, 3.0]), sf2, *trq.host_shape(30.0))[0]
    assert np.all(np.abs(k30 - sf2 * np.exp(-0.5 * np.array([0.5, 3.0]))) <= 4e-14 * sf2)


@pytest.mark.parametrize("mutate, which", [("kf_for_h", 1), ("a_without_ratio", 2), ("u_s_over_alpha", 0)])
def test_mutations_leave_the_entry_bound(mutate, which):
    """H := Kf, A without u / (1 + u), u := s / alpha: each leaves the bound of the entry it touches -- on n65_d2 and on the
    SE-limit case n257_d3_shift, where u is ~1e-5 and the margins are smallest."""
    for name in ("n65_d2", "n257_d3_shift"):
        r = _entry_ratios("rq_ard", name, mutate)
        print("%s on %s: |entry - truth| / bound  Kf %.3g  H %.3g  A %.3g" % (mutate, name, r[0], r[1], r[2]))
        assert r[which] > 1.0, (mutate, name, r)


@pytest.mark.parametrize("mutate, q", [("kf_for_h", "gc"), ("a_without_ratio", "gc")])
def test_mutations_leave_the_gradient_bound(mutate, q, oracle):
    """The same two mutations in the stand-in's descriptor: the length / alpha components leave F_RQ yardsticks, LL and the
    prediction, which read neither H nor A, stay inside."""
    c = trq.live(oracle, "rq_ard", "n65_d2")
    st = truth.standin(trq.RQ(c["cov"].hp, mutate=mutate), c["X"], c["y"], c["Xt"])
    e = truth.errors(c["cov"], *st, c["t"].ll, c["t"].grad, c["tm"], c["tv"])
    r = {k: e[k] / max(c["noise"][k], c["floor"][k]) for k in c["cov"].quantities}
    print("%s: " % mutate + "  ".join("%s %.3g" % kv for kv in r.items()))
    assert r[q] > trq.F_RQ and all(r[k] <= trq.F_RQ for k in ("ll", "gf", "gn", "mean", "var"))
