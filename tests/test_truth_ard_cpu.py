"""CPU checks of the ARD truth (tests/truth_ard.py), of its yardstick and of the factor F_ARD -- everything
tests/test_gpu_ard.py leans on.

  - TruthARD with all length scales equal reproduces truth.Truth (both longdouble; they differ in (D / l)^2 against
    D^2 / l^2) to within 1/100 of the case's fp64 yardstick -- the margin docs/ACCURACY.md demands of the truth itself;
  - TruthARD against mpmath at 50 digits with unequal length scales;
  - the stand-in table over the ARD case list, and F_ARD = the next power of two at or above twice its largest ratio.
"""
import numpy as np
import pytest

import truth
import truth_ard as ta
from conftest import synth

pytestmark = pytest.mark.skipif(not truth.EXTENDED, reason="numpy.longdouble is not an extended-precision type here")

LD = truth.LD


@pytest.mark.parametrize("name", ["n65", "n257_d3"])
def test_equal_length_scales_reproduce_the_isotropic_truth(oracle, name):
    X, y, Xt, hp = truth.live_inputs(name)
    d = X.shape[1]
    t = truth.Truth(X, y, hp)
    tm, tv = t.predict(Xt)
    a = ta.TruthARD(X, y, [hp[0]] * d + [hp[1], hp[2]])
    am, av = a.predict(Xt)
    noise, _, _ = truth.noise_level(oracle, X, y, hp, Xt, t.ll, t.grad, tm, tv)
    fl = truth.floors(truth.scales(hp, t.ll, t.grad, tm))
    e = truth.errors(a.ll, [a.grad[:d].sum(), a.grad[d], a.grad[d + 1]], am, av, t.ll, t.grad, tm, tv)
    for q in truth.QUANTITIES:
        yard = max(noise[q], fl[q])
        print("%s %s: |ARD truth - truth| %.3g, yardstick %.3g" % (name, q, e[q], yard))
        assert e[q] <= yard / 100, (name, q, e[q], yard)


def test_truth_ard_vs_mpmath(oracle):
    """n = 24, d = 3, unequal length scales: LL, the five gradient components and three predictions at 50 digits; the
    truth's error is at most 1/100 of the case's yardstick."""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    n, d = 24, 3
    hp = [0.9, 0.3, 1.6, 0.2, -1.0]
    X, y = synth(n, d=d, seed=n, scale=4.0)
    Xt = synth(3, d=d, seed=7, scale=4.0)[0]
    t = ta.TruthARD(X, y, hp)
    tm, tv = t.predict(Xt)
    noise, _, _ = ta.noise_level_ard(oracle, X, y, hp, Xt, t.ll, t.grad, tm, tv)
    fl = ta.floors_ard(ta.scales_ard(hp, t.ll, t.grad, tm))

    w = [mp.e ** (-mp.mpf(float(h))) for h in hp[:d]]
    sf2, sn2 = mp.e ** (2 * mp.mpf(float(hp[d]))), mp.e ** (2 * mp.mpf(float(hp[d + 1])))
    Xm = [[mp.mpf(float(v)) for v in r] for r in X]
    ym = mp.matrix([mp.mpf(float(v)) for v in y])
    D2 = [mp.matrix(n, n) for _ in range(d)]
    Kf = mp.matrix(n, n)
    for i in range(n):
        for j in range(n):
            for c in range(d):
                D2[c][i, j] = ((Xm[i][c] - Xm[j][c]) * w[c]) ** 2
            Kf[i, j] = sf2 * mp.e ** (-sum(D2[c][i, j] for c in range(d)) / 2)
    K = Kf + sn2 * mp.eye(n)
    L = mp.cholesky(K)
    Ki = K ** -1
    a = Ki * ym
    ll = -((ym.T * a)[0] + 2 * sum(mp.log(L[i, i]) for i in range(n)) + n * mp.mpf(truth.LL_CONST)) / 2
    W = Ki - a * a.T
    g = [sum(W[i, j] * Kf[i, j] * D2[c][i, j] for i in range(n) for j in range(n)) / 2 for c in range(d)]
    g += [sum(W[i, j] * Kf[i, j] for i in range(n) for j in range(n)), sn2 * sum(W[i, i] for i in range(n))]
    gs = max(abs(v) for v in g)

    def to_mp(v):
        hi = float(v)
        return mp.mpf(hi) + mp.mpf(float(v - LD(hi)))
    err = dict(ll=abs(to_mp(t.ll) - ll) / abs(ll), gc=max(abs(to_mp(t.grad[c]) - g[c]) for c in range(d)) / gs,
               gf=abs(to_mp(t.grad[d]) - g[d]) / gs, gn=abs(to_mp(t.grad[d + 1]) - g[d + 1]) / gs, mean=0, var=0)
    for k, xt in enumerate(Xt):
        ks = mp.matrix([sf2 * mp.e ** (-sum(((mp.mpf(float(xt[c])) - Xm[i][c]) * w[c]) ** 2 for c in range(d)) / 2)
                        for i in range(n)])
        err["mean"] = max(err["mean"], abs(to_mp(tm[k]) - (ks.T * a)[0]))
        err["var"] = max(err["var"], abs(to_mp(tv[k]) - (sf2 + sn2 - (ks.T * Ki * ks)[0])))
    for q in ta.QUANTITIES:
        yard = max(noise[q], fl[q])
        print("%s: truth error %.3g, yardstick %.3g" % (q, float(err[q]), yard))
        assert float(err[q]) <= yard / 100, (q, float(err[q]), yard)


def test_F_ARD_covers_twice_the_standin(oracle):
    """The project's rule (docs/ACCURACY.md, "The bound"): F_ARD is the next power of two at or above twice the largest
    stand-in / yardstick ratio over the ARD case list -- measured here, on the CPU; F_SOLVE likewise for alpha and
    K^-1.  The yardsticks stay under the sanity cap, and the oracle on the data as given is no outlier among the
    permuted evaluations.  The ratios are those of the BLAS this runs on (docs/ACCURACY.md has the table of the build
    it was measured with)."""
    worst, worst_solve = 0.0, 0.0
    for name in ta.ARD_CASES:
        X, y, Xt, hp = ta.ard_inputs(name)
        t = ta.TruthARD(X, y, hp)
        tm, tv = t.predict(Xt)
        noise, first, rest = ta.noise_level_ard(oracle, X, y, hp, Xt, t.ll, t.grad, tm, tv)
        fl = ta.floors_ard(ta.scales_ard(hp, t.ll, t.grad, tm))
        st = ta.standin_ard(X, y, hp, Xt, solve=True)
        se = ta.errors_ard(*st[:4], t.ll, t.grad, tm, tv)
        rows = truth.solve_rows(len(y))
        ns = ta.noise_level_solve_ard(oracle, X, y, hp, t, rows)
        ss = truth.solve_errors(st[4], st[5], t, rows)
        ratio = {q: se[q] / max(noise[q], fl[q]) for q in ta.QUANTITIES}
        rs = {q: ss[q] / max(ns[q], 4 * 2.0 ** -52) for q in truth.SOLVE_QUANTITIES}
        print("STANDIN-ARD %-14s " % name + "  ".join("%s %.2f" % kv for kv in list(ratio.items()) + list(rs.items())))
        worst, worst_solve = max(worst, *ratio.values()), max(worst_solve, *rs.values())
        for q in ta.QUANTITIES:
            assert first[q] <= ta.F_ARD * max(rest[q], fl[q]), (name, q, first[q], rest[q])
            scale = fl[q] / (4 * 2.0 ** -52)
            assert noise[q] <= ta.YARDSTICK_CAP * scale, (name, q, noise[q], scale)
    print("largest stand-in ratio %.2f (F_ARD %d), alpha / K^-1 %.2f (F_SOLVE %d)" % (worst, ta.F_ARD, worst_solve, ta.F_SOLVE))
    assert 2 * worst <= ta.F_ARD, (worst, ta.F_ARD)
    assert 2 * worst_solve <= ta.F_SOLVE, (worst_solve, ta.F_SOLVE)
    assert ta.F_ARD & (ta.F_ARD - 1) == 0
