"""CPU checks of the ARD truth (truth.Truth with the truth.ARD descriptor), of its yardstick and of the factor F_ARD --
everything tests/test_gpu_ard.py leans on.

  - the ARD truth with all length scales equal reproduces the isotropic one (both longdouble; they differ in (D / l)^2
    against D^2 / l^2) to within 1/100 of the case's fp64 yardstick -- the margin docs/ACCURACY.md demands of the
    truth itself;
  - the ARD truth against mpmath at 50 digits with unequal length scales;
  - the stand-in table over the ARD case list, and F_ARD = the next power of two at or above twice its largest ratio.
"""
import pytest

import accuracy
import truth
from conftest import synth

pytestmark = pytest.mark.skipif(not truth.EXTENDED, reason="numpy.longdouble is not an extended-precision type here")

LD = truth.LD


@pytest.mark.parametrize("name", ["n65", "n257_d3"])
def test_equal_length_scales_reproduce_the_isotropic_truth(oracle, name):
    c = accuracy.live(oracle, "se", name)
    X, y, Xt, cov, t = c["X"], c["y"], c["Xt"], c["cov"], c["t"]
    d = X.shape[1]
    a = truth.Truth(X, y, truth.ARD([cov.hp[0]] * d + cov.hp[1:]))
    am, av = a.predict(Xt)
    e = truth.errors(cov, a.ll, [a.grad[:d].sum(), a.grad[d], a.grad[d + 1]], am, av, t.ll, t.grad, c["tm"], c["tv"])
    for q in cov.quantities:
        yard = max(c["noise"][q], c["floor"][q])
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
    cov = truth.ARD(hp)
    c = accuracy.case_at(oracle, cov, X, y, Xt, truth.Truth(X, y, cov))
    t, tm, tv = c["t"], c["tm"], c["tv"]

    w = [mp.e ** (-mp.mpf(float(h))) for h in hp[:d]]
    sf2, sn2 = mp.e ** (2 * mp.mpf(float(hp[d]))), mp.e ** (2 * mp.mpf(float(hp[d + 1])))
    Xm = [[mp.mpf(float(v)) for v in r] for r in X]
    ym = mp.matrix([mp.mpf(float(v)) for v in y])
    D2 = [mp.matrix(n, n) for _ in range(d)]
    Kf = mp.matrix(n, n)
    for i in range(n):
        for j in range(n):
            for k in range(d):
                D2[k][i, j] = ((Xm[i][k] - Xm[j][k]) * w[k]) ** 2
            Kf[i, j] = sf2 * mp.e ** (-sum(D2[k][i, j] for k in range(d)) / 2)
    K = Kf + sn2 * mp.eye(n)
    L = mp.cholesky(K)
    Ki = K ** -1
    a = Ki * ym
    ll = -((ym.T * a)[0] + 2 * sum(mp.log(L[i, i]) for i in range(n)) + n * mp.mpf(truth.LL_CONST)) / 2
    W = Ki - a * a.T
    g = [sum(W[i, j] * Kf[i, j] * D2[k][i, j] for i in range(n) for j in range(n)) / 2 for k in range(d)]
    g += [sum(W[i, j] * Kf[i, j] for i in range(n) for j in range(n)), sn2 * sum(W[i, i] for i in range(n))]
    gs = max(abs(v) for v in g)

    def to_mp(v):
        hi = float(v)
        return mp.mpf(hi) + mp.mpf(float(v - LD(hi)))
    err = dict(ll=abs(to_mp(t.ll) - ll) / abs(ll), gc=max(abs(to_mp(t.grad[k]) - g[k]) for k in range(d)) / gs,
               gf=abs(to_mp(t.grad[d]) - g[d]) / gs, gn=abs(to_mp(t.grad[d + 1]) - g[d + 1]) / gs, mean=0, var=0)
    for k, xt in enumerate(Xt):
        ks = mp.matrix([sf2 * mp.e ** (-sum(((mp.mpf(float(xt[j])) - Xm[i][j]) * w[j]) ** 2 for j in range(d)) / 2)
                        for i in range(n)])
        err["mean"] = max(err["mean"], abs(to_mp(tm[k]) - (ks.T * a)[0]))
        err["var"] = max(err["var"], abs(to_mp(tv[k]) - (sf2 + sn2 - (ks.T * Ki * ks)[0])))
    for q in cov.quantities:
        yard = max(c["noise"][q], c["floor"][q])
        print("%s: truth error %.3g, yardstick %.3g" % (q, float(err[q]), yard))
        assert float(err[q]) <= yard / 100, (q, float(err[q]), yard)


def test_F_ARD_covers_twice_the_standin(oracle):
    """The project's rule (docs/ACCURACY.md, "The bound"): F_ARD is the next power of two at or above twice the largest
    stand-in / yardstick ratio over the ARD case list -- measured here, on the CPU; F_SOLVE likewise for alpha and
    K^-1.  The yardsticks stay under the sanity cap, and the oracle on the data as given is no outlier among the
    permuted evaluations.  The ratios are those of the BLAS this runs on (docs/ACCURACY.md has the table of the build
    it was measured with)."""
    worst, worst_solve = 0.0, 0.0
    for name in truth.ARD_CASES:
        c = accuracy.live(oracle, "ard", name)
        ratio, rs = accuracy.standin_ratios(c)
        print("STANDIN-ARD %-14s " % name + "  ".join("%s %.2f" % kv for kv in list(ratio.items()) + list(rs.items())))
        worst, worst_solve = max(worst, *ratio.values()), max(worst_solve, *rs.values())
        accuracy.assert_yardstick_is_sane(c, name)
    print("largest stand-in ratio %.2f (F_ARD %d), alpha / K^-1 %.2f (F_SOLVE %d)" % (worst, truth.F_ARD, worst_solve, truth.F_SOLVE))
    assert 2 * worst <= truth.F_ARD, (worst, truth.F_ARD)
    assert 2 * worst_solve <= truth.F_SOLVE, (worst_solve, truth.F_SOLVE)
    assert truth.F_ARD & (truth.F_ARD - 1) == 0
