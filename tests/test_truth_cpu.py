"""CPU checks of the extended-precision truth (tests/truth.py), of the fp64 yardstick taken from the oracle, and of
the committed fixtures under tests/golden/truth* -- everything tests/test_gpu_accuracy.py leans on.

  - the truth against mpmath at 50 digits: its own error is at most 1/100 of the case's yardstick;
  - the yardstick is sane on every live case: the oracle on the data as given is no outlier among the permuted
    evaluations, and no yardstick exceeds 1e-9 of its quantity's scale (a cap, not a measurement);
  - the stand-in (LAPACK / BLAS order), from which F was set (docs/ACCURACY.md), passes the GPU's own bound;
  - every fixture loads with its keys and its 300-row sibling regenerates to the same strings;
  - beyond one test tile (tests/test_gpu_predict_wide.py): the stand-in at 129, 200 and 257 test points, joint covariance
    included, against the factors F, F_ARD and F_MATERN by the project's rule; numpy's Cholesky and draws inside the two
    derived bounds the GPU's draws are held to.
"""
import os
import sys

import numpy as np
import pytest

import accuracy
import truth
from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import make_truth  # noqa: E402

pytestmark = pytest.mark.skipif(not truth.EXTENDED, reason="numpy.longdouble is not an extended-precision type here")


# ------------------------------------------------------------------ the truth against mpmath
def mp_eval(mp, X, y, hp, Xt):
    """The same formulas in mpmath at 50 digits, as plainly as they can be written."""
    n = len(y)
    l2, sf2, sn2 = [mp.e ** (2 * mp.mpf(float(h))) for h in hp]
    Xm = [[mp.mpf(float(v)) for v in r] for r in X]
    ym = mp.matrix([mp.mpf(float(v)) for v in y])
    S, Kf = mp.matrix(n, n), mp.matrix(n, n)
    for i in range(n):
        for j in range(n):
            S[i, j] = sum((a - b) ** 2 for a, b in zip(Xm[i], Xm[j])) / l2
            Kf[i, j] = sf2 * mp.e ** (-S[i, j] / 2)
    K = Kf + sn2 * mp.eye(n)
    L = mp.cholesky(K)
    Ki = K ** -1
    a = Ki * ym
    # n times the fp64 value of the literal 1.83787: what the device multiplies by (the decimal differs at 5e-17 of LL)
    ll = -((ym.T * a)[0] + 2 * sum(mp.log(L[i, i]) for i in range(n)) + n * mp.mpf(truth.LL_CONST)) / 2
    W = Ki - a * a.T
    g = [sum(W[i, j] * Kf[i, j] * S[i, j] for i in range(n) for j in range(n)) / 2,
         sum(W[i, j] * Kf[i, j] for i in range(n) for j in range(n)),
         sn2 * sum(W[i, i] for i in range(n))]
    mean, var = [], []
    for xt in Xt:
        ks = mp.matrix([sf2 * mp.e ** (-sum((mp.mpf(float(p)) - q) ** 2 for p, q in zip(xt, Xm[i])) / l2 / 2)
                        for i in range(n)])
        mean.append((ks.T * a)[0])
        var.append(sf2 + sn2 - (ks.T * Ki * ks)[0])
    return ll, g, mean, var


def to_mp(mp, v):
    """An 80-bit long double into mpmath exactly: high and low fp64 halves."""
    hi = float(v)
    return mp.mpf(hi) + mp.mpf(float(v - truth.LD(hi)))


@pytest.mark.parametrize("n", [24, 48])
@pytest.mark.parametrize("hp,scale", [([0.9, 0.2, -1.0], 4.0), ([1.5, 0.5, -3.0], 2.0)],
                         ids=["well-conditioned", "noise-exp-minus-6"])
def test_truth_vs_mpmath(oracle, n, hp, scale):
    """LL, gradient and three predictions: the truth's error is at most 1/100 of the case's yardstick
    max(noise, floor) -- the quantity the GPU bound multiplies -- so it can serve as truth for it.
    Seen: 4e-20 .. 2e-18 well-conditioned, 3e-17 .. 5e-16 at cond ~ 1e6 (yardstick there >= 1e-13)."""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    from conftest import synth
    X, y = synth(n, d=3, seed=n, scale=scale)
    Xt = synth(3, d=3, seed=7, scale=scale)[0]
    cov = truth.SE(hp)
    c = accuracy.case_at(oracle, cov, X, y, Xt, truth.Truth(X, y, cov, keep=False))
    t, tm, tv = c["t"], c["tm"], c["tv"]
    ll, g, mean, var = mp_eval(mp, X, y, hp, Xt)
    gs = max(abs(v) for v in g)
    err = dict(ll=abs(to_mp(mp, t.ll) - ll) / abs(ll),
               mean=max(abs(to_mp(mp, tm[k]) - mean[k]) for k in range(3)),
               var=max(abs(to_mp(mp, tv[k]) - var[k]) for k in range(3)))
    for k in range(3):
        err["g%d" % k] = abs(to_mp(mp, t.grad[k]) - g[k]) / gs
    for q in cov.quantities:
        yard = max(c["noise"][q], c["floor"][q])
        print("n=%d %s: truth error %.3g, yardstick %.3g" % (n, q, float(err[q]), yard))
        assert float(err[q]) <= yard / 100, (n, hp, q, float(err[q]), yard)


# ------------------------------------------------------------------ the yardstick
@pytest.mark.parametrize("name", list(truth.LIVE_CASES))
def test_yardstick_is_sane(oracle, name):
    """The oracle's error on the data as given is no outlier among the 7 permuted evaluations (within F of the largest
    of them, floored like the bound), and no yardstick exceeds 1e-9 of its scale: a broken truth or oracle cannot
    silently loosen the GPU test."""
    accuracy.assert_yardstick_is_sane(accuracy.live(oracle, "se", name), name)


def test_F_covers_the_standin(oracle):
    """F and F_SOLVE are the next powers of two at or above twice the largest stand-in / yardstick ratio over the case
    list (docs/ACCURACY.md).  Here: the LAPACK / BLAS-ordered evaluation itself passes the bound the GPU is held to
    on every live case.  The ratios are those of the BLAS this runs on (its blocking and thread count set the order of
    summation): the table in docs/ACCURACY.md is of the build it was measured with, and the factor of two between it
    and F is what is left for another one."""
    for name in truth.LIVE_CASES:
        ratio, rs = accuracy.standin_ratios(accuracy.live(oracle, "se", name))
        print("STANDIN %-14s " % name + "  ".join("%s %.2f" % kv for kv in list(ratio.items()) + list(rs.items())))
        for q, r in ratio.items():
            assert r <= truth.F, (name, q, r)
        for q, r in rs.items():
            assert r <= truth.F_SOLVE, (name, q, r)


# ------------------------------------------------------------------ the fixtures
KEYS = {"case", "n", "d", "hp", "experts", "nt", "ll", "grad", "mean", "var", "noise", "oracle_as_given",
        "oracle_permuted", "seconds"}
SE_FIXTURES = sorted(c for c in make_truth.CASES if make_truth.CASES[c]["family"] == "se")


@pytest.mark.parametrize("name", SE_FIXTURES)
def test_fixture_loads(name):
    for n in (None, make_truth.SIBLING_ROWS):
        f = make_truth.load(name, n)
        cov = truth.SE(f["hp"])
        assert set(f["raw"]) == KEYS, set(f["raw"]) ^ KEYS
        assert f["n"] == (make_truth.CASES[name]["n"] if n is None else n) and f["nt"] == make_truth.NT
        assert f["grad"].shape == (3,) and f["mean"].shape == (f["nt"],) and f["var"].shape == (f["nt"],)
        assert set(f["noise"]) == set(truth.QUANTITIES) == set(f["oracle_as_given"]) == set(f["oracle_permuted"])
        assert np.all(np.isfinite(f["mean"].astype(float))) and np.all(f["var"] > 0)
        sv = float(np.exp(2 * f["hp"][1]) + np.exp(2 * f["hp"][2]))
        scale = dict(ll=1.0, g0=1.0, g1=1.0, g2=1.0, mean=float(np.max(np.abs(f["mean"]))), var=sv)
        fl = truth.floors(cov, truth.scales(cov, f["ll"], f["grad"], f["mean"]))
        for q in truth.QUANTITIES:
            # the same two checks as test_yardstick_is_sane: the evaluation on the data as given is no outlier among
            # the permuted ones, and the yardstick stays under its cap
            first, rest = f["oracle_as_given"][q], f["oracle_permuted"][q]
            assert f["noise"][q] == max(first, rest) and min(first, rest) >= 0, (name, n, q)
            assert first <= truth.F * max(rest, fl[q]), (name, n, q, first, rest)
            assert f["noise"][q] <= truth.YARDSTICK_CAP * scale[q], (name, n, q)
        assert os.path.getsize(make_truth.path(name, n)) < 16384


@pytest.mark.parametrize("name", sorted(make_truth.CASES))
def test_fixture_sibling_regenerates(oracle, name):
    """The 300-row sibling of every fixture, of every family, comes out of make_truth.py with the committed strings,
    digit for digit: the generator has not drifted from the files.  And the generator's --standin row of that sibling
    (the stand-in against the committed truth and yardstick) comes out: one finite ratio per quantity of the family.
    (Its size is of the BLAS this runs on and of a case outside the lists the factors were set over: printed only.)"""
    got = make_truth.compute(name, make_truth.SIBLING_ROWS, oracle)
    want = dict(make_truth.load(name, make_truth.SIBLING_ROWS)["raw"])
    want.pop("seconds")
    assert got == want, {k: (got.get(k), want.get(k)) for k in set(got) | set(want) if got.get(k) != want.get(k)}
    row = make_truth.standin_row(name, make_truth.SIBLING_ROWS)
    print("STANDIN %s_n%d " % (name, make_truth.SIBLING_ROWS) + "  ".join("%s %.2f" % kv for kv in row.items()))
    assert list(row) == list(got["noise"]) and all(np.isfinite(r) and r >= 0 for r in row.values()), row


# ------------------------------------------------------------------ beyond one test tile
def check_wide_rule(worst, F, name):
    """The project's rule: F is a power of two and at least twice the largest stand-in ratio.  (The factor of a family
    is set over all its rows, so the wide rows alone may ask for less than it, never for more.)"""
    print("largest wide stand-in ratio %.2f -> the rule asks for %d (%s = %d)" % (worst, truth.factor_rule(worst), name, F))
    assert truth.factor_rule(worst) <= F and F & (F - 1) == 0, (worst, truth.factor_rule(worst), F)


def wide_standin_worst(oracle, family, cases, sane=False):
    """The stand-in's means, variances and joint covariance (LAPACK / BLAS) of a family's wide cases {name: sizes}
    against the longdouble truth, over the yardstick of the same test points -> the largest ratio.  sane: the yardstick
    of the wide points is as sane as that of the 64."""
    worst = 0.0
    for name, nts in cases.items():
        for nt in nts:
            c = accuracy.wide(oracle, family, name, nt)
            worst = max(worst, *accuracy.wide_standin_ratios("%s%s nt=%d" % ("" if family == "se" else family + " ", name, nt), c).values())
            if sane:
                accuracy.assert_yardstick_is_sane(c, (name, nt), ("mean", "var"))
    return worst


def test_wide_standin_se(oracle):
    """truth.WIDE_CASES at their 129 / 200 / 257 test points -> the rule gives F."""
    check_wide_rule(wide_standin_worst(oracle, "se", truth.WIDE_CASES, sane=True), truth.F, "F")


def test_wide_standin_ard(oracle):
    """The ARD case of the wide tests (n257_d3 with ARD_CASES' length scales, 200 test points) against F_ARD."""
    cases = {truth.WIDE_FAMILY_CASES["ard"]: (truth.WIDE_NT_FAMILY,)}
    check_wide_rule(wide_standin_worst(oracle, "ard", cases), truth.F_ARD, "F_ARD")


def test_wide_standin_matern(oracle):
    """The Matern case of the wide tests (n300_d17, nu = 5/2, 200 test points) against F_MATERN."""
    cases = {truth.WIDE_FAMILY_CASES["matern52"]: (truth.WIDE_NT_FAMILY,)}
    check_wide_rule(wide_standin_worst(oracle, "matern52", cases), truth.F_MATERN, "F_MATERN")


def test_wide_standin_bcm(oracle):
    """The BCM rows of the wide tests (three 300-row experts, the uneven 5-expert split of 1307 rows; 200 test points):
    truth.standin_bcm's product of experts against truth.bcm_truth, over the yardstick from the oracle's BCM with the
    rows permuted inside each expert -> the rule asks for no more than F."""
    worst = 0.0
    for N, K in truth.WIDE_BCM:
        X, y, Xt, cov = truth.wide_bcm_inputs(N, K)
        tb = truth.bcm_truth(X, y, cov, K, Xt)
        noise, _, _ = truth.bcm_yardstick(oracle, cov, X, y, K, Xt, tb)
        fl = truth.floors(cov, truth.scales(cov, tb["ll"], tb["grad"], tb["mean"]))
        _, _, m, v = truth.standin_bcm(cov, X, y, K, Xt)
        e = truth.errors_pred(m, v, tb["mean"], tb["var"])
        r = {q: e[q] / max(noise[q], fl[q]) for q in ("mean", "var")}
        print("STANDIN-WIDE bcm %dx%d nt=%d  " % (K, N, len(Xt)) + "  ".join("%s %.2f" % kv for kv in r.items())
              + "  | yardstick " + " ".join("%s %.1e" % (q, max(noise[q], fl[q])) for q in ("mean", "var")))
        worst = max(worst, *r.values())
    check_wide_rule(worst, truth.F, "F")


@pytest.mark.parametrize("name", ["n65", "n300_d17", "n515_dense"])
def test_numpy_factor_and_draws_inside_the_derived_bounds(name):
    """The two bounds tests/test_gpu_predict_wide.py holds the library's draws to, applied to an honest fp64
    implementation: numpy's Cholesky of the stand-in's joint covariance (with noise, and latent + 1e-8 sf2 on the
    diagonal) at 257 and 129 test points against truth.factor_bound_worst, and m + Z C^T (BLAS) for 7, 129 and 257
    fixed-seed draws against truth.draw_bound_worst.  Both sit well inside (factor: a few hundredths of its bound)."""
    X, y, Xt_all, cov = truth.wide_inputs(name, 257)
    sf2, sn2 = float(np.exp(2 * cov.hp[1])), float(np.exp(2 * cov.hp[2]))
    for nt in (257, 129):
        Xt = np.ascontiguousarray(Xt_all[-nt:])
        _, _, m, _, lat = truth.standin(cov, X, y, Xt, joint=True)
        lat = np.tril(lat) + np.tril(lat, -1).T
        for with_noise in (True, False):
            S = lat + (sn2 if with_noise else 1e-8 * sf2) * np.eye(nt)        # formed in fp64: this is what is factored
            C = np.linalg.cholesky(S)
            rf = truth.factor_bound_worst(S, C, nt + truth.POTRF_EXTRA_ULPS)
            print("BOUND %s nt=%d %s factor: residual / bound %.4f at %s" % (name, nt, "noise" if with_noise else "latent", rf[0], rf[1]))
            assert rf[0] <= 1.0, (name, nt, with_noise, rf)
            for ns in (7, 129, 257):
                Z = np.random.default_rng(1000 * nt + ns).standard_normal((ns, nt))
                rd = truth.draw_bound_worst(m + Z @ C.T, m, Z, C)
                print("BOUND %s nt=%d ns=%d draws: error / bound %.4f at %s" % (name, nt, ns, rd[0], rd[1]))
                assert rd[0] <= 1.0, (name, nt, ns, with_noise, rd)
