"""CPU checks of the extended-precision truth (tests/truth.py), of the fp64 yardstick taken from the oracle, and of
the committed fixtures under tests/golden/truth -- everything tests/test_gpu_accuracy.py leans on.

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

import truth
import truth_ard
import truth_matern
from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import make_truth  # noqa: E402

pytestmark = pytest.mark.skipif(not truth.EXTENDED, reason="numpy.longdouble is not an extended-precision type here")

_LIVE = {}


def live(oracle, name):
    """Truth, yardstick and stand-in errors of a live case, computed once per session."""
    if name not in _LIVE:
        X, y, Xt, hp = truth.live_inputs(name)
        t = truth.Truth(X, y, hp)
        tm, tv = t.predict(Xt)
        noise, first, rest = truth.noise_level(oracle, X, y, hp, Xt, t.ll, t.grad, tm, tv)
        fl = truth.floors(truth.scales(hp, t.ll, t.grad, tm))
        rows = truth.solve_rows(len(y))
        st = truth.standin(X, y, hp, Xt, solve=True)
        se = truth.errors(*st[:4], t.ll, t.grad, tm, tv)
        se.update(truth.solve_errors(st[4], st[5], t, rows))
        noise.update(truth.noise_level_solve(oracle, X, y, hp, t, rows))
        fl.update(alpha=4 * 2.0 ** -52, kinv=4 * 2.0 ** -52)
        _LIVE[name] = dict(noise=noise, first=first, rest=rest, floor=fl, standin=se)
    return _LIVE[name]


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
    t = truth.Truth(X, y, hp, keep=False)
    tm, tv = t.predict(Xt)
    noise, _, _ = truth.noise_level(oracle, X, y, hp, Xt, t.ll, t.grad, tm, tv)
    fl = truth.floors(truth.scales(hp, t.ll, t.grad, tm))
    ll, g, mean, var = mp_eval(mp, X, y, hp, Xt)
    gs = max(abs(v) for v in g)
    err = dict(ll=abs(to_mp(mp, t.ll) - ll) / abs(ll),
               mean=max(abs(to_mp(mp, tm[k]) - mean[k]) for k in range(3)),
               var=max(abs(to_mp(mp, tv[k]) - var[k]) for k in range(3)))
    for k in range(3):
        err["g%d" % k] = abs(to_mp(mp, t.grad[k]) - g[k]) / gs
    for q in truth.QUANTITIES:
        yard = max(noise[q], fl[q])
        print("n=%d %s: truth error %.3g, yardstick %.3g" % (n, q, float(err[q]), yard))
        assert float(err[q]) <= yard / 100, (n, hp, q, float(err[q]), yard)


# ------------------------------------------------------------------ the yardstick
@pytest.mark.parametrize("name", list(truth.LIVE_CASES))
def test_yardstick_is_sane(oracle, name):
    """The oracle's error on the data as given is no outlier among the 7 permuted evaluations (within F of the largest
    of them, floored like the bound), and no yardstick exceeds 1e-9 of its scale: a broken truth or oracle cannot
    silently loosen the GPU test."""
    c = live(oracle, name)
    for q in truth.QUANTITIES:
        assert c["first"][q] <= truth.F * max(c["rest"][q], c["floor"][q]), (name, q, c["first"][q], c["rest"][q])
        scale = c["floor"][q] / (4 * 2.0 ** -52)      # 1 for LL and gradient (relative errors), else the quantity's scale
        assert c["noise"][q] <= truth.YARDSTICK_CAP * scale, (name, q, c["noise"][q], scale)


def test_F_covers_the_standin(oracle):
    """F and F_SOLVE are the next powers of two at or above twice the largest stand-in / yardstick ratio over the case
    list (docs/ACCURACY.md).  Here: the LAPACK / BLAS-ordered evaluation itself passes the bound the GPU is held to
    on every live case.  The ratios are those of the BLAS this runs on (its blocking and thread count set the order of
    summation): the table in docs/ACCURACY.md is of the build it was measured with, and the factor of two between it
    and F is what is left for another one."""
    for name in truth.LIVE_CASES:
        c = live(oracle, name)
        ratio = {q: c["standin"][q] / max(c["noise"][q], c["floor"][q]) for q in truth.QUANTITIES + truth.SOLVE_QUANTITIES}
        print("STANDIN %-14s " % name + "  ".join("%s %.2f" % (q, r) for q, r in ratio.items()))
        for q, r in ratio.items():
            assert r <= (truth.F_SOLVE if q in truth.SOLVE_QUANTITIES else truth.F), (name, q, r)


# ------------------------------------------------------------------ the fixtures
KEYS = {"case", "n", "d", "hp", "experts", "nt", "ll", "grad", "mean", "var", "noise", "oracle_as_given",
        "oracle_permuted", "seconds"}


@pytest.mark.parametrize("name", sorted(make_truth.CASES))
def test_fixture_loads(name):
    for n in (None, make_truth.SIBLING_ROWS):
        f = make_truth.load(name, n)
        assert set(f["raw"]) == KEYS, set(f["raw"]) ^ KEYS
        assert f["n"] == (make_truth.CASES[name]["n"] if n is None else n) and f["nt"] == make_truth.NT
        assert f["grad"].shape == (3,) and f["mean"].shape == (f["nt"],) and f["var"].shape == (f["nt"],)
        assert set(f["noise"]) == set(truth.QUANTITIES) == set(f["oracle_as_given"]) == set(f["oracle_permuted"])
        assert np.all(np.isfinite(f["mean"].astype(float))) and np.all(f["var"] > 0)
        sv = float(np.exp(2 * f["hp"][1]) + np.exp(2 * f["hp"][2]))
        scale = dict(ll=1.0, g0=1.0, g1=1.0, g2=1.0, mean=float(np.max(np.abs(f["mean"]))), var=sv)
        fl = truth.floors(truth.scales(f["hp"], f["ll"], f["grad"], f["mean"]))
        for q in truth.QUANTITIES:
            # the same two checks as test_yardstick_is_sane: the evaluation on the data as given is no outlier among
            # the permuted ones, and the yardstick stays under its cap
            first, rest = f["oracle_as_given"][q], f["oracle_permuted"][q]
            assert f["noise"][q] == max(first, rest) and min(first, rest) >= 0, (name, n, q)
            assert first <= truth.F * max(rest, fl[q]), (name, n, q, first, rest)
            assert f["noise"][q] <= truth.YARDSTICK_CAP * scale[q], (name, n, q)
        assert os.path.getsize(os.path.join(make_truth.OUT, name + ("" if n is None else "_n%d" % n) + ".json")) < 16384


@pytest.mark.parametrize("name", sorted(make_truth.CASES))
def test_fixture_sibling_regenerates(oracle, name):
    """The 300-row sibling of every fixture comes out of make_truth.py with the committed strings, digit for digit:
    the generator has not drifted from the files."""
    got = make_truth.compute(name, make_truth.SIBLING_ROWS, oracle)
    want = dict(make_truth.load(name, make_truth.SIBLING_ROWS)["raw"])
    want.pop("seconds")
    assert got == want, {k: (got[k], want[k]) for k in got if got[k] != want[k]}


# ------------------------------------------------------------------ beyond one test tile
def wide_ratios(tag, st, tmean, tvar, tcov, sn2, noise, fl):
    """Stand-in error / max(noise, floor) of the means, the variances and the joint covariance (the worse of with and
    without noise; the variances' yardstick and the cov floor, as the GPU tests hold it)."""
    mean, var, cov = st
    cn = cov + float(sn2) * np.eye(len(cov))
    e = truth.joint_errors(mean, var, cn, cov, tmean, tvar, tcov, sn2)
    r = dict(mean=e["mean"] / max(noise["mean"], fl["mean"]), var=e["var"] / max(noise["var"], fl["var"]),
             cov=max(e["cov_noise"], e["cov_latent"]) / max(noise["var"], fl["cov"]))
    print("STANDIN-WIDE %-28s " % tag + "  ".join("%s %.2f" % kv for kv in r.items())
          + "  | yardstick " + " ".join("%s %.1e" % (q, max(noise[q], fl[q])) for q in ("mean", "var")))
    return r


def check_wide_rule(worst, F, name):
    """The project's rule: F is a power of two and at least twice the largest stand-in ratio.  (The factor of a family
    is set over all its rows, so the wide rows alone may ask for less than it, never for more.)"""
    print("largest wide stand-in ratio %.2f -> the rule asks for %d (%s = %d)" % (worst, truth.factor_rule(worst), name, F))
    assert truth.factor_rule(worst) <= F and F & (F - 1) == 0, (worst, truth.factor_rule(worst), F)


def test_wide_standin_se(oracle):
    """truth.WIDE_CASES at their 129 / 200 / 257 test points: the stand-in's means, variances and joint covariance
    (LAPACK / BLAS) against the longdouble truth, over the yardstick of the same test points -> the rule gives F."""
    worst = 0.0
    for name, nts in truth.WIDE_CASES.items():
        t = None
        for nt in nts:
            X, y, Xt, hp = truth.wide_inputs(name, nt)
            t = t or truth.Truth(X, y, hp, keep=False)
            tm, tv = t.predict(Xt)
            tcov = t.joint(Xt, with_noise=False)[1]
            noise, first, rest = truth.noise_level(oracle, X, y, hp, Xt, t.ll, t.grad, tm, tv)
            fl = truth.floors(truth.scales(hp, t.ll, t.grad, tm))
            st = truth.standin_joint(truth.se_fp64(hp), X, y, Xt, float(np.exp(2 * hp[1])), float(np.exp(2 * hp[2])))
            r = wide_ratios("%s nt=%d" % (name, nt), st, tm, tv, tcov, t.sn2, noise, fl)
            worst = max(worst, *r.values())
            for q in ("mean", "var"):                # the yardstick of the wide points is as sane as that of the 64
                assert first[q] <= truth.F * max(rest[q], fl[q]), (name, nt, q, first[q], rest[q])
                assert noise[q] <= truth.YARDSTICK_CAP * fl[q] / (4 * 2.0 ** -52), (name, nt, q, noise[q])
    check_wide_rule(worst, truth.F, "F")


def test_wide_standin_ard(oracle):
    """The ARD case of the wide tests (n257_d3 with truth_ard's length scales, 200 test points) against F_ARD."""
    ta = truth_ard
    X, y, _, hp = ta.ard_inputs("n257_d3")
    Xt = truth.wide_points(X, truth.WIDE_NT_FAMILY, ta.ARD_CASES["n257_d3"][5])
    t = ta.TruthARD(X, y, hp)
    tm, tv = t.predict(Xt)
    tcov = t.joint(Xt, with_noise=False)[1]
    noise, _, _ = ta.noise_level_ard(oracle, X, y, hp, Xt, t.ll, t.grad, tm, tv)
    fl = ta.floors_ard(ta.scales_ard(hp, t.ll, t.grad, tm))
    th, tf, tn = ta.split(hp)
    w, sf2, sn2 = np.exp(-th), np.exp(2 * tf), np.exp(2 * tn)
    st = truth.standin_joint(lambda A, B: sf2 * np.exp(-ta.wsqdist(A, B, w) / 2), X, y, Xt, sf2, sn2)
    r = wide_ratios("ard n257_d3 nt=%d" % len(Xt), st, tm, tv, tcov, t.sn2, noise, fl)
    check_wide_rule(max(r.values()), ta.F_ARD, "F_ARD")


def test_wide_standin_matern(oracle):
    """The Matern case of the wide tests (n300_d17, nu = 5/2, 200 test points) against F_MATERN."""
    tmat, kind = truth_matern, truth_matern.MATERN52
    X, y, Xt, hp = truth.wide_inputs("n300_d17", truth.WIDE_NT_FAMILY)
    t = tmat.TruthMatern(X, y, hp, kind)
    tm, tv = t.predict(Xt)
    tcov = t.joint(Xt, with_noise=False)[1]
    noise = tmat.noise_level_matern(oracle, X, y, hp, Xt, kind, t, tm, tv)[0]
    fl = truth.floors(truth.scales(hp, t.ll, t.grad, tm))
    l2, sf2, sn2 = np.exp(2 * np.asarray(hp, dtype=np.float64))
    st = truth.standin_joint(lambda A, B: tmat.kernel_ld(tmat.sqdist64(A, B) / l2, sf2, kind)[0], X, y, Xt, sf2, sn2)
    r = wide_ratios("matern52 n300_d17 nt=%d" % len(Xt), st, tm, tv, tcov, t.sn2, noise, fl)
    check_wide_rule(max(r.values()), tmat.F_MATERN, "F_MATERN")


WIDE_BCM = ((3 * 300, 3), (5 * 261 + 2, 5))          # tests/test_gpu_predict_wide.py::test_wide_bcm: (rows, experts)
HP_BCM_WIDE = [0.9, 0.2, -1.0]


def test_wide_standin_bcm(oracle):
    """The BCM rows of the wide tests (three 300-row experts, the uneven 5-expert split of 1307 rows; 200 test points):
    truth.standin_bcm's product of experts against truth.bcm_truth, over the yardstick from the oracle's BCM with the
    rows permuted inside each expert -> the rule asks for no more than F."""
    from conftest import synth
    worst = 0.0
    for N, K in WIDE_BCM:
        X, y = synth(N, d=5, seed=N + K, scale=3.0)
        Xt = truth.wide_points(X, truth.WIDE_NT_FAMILY, 3.0)
        tb = truth.bcm_truth(X, y, HP_BCM_WIDE, K, Xt)

        def evaluate(Xp, yp):
            b = oracle.bcm(Xp, yp, K, HP_BCM_WIDE)
            try:
                return (b.loglik()[0], b.grad()) + tuple(b.predict(Xt))
            finally:
                b.close()
        noise, _, _ = truth.noise_level(oracle, X, y, HP_BCM_WIDE, Xt, tb["ll"], tb["grad"], tb["mean"], tb["var"],
                                        evaluate=evaluate, parts=truth.bcm_rows(N, K))
        fl = truth.floors(truth.scales(HP_BCM_WIDE, tb["ll"], tb["grad"], tb["mean"]))
        _, _, m, v = truth.standin_bcm(X, y, HP_BCM_WIDE, K, Xt)
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
    X, y, Xt_all, hp = truth.wide_inputs(name, 257)
    sf2, sn2 = float(np.exp(2 * hp[1])), float(np.exp(2 * hp[2]))
    for nt in (257, 129):
        Xt = np.ascontiguousarray(Xt_all[-nt:])
        m, _, cov = truth.standin_joint(truth.se_fp64(hp), X, y, Xt, sf2, sn2)
        cov = np.tril(cov) + np.tril(cov, -1).T
        for with_noise in (True, False):
            S = cov + (sn2 if with_noise else 1e-8 * sf2) * np.eye(nt)        # formed in fp64: this is what is factored
            C = np.linalg.cholesky(S)
            rf = truth.factor_bound_worst(S, C, nt + truth.POTRF_EXTRA_ULPS)
            print("BOUND %s nt=%d %s factor: residual / bound %.4f at %s" % (name, nt, "noise" if with_noise else "latent", rf[0], rf[1]))
            assert rf[0] <= 1.0, (name, nt, with_noise, rf)
            for ns in (7, 129, 257):
                Z = np.random.default_rng(1000 * nt + ns).standard_normal((ns, nt))
                rd = truth.draw_bound_worst(m + Z @ C.T, m, Z, C)
                print("BOUND %s nt=%d ns=%d draws: error / bound %.4f at %s" % (name, nt, ns, rd[0], rd[1]))
                assert rd[0] <= 1.0, (name, nt, ns, with_noise, rd)
