"""The matrix-free GP's mixed mode on the GPU (cugp_iter_set_precision, cugp_iter_apply32): the fp32
product against numpy.longdouble under mixed_ref.py's yardstick, its bits, the solver that sweeps on it and verifies in
fp64, the fall back to fp64 where fp32 cannot refine K, and NaN / mode handling."""
import numpy as np
import pytest

import mixed_ref as mr
import truth
from conftest import synth
from cugp_amd import capi, gp
from test_gpu_iter import lambda_min

pytestmark = pytest.mark.gpu
LD = truth.LD
TOL = 1e-10
LOG_SN = 0.2 - 0.5 * np.log(1e4)                      # sf2 / sn2 = 1e4 at log sf = 0.2


@pytest.mark.parametrize("family,n,d,t,split", mr.PRODUCT)
def test_product_against_truth(family, n, d, t, split):
    X, _, _, K, M = mr.case(family, n, d)
    V = mr.vectors(t, n)
    if split:
        assert gp.IterativeGP.plan(n, n, t, split)["split"] == split
    out = mr.handle(family, n, d, split=split).apply(V, precision="fp32")
    err, Y = np.abs(out.astype(LD) - V.astype(LD) @ K.T), mr.yardstick(M, V)
    print("largest error / Y: %.3g (F_MIX %g)" % (float(np.max(err / Y)), mr.F_MIX))
    assert np.all(err <= mr.F_MIX * Y)


def test_bits():
    g, V = mr.handle("rq_ard", 65, 3), mr.vectors(17, 65)
    out = g.apply(V, precision="fp32")
    assert np.array_equal(out, g.apply(V, precision="fp32"))
    for c in (0, 1, 2, 16):
        assert np.array_equal(out[c], g.apply(V[c], precision="fp32")[0]), c
    E = np.eye(65)
    cols = g.apply(E[[0, 5, 31, 64]], precision="fp32")                 # e_j' K32: row j of the operator
    for (a, i), (b, j) in (((0, 0), (3, 64)), ((1, 5), (2, 31)), ((2, 31), (3, 64))):
        assert cols[a][j] == cols[b][i] and cols[a][j] != 0, (i, j)


def residual(K, B, Xs):
    R = B.astype(LD) - Xs.astype(LD) @ K.T
    return np.sqrt((R * R).sum(1)) / np.sqrt((B.astype(LD) ** 2).sum(1))


@pytest.mark.parametrize("family", ["se", "rq_ard"])
def test_solver_and_prediction(family):
    n = 300
    X, y, hp, K, _ = mr.case(family, n, 3, LOG_SN)
    B = np.random.default_rng(5).standard_normal((3, n))
    g, f = mr.handle(family, n, 3, LOG_SN), mr.handle(family, n, 3, LOG_SN)
    g.set_precision("mixed")
    Xs, info = g.solve(B, TOL, 40 * n, 10)
    st = g.solve_stats()
    print("sweeps", info[:, 0], "stats", st, "residual / tol", np.asarray(residual(K, B, Xs) / TOL, dtype=float))
    assert np.all(info[:, 2] == 1) and np.all(info[:, 3] == 0) and np.all(info[:, 1] <= TOL)
    assert np.all(residual(K, B, Xs) <= 2 * TOL)
    assert st["fp32_products"] > 0 and st["fell_back"] == 0 and st["verifications"] == st["fp64_products"]
    # two tol-certified solves of K x = b differ by at most 2 tol |b| / lambda_min
    Xt = synth(5, d=3, seed=7, scale=4.0)[0]
    lmin = lambda_min(K)
    res = []
    for h in (g, f):
        assert h.fit(TOL, 40 * n, 10)[2] == 1
        mean, var, vinfo = h.predict(Xt, True, TOL, 40 * n, 10)
        assert np.all(vinfo[:, 2] == 1)
        res.append((mean, var))
    cov = mr.FAMILIES[family][3](hp)
    Ks = cov.k(Xt.astype(LD), X.astype(LD))
    nk, ny = np.sqrt((Ks * Ks).sum(1)), np.sqrt((y.astype(LD) ** 2).sum())
    slack = 1 + 1e-3
    assert np.all(np.abs(res[0][0] - res[1][0]) <= 2 * TOL * nk * ny / lmin * slack)
    assert np.all(np.abs(res[0][1] - res[1][1]) <= 2 * TOL * nk * nk / lmin * slack)


def test_fallback():
    """Near-duplicate rows and sn2 = 1e-10 sf2: cond(K) > 2^24, fp32 cannot refine; a numerical condition, not a fault.
    cond(K) is 5e11 here: plain fp64 CG in numpy reaches 1e-4 in about 8 n sweeps and does not reach 1e-10 in 400 n, so the
    tolerance is 1e-4 and max_iter 40 n -- the fp64 mode converges, and the residual check below has columns to check."""
    n, tol = 200, 1e-4
    X, y, hp, _, _ = mr.case("se", n, 3)
    X = X.copy()
    X[100:] = X[:100] + 1e-9
    hp = hp[:2] + [hp[1] - 0.5 * np.log(1e10)]
    cov = truth.SE(hp)
    K = cov.k(X.astype(LD), X.astype(LD)) + cov.sn2 * np.eye(n, dtype=LD)
    ev = np.linalg.eigvalsh(K.astype(np.float64))
    assert ev[-1] / max(ev[0], float(cov.sn2)) > 2.0 ** 24
    B = np.random.default_rng(6).standard_normal((3, n))
    got = []
    for mode in ("mixed", "fp64"):
        g = gp.IterativeGP(n, 3)
        g.set_data(X, y)
        g.set_loghyper(hp)
        g.set_precision(mode)
        got.append(g.solve(B, tol, 40 * n, 10) + (g.solve_stats(),))
    (Xm, im, sm), (Xf, i64, s64) = got
    print("sweeps mixed", im[:, 0], "fp64", i64[:, 0], "stats", sm, "residual / tol", np.asarray(residual(K, B, Xm) / tol, dtype=float))
    assert sm["fell_back"] == 1 and s64["fell_back"] == 0 and s64["fp32_products"] == 0
    assert np.array_equal(im[:, 2], i64[:, 2]) and np.all(im[:, 3] == 0)
    done = im[:, 2] == 1
    assert done.any() and np.all(residual(K, B, Xm)[done] <= 2 * tol)


def test_nan_mode_and_refusals():
    X, y, hp, _, _ = mr.case("se", 65, 3)
    B = np.random.default_rng(7).standard_normal((2, 65))
    g = mr.handle("se", 65, 3)
    want = g.solve(B, TOL, 260, 7)
    g.set_precision("mixed")
    Xn = X.copy()
    Xn[7] = np.nan
    g.set_data(Xn, y)
    Xs, info = g.solve(B, TOL, 260, 7)
    assert np.all(np.isnan(Xs)) and np.all(info[:, 3] == 1) and np.all(info[:, 2] == 0)
    assert np.all(np.isnan(g.apply(B, precision="fp32")))
    g.set_data(X, y)
    for mode, drop in ((2, 0.0), (1, 1.0), (1, -0.5), (1, np.nan)):
        assert capi.lib().cugp_iter_set_precision(g._h, mode, drop) == capi.CUGP_ERR_INVALID
    assert g.solve(B, TOL, 260, 7)[1][0, 2] == 1 and g.solve_stats()["fp32_products"] > 0      # (still mixed)
    g.set_precision("fp64")
    again = g.solve(B, TOL, 260, 7)
    assert np.array_equal(again[0], want[0]) and np.array_equal(again[1], want[1])
    e = gp.IterativeGP(65, 3)                          # neither data nor theta
    with pytest.raises(capi.CugpError) as err:
        e.apply(B, precision="fp32")
    assert err.value.code == capi.CUGP_ERR_INVALID and "cugp_iter_apply32" in str(err.value)
