"""The pivoted-Cholesky preconditioner of the matrix-free exact GP (cugp_iter_set_precond) on the GPU
against numpy.longdouble: the factor along the device's own pivots, M^-1 V from the device's own L, the preconditioned
solver under test_gpu_iter.py's contract, and the states a handle goes through.  Bounds: docs/ACCURACY.md ("Pivoted-
Cholesky preconditioner"): F times the larger of a plain fp64 numpy replay's own error and a floor of 4 ulp."""
import numpy as np
import pytest

import pchol_ref as pr
import truth
from conftest import synth
from cugp_amd import capi, gp
from test_gpu_iter import FAMILIES, TOL, case, handle, hold, lambda_min, product_bound, vectors

pytestmark = pytest.mark.gpu
LD, ULP = truth.LD, 2.0 ** -52
OTHERS = ("se_ard", "matern32", "matern52_ard", "rq", "rq_ard")
FACTOR = ([("se", n, r, 3) for n, r in ((1, 1), (63, 16), (65, 17), (257, 64), (257, 130))]
          + [(f, n, r, d) for f in OTHERS for n, r, d in ((65, 17, 17), (257, 33, 1))])


def precond(family, n, d, rank):
    g = handle(family, n, d)
    g.set_precond(rank)
    return g


def noiseless(family, n, d):
    """(Kf in longdouble, Kf evaluated in fp64 numpy, the descriptor)"""
    X, _, _, cov, K, _ = case(family, n, d)
    Kf = K.copy()
    Kf[np.arange(n), np.arange(n)] -= cov.sn2
    return Kf, cov.fp64().k(X, X).astype(np.float64), cov


@pytest.mark.parametrize("family,n,r,d", FACTOR)
def test_factor(family, n, r, d):
    Kf, K64, cov = noiseless(family, n, d)
    g = precond(family, n, d, r)
    info = g.precond_info()
    L, piv = g.precond_factor()
    a = info["achieved"]
    assert info["rank"] == r and info["built"] == 1 and info["rp"] == -(-r // 64) * 64 and 1 <= a <= r
    assert L.shape == (n, a) and len(set(piv.tolist())) == a
    Lt, hist = pr.replay(Kf, list(piv))
    yard = float(np.abs(pr.replay(K64, list(piv))[0] - Lt).max())
    root = float(np.sqrt(cov.sf2))
    bound = pr.F_PCHOL * max(yard, 4 * ULP * root)
    print("yardstick %.3g" % yard)
    hold(L, Lt, bound, "L")
    for k, p in enumerate(piv):                       # (a) |d dres| <= sum_m (2 |l_m| + b) b <= 2 (k + 1) sqrt(sf2) b
        assert hist[k][p] >= hist[k].max() - 2 * (k + 1) * root * bound, (k, p)
        assert np.all(L[p, k + 1:] == 0) and L[p, k] > 0                        # (c)


OPERATOR = [("se", n, r, t) for n, r, t in ((1, 1, 1), (63, 15, 1), (64, 16, 17), (65, 17, 33), (257, 64, 17), (257, 130, 65))]


@pytest.mark.parametrize("family,n,r,t", OPERATOR + [("rq_ard", 257, 64, 17)])
def test_operator(family, n, r, t):
    sn2 = float(case(family, n, 3)[3].sn2)
    g = precond(family, n, 3, r)
    L = g.precond_factor()[0]
    V = vectors(t, n)
    out = g.precond_apply(V)
    want = pr.apply_truth(L, sn2, V)
    yard = float(np.abs(pr.apply(L, sn2, V) - want).max())
    bound = pr.F_PCAPPLY * max(yard, 4 * ULP * float(np.abs(V).max()) / sn2)
    print("yardstick %.3g" % yard)
    hold(out, want, bound, "M^-1 V")
    assert t == 1 or np.all(out[-1] == 0)
    u, v = V[0].astype(LD), V[t // 2].astype(LD)
    assert abs(u @ out[t // 2].astype(LD) - v @ out[0].astype(LD)) <= bound * (np.abs(u).sum() + np.abs(v).sum())
    assert np.array_equal(out, g.precond_apply(V)) and np.array_equal(out, precond(family, n, 3, r).precond_apply(V))
    for c in {0, t // 2, t - 1}:
        assert np.array_equal(out[c], g.precond_apply(V[c])[0]), c
    if t > 17:
        assert np.array_equal(out[:17], g.precond_apply(V[:17]))


@pytest.mark.parametrize("family", ["se", "rq_ard"])
def test_solver_and_prediction(family):
    """test_gpu_iter.py's contract under the preconditioner, and at most half the sweeps of rank 0 (the fp64 reference on the
    CPU: 14 against 96 sweeps for se, 16 against 92 for rq_ard)."""
    n = 257
    X, y, hp, cov, K, E = case(family, n, 3)
    B = vectors(17, n)
    g = precond(family, n, 3, 64)
    Xs, info = g.solve(B, TOL, 4 * n, 7)
    plain = handle(family, n, 3).solve(B, TOL, 4 * n, 7)
    print("sweeps", info[:, 0].max(), "against", plain[1][:, 0].max())
    assert np.all(info[:, 2] == 1) and np.all(info[:, 3] == 0) and np.all(info[:, 1] <= TOL)
    assert np.all(Xs[-1] == 0) and info[-1, 0] == 0 and 2 * info[:, 0].max() <= plain[1][:, 0].max()
    R = B.astype(LD) - Xs.astype(LD) @ K.T
    Kinv = truth.gram_lower(truth.tri_inverse(truth.cholesky(K)))
    D = Xs.astype(LD) - B.astype(LD) @ Kinv.T
    lmin = lambda_min(K)
    assert np.all(np.sqrt((D * D).sum(1)) <= np.sqrt((R * R).sum(1)) / lmin)
    g.set_precond(0)                                   # rank 0 again: the bits of a handle that never had one
    again = g.solve(B, TOL, 4 * n, 7)
    assert np.array_equal(again[0], plain[0]) and np.array_equal(again[1], plain[1])
    g.set_precond(64)
    Xt = synth(65, d=3, seed=7, scale=4.0)[0]
    assert g.fit(TOL, 4 * n, 7)[2] == 1
    mean, var, vinfo = g.predict(Xt, True, TOL, 4 * n, 7)
    assert np.all(vinfo[:, 2] == 1)
    t = truth.Truth(X, y, cov)                         # the bounds of test_gpu_iter.py::test_prediction, term for term
    tmean, tvar = t.predict(Xt)
    Ks, Ek = cov.k(Xt.astype(LD), X.astype(LD)), FAMILIES[family][2](Xt, X, cov)
    norm = lambda A: np.sqrt((A * A).sum(-1))
    a = g.alpha()
    hold(mean, tmean, product_bound(Ks, Ek, a[None, :], n)[0] + norm(Ks) * norm(y.astype(LD) - K @ a.astype(LD)) / lmin, "mean")
    W = Ks @ t.Kinv
    aw = np.abs(Ks) * np.abs(W)
    rw = TOL * norm(Ks) + norm(product_bound(K, E, W, n))
    hold(var, tvar, norm(Ks) * rw / lmin + truth.gamma(n + 2) * aw.sum(1) + 2 * (Ek * aw).sum(1)
         + truth.U * (t.sf2 + t.sn2 + np.abs(tvar)), "var")


def test_stale_factor_is_rebuilt():
    X, y, hp, _, _, _ = case("se", 65, 3)
    B = vectors(3, 65)
    g = precond("se", 65, 3, 17)
    first = g.solve(B, TOL, 260, 7)
    hp2 = [hp[0] - 0.3] + hp[1:]
    g.set_loghyper(hp2)
    f = gp.IterativeGP(65, 3)
    f.set_data(X, y)
    f.set_loghyper(hp2)
    f.set_precond(17)
    for a, b in zip(g.solve(B, TOL, 260, 7) + g.precond_factor(), f.solve(B, TOL, 260, 7) + f.precond_factor()):
        assert np.array_equal(a, b)
    g.set_loghyper(hp)
    g.set_data(X, y)
    again = g.solve(B, TOL, 260, 7)
    assert np.array_equal(again[0], first[0]) and np.array_equal(again[1], first[1])


def test_early_end_nan_and_refusals():
    X, y, hp, cov, _, _ = case("se", 65, 3)
    Xr = X[np.arange(65) % 20]
    g = precond("se", 65, 3, 64)
    g.set_data(Xr, y)
    info = g.precond_info()
    L = g.precond_factor()[0]
    assert 1 <= info["achieved"] <= 20 and L.shape == (65, info["achieved"])
    K = cov.k(Xr.astype(LD), Xr.astype(LD)) + cov.sn2 * np.eye(65, dtype=LD)
    B = vectors(3, 65)
    Xs, sinfo = g.solve(B, TOL, 260, 7)
    assert np.all(sinfo[:, 2] == 1)
    R = B.astype(LD) - Xs.astype(LD) @ K.T
    D = Xs.astype(LD) - B.astype(LD) @ truth.gram_lower(truth.tri_inverse(truth.cholesky(K))).T
    assert np.all(np.sqrt((D * D).sum(1)) <= np.sqrt((R * R).sum(1)) / lambda_min(K))
    Xn = X.copy()
    Xn[7] = np.nan
    g.set_data(Xn, y)
    Xs, sinfo = g.solve(B, TOL, 260, 7)                # CUGP_OK: no factor, or NaN columns by the breakdown contract
    assert g.precond_info()["achieved"] == 0 or np.all(np.isnan(Xs[:-1]))
    assert np.all(np.isnan(Xs[:-1])) and np.all(sinfo[:-1, 3] == 1) and np.all(Xs[-1] == 0)
    g.set_data(X, y)
    for rank in (-1, 66, 513):
        with pytest.raises(capi.CugpError) as e:
            g.set_precond(rank)
        assert e.value.code == capi.CUGP_ERR_INVALID and "cugp_iter_set_precond" in str(e.value)
    assert g.precond_info()["rank"] == 64 and np.all(g.solve(B, TOL, 260, 7)[1][:, 2] == 1)
