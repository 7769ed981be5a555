"""Pathwise posterior draws of the matrix-free GP on the GPU (cugp_iter_features_apply / _paths_fit / _paths_eval) against
numpy.longdouble.

The feature product's bound follows k_rff_apply's rounding sequence (docs/ACCURACY.md, "Random-feature product"), u = 2^-53.
A phase term fl(fl(x_f - c_f) fl(omega_kf s_f)) carries 6 u -- the difference 1, the scale 3 (ARD: exp on the host 2;
isotropic: 1 / sqrt(exp(2 theta)) 3) and its product 1, the term's product 1 --, the fma-free chain b_k + d terms gamma_d: a
phase error of (d + 7) u S_ik, S_ik = sum_f |(x - c)_f omega_kf / l_f| + |b_k|, which the cosine (slope <= 1) hands on; the
device library's cos adds 4 ulp <= 8 u |cos|.  The m-term sum (4 per MFMA), the additions of the ranges' blocks (fewer than
the ceil(m / 32) stages), amp = sqrt(2 sf2 / m) formed on the host (3) and its product: gamma_{m + stages + 6} sum_k |cos| |W|."""
import numpy as np
import pytest

import truth
from conftest import synth
from cugp_amd import gp
from test_gpu_iter import FAMILIES, TOL, case, handle, hold, lambda_min, product_bound

pytestmark = pytest.mark.gpu
LD, U, gamma = truth.LD, truth.U, truth.gamma


def features(hp, ard, Xq, c, Om, b, W):
    """-> (amp cos(phase) W [s, nq], its bound), longdouble"""
    d, m = Om.shape[1], len(b)
    ell = np.exp(np.asarray(hp[:d] if ard else [hp[0]] * d, dtype=LD))
    Xc, Ot = Xq.astype(LD) - c.astype(LD), Om.astype(LD) / ell
    C = np.cos(Xc @ Ot.T + b.astype(LD))
    S = np.abs(Xc) @ np.abs(Ot).T + np.abs(b)
    amp, Wa = np.sqrt(2 * np.exp(2 * LD(hp[-2])) / m), np.abs(W).astype(LD)
    return amp * (W.astype(LD) @ C.T), amp * (Wa @ ((d + 7) * U * S + 8 * U * np.abs(C)).T + gamma(m + -(-m // 32) + 6) * (Wa @ np.abs(C).T))


def draws(family, d, m, s, n, seed=0):
    rng = np.random.default_rng(seed + 1000 * m + s)
    alpha = np.exp(FAMILIES[family][0](d)[-3]) if family.startswith("rq") else None
    Om = gp.spectral_frequencies("se" if family == "se_ard" else family, d, m, rng, alpha)
    return Om, rng.uniform(0, 2 * np.pi, m), rng.standard_normal((s, m)), rng.standard_normal((s, n))


BASE = ("se", 65, 33, 17, 3, 0)
CASES = sorted({BASE} | {("se", nq, 33, 17, 3, 0) for nq in (1, 63, 130)} | {("se", 65, m, 17, 3, 0) for m in (1, 31, 100)}
               | {("se", 65, 33, s, 3, 0) for s in (1, 16, 64)} | {(f, 65, 33, 17, d, 0) for f in ("se", "matern52_ard") for d in (1, 16, 17)}
               | {(f, 130, 100, 17, 3, sp) for f in ("se", "matern52_ard") for sp in (1, 3)} | {("se", 130, 160, 17, 3, 3)}
               | {("rq_ard", 65, 33, 17, 3, 0)})


@pytest.mark.parametrize("family,nq,m,s,d,split", CASES)
def test_feature_product_against_longdouble(family, nq, m, s, d, split):
    X, _, hp = case(family, 65, d)[:3]
    Om, b, W, _ = draws(family, d, m, s, 65)
    Xq = None if nq == 65 else synth(nq, d=d, seed=11, scale=4.0 if d <= 3 else 1.8)[0]       # (None: the training rows)
    c = np.linspace(-0.5, 0.5, d)
    g = handle(family, 65, d, split)
    out = g.features_apply(Xq, Om, b, W, c)
    want, bound = features(hp, family.endswith("ard"), X if Xq is None else Xq, c, Om, b, W)
    hold(out, want, bound, "features_apply %s" % ((family, nq, m, s, d, split),))
    assert np.array_equal(out, g.features_apply(Xq, Om, b, W, c))


def test_shifted_data_with_the_default_origin():
    X, y, hp = case("matern52_ard", 65, 3)[:3]
    Om, b, W, _ = draws("matern52_ard", 3, 33, 17, 65)
    g = gp.IterativeGP(65, 3, kernel="matern52_ard")
    g.set_data(X + 1e3, y)
    g.set_loghyper(hp)
    Xq = synth(63, d=3, seed=11, scale=4.0)[0] + 1e3
    want, bound = features(hp, True, Xq, g._origin, Om, b, W)
    assert np.all(np.abs(g._origin - 1e3) < 4.0)
    hold(g.features_apply(Xq, Om, b, W, g._origin), want, bound, "shifted by 1e3")


def test_a_column_carries_the_bits_of_its_own_call():
    Om, b, W, _ = draws("matern52_ard", 3, 100, 17, 65)
    g = handle("matern52_ard", 65, 3)
    out = g.features_apply(None, Om, b, W)
    for c in (0, 5, 16):
        assert np.array_equal(out[c], g.features_apply(None, Om, b, W[c])[0]), c


@pytest.mark.parametrize("family", ["se", "rq_ard"])
def test_zero_weights_give_the_fit_and_the_mean_in_bits(family):
    """cos 0 = 0, y - 0 = y, 0 + x = x: the conditioning is fit's solve and predict's product."""
    n = 150
    Om, b, W, _ = draws(family, 3, 33, 3, n)
    Xt = synth(70, d=3, seed=7, scale=4.0)[0]
    g = handle(family, n, 3)
    assert g.fit(TOL, 4 * n, 7)[2] == 1
    paths = g.sample_paths(3, Omega=Om, b=b, W=0 * W, tol=TOL, max_iter=4 * n, check_every=7)
    mean = g.predict(Xt, var=False)[0]
    out = paths(Xt)
    for c in range(3):
        assert np.array_equal(paths.V[c], g.alpha()) and np.array_equal(out[c], mean), c


@pytest.mark.parametrize("family", ["se", "rq_ard"])
def test_posterior_paths_against_a_direct_solve(family):
    """f = Phi_t w + ks' v, v the device's V with true residual r - K v, r = (y - Phi w) - sn eps: the bound of test_gpu_iter's
    mean, |ks| |r - K v| / lmin plus the product bound at V = v, plus the feature bound at Xt.  The residual itself is held
    to the solve's contract: tol |r| plus the product bound at v plus what the device's right-hand side may differ from r by --
    the feature bound on X and the three roundings of (y - f) - sn eps (sn = exp(theta_n) on the host: 2 more on its term)."""
    n, nt, m, s = 150, 70, 33, 3
    X, y, hp, cov, K, E = case(family, n, 3)
    Xt = synth(nt, d=3, seed=7, scale=4.0)[0]
    Om, b, W, Eps = draws(family, 3, m, s, n)
    g = handle(family, n, 3)
    paths = g.sample_paths(s, Omega=Om, b=b, W=W, Eps=Eps, tol=TOL, max_iter=4 * n, check_every=7)
    assert np.all(paths.info[:, 2] == 1) and np.array_equal(paths.origin, X.mean(axis=0))
    ard, norm = family.endswith("ard"), lambda A: np.sqrt((A * A).sum(-1))
    fx, bx = features(hp, ard, X, paths.origin, Om, b, W)
    ft, bt = features(hp, ard, Xt, paths.origin, Om, b, W)
    noise = np.exp(LD(hp[-1])) * Eps.astype(LD)
    r = (y.astype(LD) - fx) - noise
    V = paths.V.astype(LD)
    res = norm(r - V @ K.T)
    rhs = bx + U * (np.abs(y.astype(LD) - fx) + 4 * np.abs(noise) + np.abs(r))
    print("true residual / (tol |r|):", np.asarray(res / norm(r) / TOL, dtype=float))
    assert np.all(res <= TOL * (norm(r) + norm(rhs)) + norm(product_bound(K, E, paths.V, n)) + norm(rhs))
    Ks = cov.k(Xt.astype(LD), X.astype(LD))
    Kinv = truth.gram_lower(truth.tri_inverse(truth.cholesky(K)))
    bound = bt + product_bound(Ks, FAMILIES[family][2](Xt, X, cov), paths.V, n) + np.outer(res, norm(Ks)) / lambda_min(K)
    hold(paths(Xt), ft + (r @ Kinv.T) @ Ks.T, bound + U * np.abs(ft + V @ Ks.T), "paths(Xt) " + family)
