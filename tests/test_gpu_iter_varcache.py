"""The variance cache on the GPU (cugp_iter_varcache_*, cugp_iter_predict_cached) against numpy.longdouble.

Yardstick: var_bound() is test_gpu_iter.test_prediction's bound on predict's variance (TOL = 1e-10, the same K, so the same
cond(K)), computed from the truth.  The cached variance is held to F_VC x it at full rank (truth: the exact variance) and to
F_VCK x it at partial rank (truth: the Galerkin variance of the SAME block Krylov space, built in longdouble by block Arnoldi
with double orthogonalisation from the same start block).  F = 4 x the largest error / yardstick of the fp64 numpy stand-in
(tools/varcache_standin.py) on these very cases; docs/ACCURACY.md, "Variance cache", lists the ratios.

Factor contract, counted in u = 2^-53 for unit columns q: an entry of Q'Q - I is what one projection step leaves -- the
coefficient q'w is a dot product of n terms (n u), the update w - Q c adds k + 1 terms per entry (k + 1), the scaling by
T^-1 three more -- and the second CholQR round forms the same dot products again: 2 (n + k + 4) u = c k u with
c = 2 (n + k + 4) / k.  An entry of H - Q'KQ: the product's (n + 2) u + E per entry of K, the projection's n u, both times
|K|_2 (the families here have positive entries, so | |q|'|K||q'| | <= |K|_2), and the k columns' loss of orthogonality
times |K|_2 each: (2 n + 2 + E / u + k * 2 (n + k + 4)) u |K|_2."""
import functools

import numpy as np
import pytest

import test_gpu_iter as ti
import truth
import truth_ard_matern as tam
import truth_matern as tm
from conftest import synth
from cugp_amd import capi, gp

pytestmark = pytest.mark.gpu
LD, U, gamma = truth.LD, truth.U, truth.gamma
F_VC, F_VCK = 4 * 3.97e-7, 4 * 1.56e-7     # stand-in: tools/varcache_standin.py (docs/ACCURACY.md, "Variance cache")

# the seven instantiations of k_cov_var: test_gpu_iter's six families and the two Matern forms it leaves out
FAMILIES = dict(ti.FAMILIES)
FAMILIES["matern52"] = (FAMILIES["matern32"][0], lambda hp: truth.Matern(hp, 2),
                        lambda A, B, c: tm.k_entry_bound(tm.a_of(A, B, c.hp, 2), A.shape[1], 2))
FAMILIES["matern32_ard"] = (FAMILIES["matern52_ard"][0], lambda hp: tam.ARDMatern(hp, 1),
                            lambda A, B, c: tam.k_entry_bound(tam.a_of(A, B, c), A.shape[1], 1))
SEVEN = ("se", "se_ard", "matern32", "matern32_ard", "matern52", "matern52_ard", "rq_ard")
D = 3


@functools.lru_cache(maxsize=None)
def case(family, n):
    """test_gpu_iter.case for all of FAMILIES, with the truth and the start block: y and 15 Rademacher rows."""
    truth.require_extended()
    X, y = synth(n, d=D, seed=3 * n + D, scale=4.0)
    hp = FAMILIES[family][0](D)
    cov = FAMILIES[family][1](hp)
    t = truth.Truth(X, y, cov)
    B = np.vstack([y[None, :], gp.rademacher(np.random.default_rng(n), 15, n)])
    return X, y, hp, cov, t, FAMILIES[family][2](X, X, cov), B


def handle(family, n, split=0):
    X, y, hp = case(family, n)[:3]
    g = gp.IterativeGP(n, D, kernel="se" if family == "se_ard" else family, ard=family == "se_ard")
    g.set_data(X, y)
    g.set_loghyper(hp)
    g.set_split(split)
    g.fit(ti.TOL, 4 * n, 7)                    # predict(var="cached") returns the mean too, as predict does
    return g


def points(family, n, nt):
    Xt = synth(nt, d=D, seed=7, scale=4.0)[0]
    Xt[0] = case(family, n)[0][n // 2]
    return Xt


@functools.lru_cache(maxsize=None)
def var_bound(family, n, nt):
    """-> (exact variance, test_prediction's bound bv on predict's variance) at points(family, n, nt), longdouble"""
    X, y, hp, cov, t, E, _ = case(family, n)
    Xt = points(family, n, nt)
    Ks = cov.k(Xt.astype(LD), X.astype(LD))
    Ek = FAMILIES[family][2](Xt, X, cov)
    norm = lambda A: np.sqrt((A * A).sum(-1))
    W = Ks @ t.Kinv
    rw = ti.TOL * norm(Ks) + norm(ti.product_bound(t.K, E, W, n))
    aw = np.abs(Ks) * np.abs(W)
    tvar = t.predict(Xt)[1]
    return tvar, norm(Ks) * rw / ti.lambda_min(t.K) + gamma(n + 2) * aw.sum(1) + 2 * (Ek * aw).sum(1) + U * (t.sf2 + t.sn2 + np.abs(tvar))


def krylov_basis(K, B, rank):
    """Orthonormal columns [n, rank] spanning the first `rank` of [B', K B', K^2 B', ...] (block width len(B)): block Arnoldi
    with classical Gram-Schmidt twice against everything before and a column-wise pass twice inside the block, in K's dtype."""
    Q = np.zeros((K.shape[0], 0), dtype=K.dtype)
    W = B.T.astype(K.dtype)
    while Q.shape[1] < rank:
        for c in range(min(W.shape[1], rank - Q.shape[1])):
            w = W[:, c]
            for _ in range(2):
                w = w - Q @ (Q.T @ w)
            Q = np.hstack([Q, (w / np.sqrt(w @ w))[:, None]])
        W = K @ Q[:, -W.shape[1]:]
    return Q


@functools.lru_cache(maxsize=None)
def galerkin_var(family, n, rank, nt):
    """The Galerkin variance prior - ks' Q (Q'KQ)^-1 Q' ks of the block Krylov space of case()'s start block, longdouble"""
    X, _, _, cov, t, _, B = case(family, n)
    Q = krylov_basis(t.K, B, rank)
    Ks = cov.k(points(family, n, nt).astype(LD), X.astype(LD))
    Z = (Ks @ Q) @ truth.tri_inverse(truth.cholesky(Q.T @ t.K @ Q)).T
    return t.sf2 + t.sn2 - (Z * Z).sum(1)


@pytest.mark.parametrize("n", [48, 40])
@pytest.mark.parametrize("family", SEVEN)
def test_exact_at_full_rank(family, n):
    """rank = n: three block steps, the last exactly full (48) or ragged (40); nt = 70 is more than one 64-row workgroup"""
    g = handle(family, n)
    info = g.variance_cache(n, case(family, n)[6])
    assert info == {"achieved": n, "rp": 64, "products": 3, "reason": 0}
    for nt in (5, 70):
        tvar, bv = var_bound(family, n, nt)
        ti.hold(g.predict(points(family, n, nt), var="cached")[1], tvar, F_VC * bv, "cached var, full rank, nt %d" % nt)


@pytest.mark.parametrize("n", [200, 257])
@pytest.mark.parametrize("family", ["se", "rq_ard"])
def test_galerkin_conservative_and_monotone(family, n):
    assert np.linalg.cond(case(family, n)[4].K.astype(np.float64)) <= 1e4
    g, nt, var = handle(family, n), 70, {}
    tvar, bv = var_bound(family, n, nt)
    for rank in (32, 64):
        assert g.variance_cache(rank, case(family, n)[6])["achieved"] == rank
        mean, var[rank], _ = g.predict(points(family, n, nt), var="cached")
        assert np.array_equal(mean, g.predict(points(family, n, nt), var=False)[0])
        ti.hold(var[rank], galerkin_var(family, n, rank, nt), F_VCK * bv, "cached var, rank %d" % rank)
        assert np.all(var[rank].astype(LD) >= tvar - F_VCK * bv)
    assert np.all(var[64].astype(LD) <= var[32].astype(LD) + F_VCK * bv)


@pytest.mark.parametrize("family,n,rank", [("se", 200, 64), ("rq_ard", 257, 32)])
def test_factor_contract(family, n, rank):
    g = handle(family, n)
    g.variance_cache(rank, case(family, n)[6])
    Q, R, H = g.variance_cache_factor()
    K, E = case(family, n)[4].K, case(family, n)[5]
    Ql, k2 = Q.astype(LD), np.linalg.norm(K.astype(np.float64), 2)
    eq = np.abs(Ql @ Ql.T - np.eye(rank)).max()
    eh = np.abs(Ql @ K @ Ql.T - H.astype(LD)).max() / k2
    cq = 2 * (n + rank + 4)
    chh = 2 * n + 2 + float(np.max(E)) / U + rank * cq
    print("|Q'Q - I| / (c k u) %.3g, |Q'KQ - H| / (|K| c k u) %.3g" % (eq / (cq * U), eh / (chh * U)))
    assert eq <= cq * U and eh <= chh * U
    L = np.linalg.cholesky(H)
    assert np.abs(R.T @ L.T - Q.T).max() <= 64 * rank * U * np.linalg.cond(H)      # R L' = Q by substitution


def test_ends():
    g = handle("se", 20)                                        # the second block has 4 live columns
    B = case("se", 20)[6]
    assert g.variance_cache(20, B) == {"achieved": 20, "rp": 64, "products": 2, "reason": 0}
    tvar, bv = var_bound("se", 20, 5)
    ti.hold(g.predict(points("se", 20, 5), var="cached")[1], tvar, F_VC * bv, "n = 20")
    g, B = handle("se", 200), case("se", 200)[6].copy()
    B[1] = B[0]                                                 # the second column repeats the first: the basis ends there
    info = g.variance_cache(64, B)
    assert info["achieved"] == 1 and info["reason"] == 1
    assert all(np.all(np.isfinite(A)) for A in g.variance_cache_factor())
    assert np.all(np.isfinite(g.predict(points("se", 200, 5), var="cached")[1]))
    info = g.variance_cache(16, np.zeros((16, 200)))            # a start block of zeros: rank 0, the prior
    assert info["achieved"] == 0 and np.all(g.predict(points("se", 200, 5), var="cached")[1] == np.exp(0.4) + np.exp(-2.0))


@pytest.mark.parametrize("split", [0, 3])
def test_bits(split):
    n, B = 200, case("rq_ard", 200)[6]
    g, g2 = handle("rq_ard", n, split), handle("rq_ard", n, split)
    Xt = points("rq_ard", n, 70)
    before = g.predict(Xt[:3], True, ti.TOL, 4 * n, 7)
    g.variance_cache(64, B)
    g2.variance_cache(64, B)
    assert np.array_equal(g.variance_cache_factor()[1], g2.variance_cache_factor()[1])
    var = g.predict(Xt, var="cached")[1]
    for i in (0, 63, 64, 69):
        assert np.array_equal(var[i:i + 1], g.predict(Xt[i], var="cached")[1]), i
    after = g.predict(Xt[:3], True, ti.TOL, 4 * n, 7)
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    g.set_loghyper(case("rq_ard", n)[2])
    assert g.variance_cache_info()["achieved"] == 0
    with pytest.raises(capi.CugpError):
        g.predict(Xt, var="cached")
