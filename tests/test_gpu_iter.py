"""The matrix-free exact GP on the GPU (cugp_iter_*, gp.IterativeGP) against numpy.longdouble: the fused product K V, its
rectangular and split forms, determinism, the conjugate-gradient solver's contract and the prediction built on them.

Every bound is computed here from the truth.  The product bound: with K never rounded to storage, out_ic is a sum of nb
products of computed entries k_ij (1 + e_ij), |e_ij| <= E_ij, added in some fixed order (4 per MFMA, fused or not) and, in
the square form, one fma with sn2:  |out_ic - truth_ic| <= sum_j (gamma_{nb+2} + E_ij) |K_ij| |V_jc|.
E: SE 4.5e-16; Matern and RQ the entry bounds of truth_matern / truth_ard_matern / truth_rq; ARD-SE
counted along the kernel in u = 2^-53: difference 1, w_c = exp(-theta_c) on the host 2, product 1 -> 4; the square 2 * 4 + 1,
the d-term sum of positive terms d - 1 -> s: d + 8; -s / 2 exact; exp turns the argument's absolute error (s / 2)(d + 8) u
into a relative one and adds its own 2; sf2 on the host 2, the product 1:  E = (5 + (s / 2)(d + 8)) u."""
import functools

import numpy as np
import pytest

import truth
import truth_ard_matern as tam
import truth_matern as tm
import truth_rq as trq
from conftest import synth
from cugp_amd import capi, gp

pytestmark = pytest.mark.gpu
LD, U, gamma = truth.LD, truth.U, truth.gamma
TOL = 1e-10


def _ls(d):
    return np.linspace(0.7, 1.3, d).tolist()


def _e_ard_se(A, B, c):
    return (5 + tam.wsqdist64(A, B, np.asarray(c.w, dtype=np.float64)) / 2 * (A.shape[1] + 8)) * U


# family -> (d -> theta, theta -> descriptor, (A, B, descriptor) -> E)
FAMILIES = {
    "se": (lambda d: [0.9, 0.2, -1.0], truth.SE, lambda A, B, c: 4.5e-16),
    "se_ard": (lambda d: _ls(d) + [0.2, -1.0], truth.ARD, _e_ard_se),
    "matern32": (lambda d: [0.9, 0.2, -1.0], lambda hp: truth.Matern(hp, 1),
                 lambda A, B, c: tm.k_entry_bound(tm.a_of(A, B, c.hp, 1), A.shape[1], 1)),
    "matern52_ard": (lambda d: _ls(d) + [0.2, -1.0], lambda hp: tam.ARDMatern(hp, 2),
                     lambda A, B, c: tam.k_entry_bound(tam.a_of(A, B, c), A.shape[1], 2)),
    "rq": (lambda d: [0.9, 0.4, 0.2, -1.0], lambda hp: trq.RQ(hp, tied=True),
           lambda A, B, c: trq.k_entry_bound(trq.true_u(A, B, c), float(c.alpha), A.shape[1])[0]),
    "rq_ard": (lambda d: _ls(d) + [0.4, 0.2, -1.0], trq.RQ,
               lambda A, B, c: trq.k_entry_bound(trq.true_u(A, B, c), float(c.alpha), A.shape[1])[0]),
}


@functools.lru_cache(maxsize=None)
def case(family, n, d):
    """-> (X, y, theta, descriptor, K = Kf + sn2 I in longdouble, E of the square): computed once, never changed."""
    truth.require_extended()
    X, y = synth(n, d=d, seed=3 * n + d, scale=4.0 if d <= 3 else 1.8)
    hp = FAMILIES[family][0](d)
    cov = FAMILIES[family][1](hp)
    K = cov.k(X.astype(LD), X.astype(LD))
    K[np.arange(n), np.arange(n)] += cov.sn2
    return X, y, hp, cov, K, FAMILIES[family][2](X, X, cov)


def handle(family, n, d, split=0):
    X, y, hp = case(family, n, d)[:3]
    g = gp.IterativeGP(n, d, kernel="se" if family == "se_ard" else family, ard=family == "se_ard")
    g.set_data(X, y)
    g.set_loghyper(hp)
    g.set_split(split)
    return g


def vectors(t, n, seed=0):
    V = np.random.default_rng(100 * t + n + seed).standard_normal((t, n))
    if t > 1:
        V[-1] = 0.0
    return V


def product_bound(K, E, V, nb):
    """[t, na]: sum_j (gamma_{nb+2} + E_ij) |K_ij| |V_jc|"""
    return (np.abs(V).astype(LD) @ ((gamma(nb + 2) + E) * np.abs(K)).T)


def lambda_min(K):
    """A lower bound on the smallest eigenvalue of the truth's K: Weyl, lambda_min(K) >= lambda_min(K64) - |K - K64|_2 with
    the Frobenius norm for the 2-norm, less LAPACK's backward error n u |K64|_2 of the computed eigenvalue."""
    K64 = K.astype(np.float64)
    ev = np.linalg.eigvalsh(K64)
    D = K - K64.astype(LD)
    return LD(ev[0]) - np.sqrt((D * D).sum()) - len(K) * U * LD(ev[-1])


def hold(out, want, bound, what):
    err = np.abs(out.astype(LD) - want)
    with np.errstate(all="ignore"):
        print("%s: largest error / bound %.3g" % (what, float(np.max(np.where(err == 0, 0, err / bound)))))
    assert np.all(err <= bound), what


NS, TS = (1, 3, 63, 64, 65, 129, 257), (1, 15, 16, 17, 33)
PRODUCT = ([("se", n, t, 3) for n in NS for t in TS] + [("se", n, 16, 3) for n in (31, 32, 33)]      # (stage edge: 32 rows)
           + [("se", 65, 17, 1), ("se", 129, 16, 17)]
           + [(f, n, t, d) for f in ("se_ard", "matern32", "matern52_ard", "rq", "rq_ard") for n, t, d in ((65, 17, 17), (257, 33, 1))])


@pytest.mark.parametrize("family,n,t,d", PRODUCT)
def test_product_against_truth(family, n, t, d):
    _, _, _, _, K, E = case(family, n, d)
    V = vectors(t, n)
    out = handle(family, n, d).apply(V)
    assert np.all(out[-1] == 0) or t == 1
    hold(out, V.astype(LD) @ K.T, product_bound(K, E, V, n), "apply")


@pytest.mark.parametrize("nt", [1, 65, 129])
@pytest.mark.parametrize("split", [1, 2, 3])
def test_rectangular_and_forced_split(nt, split):
    X, _, _, cov, _, _ = case("se", 257, 3)
    Xt = synth(nt, d=3, seed=7, scale=4.0)[0]
    Xt[0] = X[128]
    V = vectors(17, 257)
    assert gp.IterativeGP.plan(nt, 257, 17, split)["split"] == split
    out = handle("se", 257, 3, split).apply_cross(Xt, V)
    Ks = cov.k(Xt.astype(LD), X.astype(LD))
    hold(out, V.astype(LD) @ Ks.T, product_bound(Ks, 4.5e-16, V, 257), "apply_cross")


def test_square_is_rectangular_plus_noise():
    """split 1: the two forms sum the same entries in the same order, so apply = RN(cross + sn2 V) by its one fma: it differs
    from cross + sn2 V, formed in longdouble, by that one rounding."""
    X, _, hp, _, _, _ = case("rq_ard", 257, 3)
    V = vectors(17, 257)
    g = handle("rq_ard", 257, 3, 1)
    sq, cr = g.apply(V), g.apply_cross(X, V)
    sn2 = gp.prior_scalars(hp)[1]
    ref = cr.astype(LD) + LD(sn2) * V.astype(LD)
    assert np.all(np.abs(sq.astype(LD) - ref) <= U * np.abs(ref) * (1 + 1e-3))


def test_bits_repeat_and_columns_are_independent():
    V = vectors(17, 257)
    g = handle("matern52_ard", 257, 3)
    out = g.apply(V)
    assert np.array_equal(out, g.apply(V)) and np.array_equal(out, handle("matern52_ard", 257, 3).apply(V))
    for c in (0, 5, 16):
        assert np.array_equal(out[c], g.apply(V[c])[0]), c
    Xs, info = g.solve(V, TOL, 4 * 257, 5)
    X1, info1 = g.solve(V[5], TOL, 4 * 257, 5)
    assert np.array_equal(Xs[5], X1[0]) and np.array_equal(info[5], info1[0])


def test_batches_beyond_64_columns():
    """t = 70 travels as 64 + 6 columns: every column has the bits of its own one-column call."""
    V = vectors(70, 65)
    g = handle("se", 65, 3)
    out, (Xs, info) = g.apply(V), g.solve(V, TOL, 260, 7)
    for c in (0, 63, 64, 68):
        assert np.array_equal(out[c], g.apply(V[c])[0]) and np.array_equal(Xs[c], g.solve(V[c], TOL, 260, 7)[0][0]), c
    assert np.all(info[:, 2] == 1) and np.all(out[-1] == 0)


@pytest.mark.parametrize("call,args", [
    ("apply", lambda V, Xt: (np.zeros((0, 65)),)), ("apply_cross", lambda V, Xt: (Xt[:0], V)),
    ("apply_cross", lambda V, Xt: (Xt, np.zeros((0, 65)))), ("solve", lambda V, Xt: (np.zeros((0, 65)),)),
    ("solve", lambda V, Xt: (V, 0.0)), ("solve", lambda V, Xt: (V, np.inf)), ("solve", lambda V, Xt: (V, np.nan)),
    ("solve", lambda V, Xt: (V, TOL, 0)), ("solve", lambda V, Xt: (V, TOL, 10, 0)), ("fit", lambda V, Xt: (-1.0,)),
    ("fit", lambda V, Xt: (TOL, 0)), ("fit", lambda V, Xt: (TOL, 10, 0)), ("predict", lambda V, Xt: (Xt[:0],)),
    ("predict", lambda V, Xt: (Xt, True, 0.0)), ("predict", lambda V, Xt: (Xt, True, TOL, 0)),
    ("predict", lambda V, Xt: (Xt, True, TOL, 10, 0)), ("set_split", lambda V, Xt: (-1,)), ("set_split", lambda V, Xt: (65536,))])
def test_refusals_on_a_live_handle(call, args):
    """Through the C ABI (IterativeGP's own shape checks are bypassed where they would answer first)."""
    g = handle("se", 65, 3)
    g.fit(TOL, 260, 7)
    g._block = lambda V: gp.f64(V)
    with pytest.raises(capi.CugpError) as e:
        getattr(g, call)(*args(vectors(2, 65), synth(3, d=3, seed=7, scale=4.0)[0]))
    assert e.value.code == capi.CUGP_ERR_INVALID and "cugp_iter_" + call in str(e.value)
    assert g.predict(synth(3, d=3, seed=7, scale=4.0)[0], var=False)[0].shape == (3,)       # the handle and its fit stand


def cg_longdouble(K, B, max_iter):
    """Plain CG per column in longdouble: -> all columns reach |r| <= TOL |b| within max_iter sweeps."""
    x, r = np.zeros_like(B), B.copy()
    p, rr, bb = r.copy(), (r * r).sum(0), (B * B).sum(0)
    for _ in range(max_iter):
        live = rr > TOL * TOL * bb
        if not live.any():
            return True
        q = K @ p
        a = np.where(live, rr / np.where(live, (p * q).sum(0), 1), 0)
        x, r = x + a * p, r - a * q
        rn = (r * r).sum(0)
        p, rr = np.where(live, r + rn / np.where(live, rr, 1) * p, p), np.where(live, rn, rr)
    return not (rr > TOL * TOL * bb).any()


@pytest.mark.parametrize("family", ["se", "matern52_ard", "rq_ard"])
@pytest.mark.parametrize("n", [65, 257])
@pytest.mark.parametrize("t", [1, 17])
def test_solver(family, n, t):
    _, _, _, _, K, E = case(family, n, 3)
    B = vectors(t, n, seed=1)
    assert cg_longdouble(K, B.T.astype(LD), 4 * n), "the inputs must be ones on which longdouble CG converges"
    Xs, info = handle(family, n, 3).solve(B, TOL, 4 * n, 7)
    assert np.all(info[:, 2] == 1) and np.all(info[:, 3] == 0)
    if t > 1:
        assert np.all(Xs[-1] == 0) and info[-1, 0] == 0 and info[-1, 1] == 0
    R = B.astype(LD) - Xs.astype(LD) @ K.T
    rn, bn = np.sqrt((R * R).sum(1)), np.sqrt((B.astype(LD) ** 2).sum(1))
    pb = product_bound(K, E, Xs, n)
    print("true residual / (tol |b|):", np.asarray(rn / np.maximum(bn, 1e-300) / TOL, dtype=float), "sweeps", info[:, 0])
    assert np.all(rn <= TOL * bn + np.sqrt((pb * pb).sum(1)))
    Kinv = truth.gram_lower(truth.tri_inverse(truth.cholesky(K)))
    lmin = lambda_min(K)
    D = Xs.astype(LD) - B.astype(LD) @ Kinv.T
    assert np.all(np.sqrt((D * D).sum(1)) <= rn / lmin)


def test_breakdown_is_nan_and_leaves_nothing_behind():
    X, y, hp, _, _, _ = case("rq_ard", 65, 3)
    B = vectors(17, 65, seed=1)
    g = handle("rq_ard", 65, 3)
    g.set_loghyper(hp[:3] + [800.0] + hp[4:])                         # alpha = exp(800) = inf, h2a = 0: every entry NaN
    Xs, info = g.solve(B, TOL, 260, 7)
    assert np.all(np.isnan(Xs[:-1])) and np.all(info[:-1, 3] == 1) and np.all(info[:-1, 2] == 0)
    assert np.all(Xs[-1] == 0) and info[-1, 2] == 1                   # (the zero column never multiplies)
    g.set_loghyper(hp)
    got, want = g.solve(B, TOL, 260, 7), handle("rq_ard", 65, 3).solve(B, TOL, 260, 7)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("family", ["se", "matern52_ard", "rq_ard"])
@pytest.mark.parametrize("nt", [1, 65])
def test_prediction(family, nt):
    """mean = ks' a, a the device's alpha with true residual r = y - K a:  |ks'a - ks'K^-1 y| <= |ks| |r| / lmin, plus the
    product bound at V = a.  var = prior - ks_d' w: the solve's contract (converged on the true residual, test_solver) gives
    |r_w| <= tol |ks| + |product bound at w|, so |ks' K^-1 r_w| <= |ks| |r_w| / lmin; the fixed-order dot adds gamma_{n+2}
    sum |ks||w|, the computed right-hand side ks_d = ks (1 + e) twice sum E |ks||w|, the last subtraction u (prior + |var|)."""
    n, d = 257, 3
    X, y, hp, cov, K, E = case(family, n, d)
    Xt = synth(nt, d=d, seed=7, scale=4.0)[0]
    Xt[0] = X[n // 2]
    g = handle(family, n, d)
    for stale in (lambda: None, lambda: (g.fit(TOL, 4 * n, 7), g.set_loghyper(hp))):
        stale()
        with pytest.raises(capi.CugpError) as e:
            g.predict(Xt, var=False)
        assert e.value.code == capi.CUGP_ERR_INVALID and "cugp_iter_predict" in str(e.value)
    assert g.fit(TOL, 4 * n, 7)[2] == 1
    mean, var, info = g.predict(Xt, True, TOL, 4 * n, 7)
    assert np.all(info[:, 2] == 1) and np.array_equal(mean, g.predict(Xt, var=False)[0])
    t = truth.Truth(X, y, cov)
    tmean, tvar = t.predict(Xt)
    Ks = cov.k(Xt.astype(LD), X.astype(LD))
    Ek = FAMILIES[family][2](Xt, X, cov)
    lmin = lambda_min(K)
    norm = lambda A: np.sqrt((A * A).sum(-1))
    a = g.alpha()
    bm = product_bound(Ks, Ek, a[None, :], n)[0] + norm(Ks) * norm(y.astype(LD) - K @ a.astype(LD)) / lmin
    hold(mean, tmean, bm, "mean")
    W = Ks @ t.Kinv                                                    # [nt, n]: w_c = K^-1 ks_c
    rw = TOL * norm(Ks) + norm(product_bound(K, E, W, n))
    aw = np.abs(Ks) * np.abs(W)
    bv = norm(Ks) * rw / lmin + gamma(n + 2) * aw.sum(1) + 2 * (Ek * aw).sum(1) + U * (t.sf2 + t.sn2 + np.abs(tvar))
    hold(var, tvar, bv, "var")
