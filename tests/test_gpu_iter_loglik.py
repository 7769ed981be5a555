"""The matrix-free GP's log marginal likelihood by Lanczos quadrature on the GPU (cugp_iter_loglik, cugp_iter_precond_sample;
DESIGN.md section 40) against numpy.longdouble, with test_gpu_iter's cases and handles.

Bounds follow docs/ACCURACY.md's pattern: error <= F x yardstick, the yardstick u = 2^-53 times the sum of the magnitudes the
quantity is added up from, F = 4 x the largest ratio an independent fp64 numpy stand-in of the same recurrences and quadrature
(tools/slq_standin.py, CPU) shows against the same truth on these very cases -- never a figure the GPU gave.
  ll      yardstick u (|y'alpha| / 2 + sum_i |log lambda_i(K)| / 2 + n 1.83787 / 2)      stand-in's largest ratio 86.5 -> F_SLQ
  quad_p  yardstick u sum_i |log mu_i| (v_i'z_p)^2, (mu, v) of K v = mu M v              stand-in's largest ratio 331 -> F_QUAD
The largest GPU ratios are recorded in docs/ACCURACY.md.
precond_sample is held to a rounding count: r terms through the MFMA's accumulator, sn = sqrt(sn2) from a host exp (3), its
product (1), the last sum (1): gamma_(r + 5) (|L| |G1| + sn |G2|)."""
import numpy as np
import pytest

import test_gpu_iter as ti
import truth
from cugp_amd import gp

pytestmark = pytest.mark.gpu
LD, U, gamma = truth.LD, truth.U, truth.gamma
TOL, D = 1e-12, 3
F_SLQ, F_QUAD = 4 * 86.5, 4 * 331
KERNELS = ("se", "matern32", "rq_ard")
CASES = [(n, r) for n in (1, 5, 65, 200) for r in (0, 5, 8) if r < n]


def complete_probes(n, r):
    """(G2 [t, n], G1 [t, r] or None): the t = n + r columns of sqrt(t) I_t, so that (1/t) sum z z' = M exactly"""
    G = np.sqrt(float(n + r)) * np.eye(n + r)
    return np.ascontiguousarray(G[:, r:]), (np.ascontiguousarray(G[:, :r]) if r else None)


def ll_yardstick(family, n):
    X, y, _, cov, K, _ = ti.case(family, n, D)
    t = truth.Truth(X, y, cov)
    lam = np.linalg.eigvalsh(K.astype(np.float64))
    return t.ll, U * (abs(float(y @ t.alpha)) + np.abs(np.log(lam)).sum() + n * truth.LL_CONST) / 2


def quad_truth(family, n, L, Z):
    """-> (z~' log(M^-1/2 K M^-1/2) z~ per probe, its yardstick) from the generalised eigenproblem K v = mu M v, V'MV = I"""
    import scipy.linalg as sl
    cov, K = ti.case(family, n, D)[3:5]
    M = L @ L.T + float(cov.sn2) * np.eye(n) if L.shape[1] else np.eye(n)
    mu, V = sl.eigh(K.astype(np.float64), M)
    W = (Z @ V) ** 2
    return W @ np.log(mu), U * (W @ np.abs(np.log(mu)))


def ready(family, n, r):
    g = ti.handle(family, n, D)
    g.set_precond(r)
    assert g.precond_info()["achieved"] == r
    return g


@pytest.mark.parametrize("n,r", CASES)
@pytest.mark.parametrize("family", KERNELS)
def test_value_against_truth(family, n, r):
    g = ready(family, n, r)
    G2, G1 = complete_probes(n, r)
    out = g.loglik(G2, G1, tol=TOL, max_iter=4 * n + 8, check_every=7)
    want, yard = ll_yardstick(family, n)
    L = g.precond_factor()[0].astype(LD)
    sn2 = ti.case(family, n, D)[3].sn2
    ldm = np.linalg.slogdet((L @ L.T + sn2 * np.eye(n, dtype=LD)).astype(np.float64))[1] if r else 0.0
    print("ll: error / yardstick %.3g (F_SLQ %.3g)" % (abs(LD(out["ll"]) - want) / yard, F_SLQ))
    assert np.all(out["solves"][:, 2] == 1) and out["logdet_precond"] == pytest.approx(ldm, rel=1e-9, abs=1e-9)
    assert abs(LD(out["ll"]) - want) <= F_SLQ * yard


@pytest.mark.parametrize("r", (0, 8))
@pytest.mark.parametrize("family", KERNELS)
def test_quadratures_per_probe(family, r):
    n = 200
    g = ready(family, n, r)
    rng = np.random.default_rng(5)
    G2, G1 = gp.rademacher(rng, 9, n), (gp.rademacher(rng, 9, r) if r else None)
    out = g.loglik(G2, G1, grad=False, tol=TOL, max_iter=4 * n, check_every=7)
    L = g.precond_factor()[0]
    Z = g.precond_sample(G1, G2) if r else G2
    want, yard = quad_truth(family, n, L, Z)
    print("quad: largest error / yardstick %.3g (F_QUAD %.3g)" % (np.max(np.abs(out["quad"] - want) / yard), F_QUAD))
    assert out["g"] is None and np.all(np.abs(out["quad"] - want) <= F_QUAD * yard)


@pytest.mark.parametrize("t", (1, 17, 64))
@pytest.mark.parametrize("n,r", [(n, r) for n in (5, 65, 200) for r in (1, 5, 8) if r < n])
def test_precond_sample(n, r, t):
    g = ready("se", n, r)
    rng = np.random.default_rng(n + r + t)
    G1, G2 = rng.standard_normal((t, r)), rng.standard_normal((t, n))
    L, sn = g.precond_factor()[0].astype(LD), np.sqrt(ti.case("se", n, D)[3].sn2)
    ti.hold(g.precond_sample(G1, G2), G1.astype(LD) @ L.T + sn * G2.astype(LD),
            gamma(r + 5) * (np.abs(G1).astype(LD) @ np.abs(L).T + sn * np.abs(G2).astype(LD)), "precond_sample")


def test_bits():
    n = 65
    Z = gp.rademacher(np.random.default_rng(4), 5, n)
    g, ref = ti.handle("rq_ard", n, D), ti.handle("rq_ard", n, D)
    B = ti.vectors(3, n)
    args = dict(tol=1e-10, max_iter=4 * n, check_every=7)
    before = (ref.solve(B, 1e-10, 4 * n, 7)[0], ref.fit(1e-10, 4 * n, 7), ref.alpha())
    a, b = g.loglik(Z, **args), g.loglik(Z, **args)
    assert np.array_equal(a["g"], ref.loglik_grad(Z, **args)[0]) and a["y_alpha"] == ref.loglik_grad(Z, **args)[1]["quad"]
    assert all(np.array_equal(a[k], b[k]) for k in a) and np.isfinite(a["ll"])
    after = (g.solve(B, 1e-10, 4 * n, 7)[0], g.fit(1e-10, 4 * n, 7), g.alpha())
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    g.set_precond(8)                                         # preconditioned: the same bits twice, the handle's too
    G1 = gp.rademacher(np.random.default_rng(6), 5, 8)
    a, b = g.loglik(Z, G1, **args), g.loglik(Z, G1, **args)
    assert all(np.array_equal(a[k], b[k]) for k in a) and np.isfinite(a["ll"]) and np.all(np.isfinite(a["g"]))
    with pytest.raises(ValueError):
        g.loglik(Z, **args)                                  # an array of probes without probes_factor


def test_edges():
    n = 65
    X, y, hp = ti.case("se", n, D)[:3]
    Z = gp.rademacher(np.random.default_rng(4), 5, n)
    short = ti.handle("se", n, D).loglik(Z, tol=TOL, max_iter=3, check_every=7)
    assert np.all(short["solves"][:, 2] == 0) and np.all(short["solves"][:, 0] == 3) and np.isfinite(short["ll"])
    Xn = X.copy()
    Xn[7] = np.nan
    bad = gp.IterativeGP(n, D)
    bad.set_data(Xn, y)
    bad.set_loghyper(hp)
    assert np.isnan(bad.loglik(Z, tol=TOL, max_iter=4 * n, check_every=7)["ll"])          # CUGP_OK: no exception
    mixed = ti.handle("se", n, D)
    mixed.set_precision("mixed")
    with pytest.raises(Exception, match="cugp_iter_loglik"):
        mixed.loglik(Z)
