"""The matrix-free exact GP's gradient on the GPU (cugp_iter_grad_forms, cugp_iter_loglik_grad)
against numpy.longdouble, with test_gpu_iter's cases, handles and eigenvalue bound.

Forms.  out_h = sum_ij W_ij dK_ij/dtheta_h, W = sum_c u_c v_c'.  Bound per component, from the truth:
    sum_ij (gamma_m |dK_ij| + A_ij) (|U|'|V|)_ij,   A_ij = E^h_ij |dK_ij| the computed factor's absolute error.
m, the longest chain of roundings one output passes through, along k_cov_grad: the weight's terms, at most 64 a block
(min(t, 64)); w times the factor,
ARD again times u_c^2 (2); the lane's 8 entries of each of ceil(n / 32) stages; wave_sum (6); the four waves (2); the partial
rows (row blocks x split - 1); a tied handle's d columns (d - 1); the blocks of 64 columns (ceil(t / 64) - 1).  The noise
component runs along k_iter_dot instead: product (1), a class's rows (ceil(min(n, 512) / 16)), the classes (15), the blocks
(ceil(n / 512) - 1), a block's columns (min(t, 64) - 1), the column blocks, sn2 on the host (2) and two products (2).  m = the
larger.
E^h in u = 2^-53, on top of test_gpu_iter's E of the Kf entry (derived there or in truth_matern / truth_ard_matern / truth_rq):
  se          dKf/dlog l = kf * (d2 / l^2): d2 d + 2, l^2 on the host 2, the division 1, the product 1           E + (d + 6) u
  matern32    truth_matern bounds kf only; dk = sf2 ((a a) e) differs from kf = sf2 ((1 + a) e) in one factor.  Along
              truth_matern's count (eps_a = (d + 11) / 2 u): e a eps_a + 2; a a 2 eps_a + 1 where 1 + a has at most eps_a + 1;
              the two products and sf2 4 as there: (7 + (a + 2) eps_a) u = E + eps_a; one u more is allowed
                                                                                                       E + ((d + 11) / 2 + 1) u
  ARD route   H: se_ard H = Kf.  matern52_ard: truth_ard_matern bounds kf only; H = sf2 ((RN(5/3) (1 + a)) e).  Along its
              count (eps_a = (d + 14) / 2 u): e a eps_a + 2; 1 + a at most eps_a + 1; the constant 1, its product 1; the
              product with e and sf2 4: (9 + (1 + a) eps_a) u, below kf's (10 + (a + 2) eps_a) u <= E: E_H = E.  RQ:
              truth_rq.k_entry_bound's own H and A bounds (A's is absolute, in Kf alpha).  u_c^2: u_c is 4 (test_gpu_iter),
              the square 2 * 4 + 1                                                                                E_H + 9 u
Estimator.  With Z = sqrt(n) I the estimate is the exact gradient; beside the forms' bounds at the device's own solutions stand
the solver's terms |du_p| <= tol |z_p| / lmin and |dalpha| <= tol |y| / lmin (every column converged on its true residual)
through |du' dK z| <= |du| |dK z|, and the two roundings of g = (F_p / t - F_a) / 2."""
import functools

import numpy as np
import pytest

import test_gpu_iter as ti
import truth
import truth_ard_matern as tam
import truth_rq as trq
from cugp_amd import gp

pytestmark = pytest.mark.gpu
LD, U, gamma = truth.LD, truth.U, truth.gamma
TOL = 1e-10


@functools.lru_cache(maxsize=None)
def derivs(family, n, d):
    """-> [(dK/dtheta_h, A_h)] in longdouble, h in the handle's order: computed once, never changed."""
    X, _, _, cov, _, E = ti.case(family, n, d)
    Xl = X.astype(LD)
    Kf = cov.k(Xl, Xl)
    out = []
    if family in ("se", "matern32"):
        S = truth.sqdist(Xl, Xl) / cov.l2
        dl, El = (Kf * S, E + (d + 6) * U) if family == "se" else (truth.matern_kernel(S, cov.sf2, 1)[1], E + ((d + 11) / 2 + 1) * U)
        out.append((dl, El * dl))
    else:
        D2 = []
        S = truth.wsqdist(Xl, Xl, cov.weights(d) if family.startswith("rq") else cov.w, lambda c, D: D2.append(D))
        if family.startswith("rq"):
            _, H, A = trq.parts(S, cov.sf2, cov.alpha)
            _, EH, EA = trq.k_entry_bound(trq.true_u(X, X, cov), float(cov.alpha), d)
        else:
            H, EH = (Kf if family == "se_ard" else tam.parts(S, cov.sf2, 2)[1]), E
        per = [(H * D, (EH + 9 * U) * H * D) for D in D2]
        out += [tuple(sum(p[k] for p in per) for k in (0, 1))] if family == "rq" else per
        if family.startswith("rq"):
            out.append((A, Kf * cov.alpha * EA))
    return out + [(2 * Kf, 2 * E * Kf), (2 * cov.sn2 * np.eye(n, dtype=LD), np.zeros((n, n), dtype=LD))]


def chain(n, t, d, split):
    p = gp.IterativeGP.plan(n, n, t, split)
    forms = min(t, 64) + 2 + 8 * -(-n // 32) + 6 + 2 + p["row_blocks"] * p["split"] - 1 + d - 1 + -(-t // 64) - 1
    dot = 1 + -(-min(n, 512) // 16) + 15 + -(-n // 512) - 1 + min(t, 64) - 1 + -(-t // 64) - 1 + 4
    return max(forms, dot)


def forms_truth(family, n, d, Uv, Vv, split=0):
    """-> (truth [nh], bound [nh]) of grad_forms(Uv, Vv)"""
    W, P = Uv.astype(LD).T @ Vv.astype(LD), np.abs(Uv).astype(LD).T @ np.abs(Vv).astype(LD)
    g = gamma(chain(n, len(Uv), d, split))
    return (np.array([(W * dK).sum() for dK, _ in derivs(family, n, d)]),
            np.array([((g * np.abs(dK) + A) * P).sum() for dK, A in derivs(family, n, d)]))


FORMS = ([("se", n, t, 3, 0) for n in ti.NS for t in (1, 15, 16, 17, 64, 65)] + [("se", 65, 17, 1, 0), ("se", 129, 16, 17, 0)]
         + [(f, n, t, d, 0) for f in ("se_ard", "matern32", "matern52_ard", "rq", "rq_ard") for n, t, d in ((65, 17, 17), (257, 33, 1))]
         + [("se_ard", 257, 17, 3, s) for s in (1, 2, 3)])


@pytest.mark.parametrize("family,n,t,d,split", FORMS)
def test_forms_against_truth(family, n, t, d, split):
    Uv, Vv = ti.vectors(t, n, seed=1), ti.vectors(t, n, seed=2)
    assert split == 0 or gp.IterativeGP.plan(n, n, t, split)["split"] == split
    want, bound = forms_truth(family, n, d, Uv, Vv, split)
    ti.hold(ti.handle(family, n, d, split).grad_forms(Uv, Vv), want, bound, "grad_forms")


def test_bits():
    Uv, Vv = ti.vectors(16, 257, seed=1)[:15], ti.vectors(16, 257, seed=2)[:15]          # (vectors() zeroes its last row)
    g = ti.handle("matern52_ard", 257, 3)
    out = g.grad_forms(Uv, Vv)
    assert np.array_equal(out, g.grad_forms(Uv, Vv)) and np.array_equal(out, ti.handle("matern52_ard", 257, 3).grad_forms(Uv, Vv))
    for pad in (1, 2):                                      # t = 15, then 16 (tp = 16) and 17 (tp = 64): zero columns change nothing
        z = np.zeros((pad, 257))
        assert np.array_equal(out, g.grad_forms(np.vstack([Uv, z]), np.vstack([Vv, z]))), pad
    tied, ard = ti.handle("rq", 257, 3), ti.handle("rq_ard", 257, 3)
    ard.set_loghyper([ti.case("rq", 257, 3)[2][0]] * 3 + ti.case("rq", 257, 3)[2][1:])
    a, b = tied.grad_forms(Uv, Vv), ard.grad_forms(Uv, Vv)
    assert a[0] == (b[0] + b[1]) + b[2] and np.array_equal(a[1:], b[3:])


@pytest.mark.parametrize("family,rank", [("se", 0), ("rq_ard", 0), ("se", 16)])
def test_estimator_is_exact_for_a_complete_probe_set(family, rank):
    n, d = 65, 3
    X, y, _, cov, K, _ = ti.case(family, n, d)
    lmin = ti.lambda_min(K)
    assert lmin > 0
    Z = np.sqrt(float(n)) * np.eye(n)
    g = ti.handle(family, n, d)
    g.set_precond(rank)
    got, info = g.loglik_grad(Z, tol=TOL, max_iter=4 * n, check_every=7)
    Us, sinfo = g.solve(Z, TOL, 4 * n, 7)                   # the probes' solutions as loglik_grad formed them
    a = g.alpha()
    assert np.all(info["solves"][:, 2] == 1) and np.array_equal(info["solves"], sinfo) and info["quad"] == pytest.approx(y @ a)
    t = truth.Truth(X, y, cov)
    norm = lambda v: np.sqrt((v * v).sum())
    Fp, Bp = forms_truth(family, n, d, Us, Z)
    Fa, Ba = forms_truth(family, n, d, a[None, :], a[None, :])
    want, solver = [], []
    for dK, _ in derivs(family, n, d):
        want.append(((t.Kinv - np.outer(t.alpha, t.alpha)) * dK).sum() / 2)
        du = sum(TOL * norm(Z[p].astype(LD)) / lmin * norm(dK @ Z[p].astype(LD)) for p in range(n))
        solver.append(du / n + TOL * norm(y.astype(LD)) / lmin * (norm(dK @ a.astype(LD)) + norm(dK @ t.alpha)))
    bound = (Bp / n + Ba + np.array(solver)) / 2 * (1 + 4 * U) + 2 * U * (np.abs(Fp) / n + np.abs(Fa))
    ti.hold(got, np.array(want), bound, "loglik_grad")


def test_contract():
    n = 65
    X, y, hp = ti.case("se", n, 3)[:3]
    Z = gp.rademacher(np.random.default_rng(4), 5, n)
    g, ref = ti.handle("se", n, 3), ti.handle("se", n, 3)
    V = ti.vectors(3, n)
    before = g.apply(V)
    grad, info = g.loglik_grad(Z, tol=TOL, max_iter=4 * n, check_every=7)            # a fresh handle: the fit is fit's
    ref.fit(TOL, 4 * n, 7)
    assert np.array_equal(g.alpha(), ref.alpha()) and np.all(info["solves"][:, 2] == 1) and np.all(np.isfinite(grad))
    assert np.array_equal(grad, g.loglik_grad(5, np.random.default_rng(4), TOL, 4 * n, 7)[0])
    assert np.array_equal(before, g.apply(V)) and np.array_equal(g.fit(TOL, 4 * n, 7), ref.fit(TOL, 4 * n, 7))
    assert np.array_equal(g.alpha(), ref.alpha())
    short = ti.handle("se", n, 3).loglik_grad(Z, tol=TOL, max_iter=1, check_every=7)
    assert np.all(short[1]["solves"][:, 2] == 0) and np.all(short[1]["solves"][:, 3] == 0) and np.all(np.isfinite(short[0]))
    Z[2, 7] = np.nan
    bad, binfo = g.loglik_grad(Z, tol=TOL, max_iter=4 * n, check_every=7)            # CUGP_OK: no exception
    assert np.all(np.isnan(bad)) and binfo["solves"][2, 3] == 1 and np.all(binfo["solves"][[0, 1, 3, 4], 2] == 1)
