"""The matrix-free exact GP's test-input gradients on the GPU (cugp_iter_input_grad, cugp_iter_predict_grad; DESIGN.md
section 37) against numpy.longdouble, with test_gpu_iter's cases, handles, eigenvalue bound and `hold`.

Forms.  out_ia = sum_j W_j dk_ij/dx*_ia = -s_a sum_j G_ij W_j (x*_ia - x_ja).  Bound per output, from the truth:
    s_a sum_j (gamma_m + E^G_ij) |G_ij| |W_j| |x*_ia - x_ja|
m, the chain of roundings one output passes through along k_cov_xgrad: the difference (1); G w (1); times the difference (1);
the lane's 8 entries of each of ceil(n / 32) stages; the fk groups (2); the ranges (split - 1); in the finish s_a = w_a^2 from
w_a = exp(-theta_a) of the host (5; 1 / l^2: 3), its product with the sum (1), the sign exact.  E^G, the entry factor's error,
is what test_gpu_iter_grad's docstring tabulates: E of the Kf entry for SE and SE-ARD (G = Kf), E_H = E for matern52_ard,
truth_rq.k_entry_bound's H bound for RQ; Matern 3/2's H = sf2 (3 e), isotropic or ARD, takes two roundings fewer than kf =
sf2 ((1 + a) e): E; isotropic Matern 5/2's H = sf2 ((RN(5/3) (1 + a)) e) counts (9 + (1 + a) eps_a) u along truth_matern's
lines, below kf's (10 + (a + 2) eps_a) u <= E, as for matern52_ard: E.  The two families test_gpu_iter.FAMILIES lacks (matern52,
matern32_ard) get cases of their own on the same data (OWN).
The bound is in |x* - x|, so the coordinate form x*_a sum(G w) - sum(G w x_a) cannot pass it on shifted data: at n = 257,
d = 3, nt = 17, X + 1e6 and Xt + 1e6, on the CPU, the fp64 numpy difference-first sums (truth_predict_grad.sums) reach 0.0074
of the bound (t = 1; t = nt: 0.0065) and its coordinate=True form 7.1e+03 times the bound (both).
The chain takes the largest split over the launches of a call (t == nt: 64 points a launch, each planned by itself).
predict_grad.  dmean and dvar against the truth's alpha = K^-1 y and v = K^-1 k*: the forms' bound at the device's own alpha
(dvar: twice the forms' bound at the truth's |v| -- the device's v does not cross the ABI), plus the solver's terms
|dk row|_2 tol |y| / lmin and 2 |dk row|_2 tol |k*| / lmin, every column converged on its true residual."""
import functools

import numpy as np
import pytest

import test_gpu_iter as ti
import truth
import truth_ard_matern as tam
import truth_matern as tm
import truth_rq as trq
from conftest import synth
from cugp_amd import capi, gp

pytestmark = pytest.mark.gpu
LD, U, gamma = truth.LD, truth.U, truth.gamma
TOL = 1e-10


# the two rows of CUGP_COV_KERNEL that test_gpu_iter.FAMILIES does not hold, in its format: (d -> theta, theta -> descriptor, E)
OWN = {
    "matern52": (lambda d: [0.9, 0.2, -1.0], lambda hp: truth.Matern(hp, 2),
                 lambda A, B, c: tm.k_entry_bound(tm.a_of(A, B, c.hp, 2), A.shape[1], 2)),
    "matern32_ard": (lambda d: ti._ls(d) + [0.2, -1.0], lambda hp: tam.ARDMatern(hp, 1),
                     lambda A, B, c: tam.k_entry_bound(tam.a_of(A, B, c), A.shape[1], 1)),
}


@functools.lru_cache(maxsize=None)
def case(family, n, d):
    """-> (X, y, theta, descriptor, E's function): test_gpu_iter's case, or the same data for a family of OWN"""
    if family in ti.FAMILIES:
        return ti.case(family, n, d)[:4] + (ti.FAMILIES[family][2],)
    truth.require_extended()
    X, y = synth(n, d=d, seed=3 * n + d, scale=4.0 if d <= 3 else 1.8)
    hp = OWN[family][0](d)
    return X, y, hp, OWN[family][1](hp), OWN[family][2]


@functools.lru_cache(maxsize=None)
def cross(family, n, d, nt, shift=0.0):
    """-> (X, Xt, F [nt, n, d] = G (x* - x) s, the truth's dk/dx* negated; B = E^G |F|): computed once, never changed."""
    cov, efn = case(family, n, d)[3:]
    X, Xt = case(family, n, d)[0] + shift, synth(nt, d=d, seed=7, scale=4.0 if d <= 3 else 1.8)[0] + shift
    Xt[0] = X[n // 2]
    Xl, Tl = X.astype(LD), Xt.astype(LD)
    if family in ("se", "matern32", "matern52"):
        S, s = truth.sqdist(Tl, Xl) / cov.l2, np.full(d, 1 / cov.l2)
        G = cov.k(Tl, Xl) if family == "se" else tam.parts(S, cov.sf2, cov.kind)[1]
    else:
        w = cov.weights(d) if family.startswith("rq") else cov.w
        S, s = truth.wsqdist(Tl, Xl, w), w * w
        G = trq.parts(S, cov.sf2, cov.alpha)[1] if family.startswith("rq") else (
            cov.k(Tl, Xl) if family == "se_ard" else tam.parts(S, cov.sf2, cov.kind)[1])
    E = trq.k_entry_bound(trq.true_u(Xt, X, cov), float(cov.alpha), d)[1] if family.startswith("rq") else efn(Xt, X, cov)
    F = G[:, :, None] * (Tl[:, None, :] - Xl[None, :, :]) * s
    return X, Xt, F, np.abs(F) * np.asarray(E, dtype=LD)[..., None]


def chain(n, split):
    return 3 + 8 * -(-n // 32) + 2 + split - 1 + 6


def forms(F, B, W, m):
    """-> (truth, bound) [nt, d] for weights W [1 | nt, n]"""
    Wl = W.astype(LD)[:, :, None]
    return -(F * Wl).sum(1), ((gamma(m) * np.abs(F) + B) * np.abs(Wl)).sum(1)


def handle(family, n, d, X, split=0):
    _, y, hp = case(family, n, d)[:3]
    g = gp.IterativeGP(n, d, kernel="se" if family == "se_ard" else family, ard=family == "se_ard")
    g.set_data(X, y)
    g.set_loghyper(hp)
    g.set_split(split)
    return g


FORMS = ([("se", n, 17, 3, 0) for n in (1, 31, 32, 33, 63, 64, 65, 257)] + [("se", 65, nt, 3, 0) for nt in (1, 15, 16, 64, 65, 70)]
         + [("se", 65, 17, d, 0) for d in (1, 17, 33)]
         + [(f, n, nt, d, 0) for f in ("se_ard", "matern32", "matern52", "matern32_ard", "matern52_ard", "rq", "rq_ard")
            for n, nt, d in ((65, 17, 17), (257, 33, 1))]
         + [("se", 257, 17, 3, s) for s in (1, 2, 3)])


@pytest.mark.parametrize("per_point", [False, True])
@pytest.mark.parametrize("family,n,nt,d,split", FORMS)
def test_forms_against_truth(family, n, nt, d, split, per_point):
    X, Xt, F, B = cross(family, n, d, nt)
    W = ti.vectors(nt + 1, n, seed=3)[:nt if per_point else 1]
    # t == nt travels 64 points a launch, each batch with a plan of its own: the longest chain over the batches
    batches = [min(64, nt - c0) for c0 in range(0, nt, 64)] if per_point else [nt]
    splits = [gp.IterativeGP.plan(b, n, 1, split)["split"] for b in batches]
    assert split == 0 or splits == [split] * len(batches)
    want, bound = forms(F, B, W, chain(n, max(splits)))
    ti.hold(handle(family, n, d, X, split).input_grad(Xt, W), want, bound, "input_grad")


@pytest.mark.parametrize("per_point", [False, True])
def test_shifted_data_keeps_the_bound(per_point):
    """|x| = 1e6 >> |x - x'|: the case the coordinate form fails (the docstring's two CPU ratios)."""
    X, Xt, F, B = cross("se", 257, 3, 17, 1e6)
    W = ti.vectors(18, 257, seed=3)[:17 if per_point else 1]
    want, bound = forms(F, B, W, chain(257, 1))
    ti.hold(handle("se", 257, 3, X).input_grad(Xt, W), want, bound, "input_grad, shifted")


def test_bits():
    X, Xt, _, _ = cross("matern52_ard", 257, 3, 70)
    W = ti.vectors(71, 257, seed=3)[:70]
    g = handle("matern52_ard", 257, 3, X)
    one, per = g.input_grad(Xt, W[:1]), g.input_grad(Xt, W)
    assert np.array_equal(one, g.input_grad(Xt, W[:1])) and np.array_equal(per, handle("matern52_ard", 257, 3, X).input_grad(Xt, W))
    # Row i of an nt = 70 call against its own nt = 1 call.  At nt = 1, t == 1 == nt: the single call takes the one-vector
    # (mean) path, so per[i] is checked across the two paths -- more than asked.  It holds while the automatic split is the
    # same for 70, 64, 6 and 1 test rows, which it is at n = 257 (9 stages: one range, whatever the row blocks)
    assert {gp.IterativeGP.plan(k, 257)["split"] for k in (70, 64, 6, 1)} == {1}
    for i in (0, 15, 16, 63, 64, 69):
        assert np.array_equal(one[i], g.input_grad(Xt[i], W[:1])[0]) and np.array_equal(per[i], g.input_grad(Xt[i], W[i])[0]), i


@functools.lru_cache(maxsize=None)
def posterior(family):
    """-> (K^-1 in longdouble: numpy's fp64 inverse and one Newton step, lambda_min's bound) of the n = 257, d = 3 case"""
    K = ti.case(family, 257, 3)[4]
    Kinv = np.linalg.inv(K.astype(np.float64)).astype(LD)
    return Kinv @ (2 * np.eye(257, dtype=LD) - K @ Kinv), ti.lambda_min(K)


@pytest.mark.parametrize("family,nt,rank,mode", [("se", 17, 0, "fp64"), ("se", 70, 0, "fp64"), ("rq_ard", 17, 0, "fp64"),
                                                 ("rq_ard", 70, 0, "fp64"), ("se", 17, 16, "fp64"), ("se", 17, 0, "mixed")])
def test_predict_grad(family, nt, rank, mode):
    n, d = 257, 3
    _, y, hp, cov = ti.case(family, n, d)[:4]
    X, Xt, F, B = cross(family, n, d, nt)
    g = ti.handle(family, n, d)
    g.set_precond(rank), g.set_precision(mode)
    assert g.fit(TOL, 4 * n, 7)[2] == 1
    m, v, dm, dv, info = g.predict_grad(Xt, tol=TOL, max_iter=4 * n, check_every=7)
    pm, pv, pinfo = g.predict(Xt, tol=TOL, max_iter=4 * n, check_every=7)
    assert np.array_equal(m, pm) and np.array_equal(v, pv) and np.array_equal(info, pinfo) and np.all(info[:, 2] == 1)
    lat = g.predict_grad(Xt, with_noise=False, tol=TOL, max_iter=4 * n, check_every=7)
    assert np.array_equal(lat[1], v - gp.prior_scalars(hp)[1]) and np.array_equal(lat[2], dm) and np.array_equal(lat[3], dv)
    Kinv, lmin, norm = posterior(family) + (lambda a, ax: np.sqrt((a * a).sum(ax)),)
    assert lmin > 0
    Ks = cov.k(Xt.astype(LD), X.astype(LD))
    alpha, V = Kinv @ y.astype(LD), Ks @ Kinv
    da, dvn = TOL * norm(y.astype(LD), 0) / lmin, TOL * norm(Ks, 1) / lmin
    rows, c = norm(F, 1), chain(n, 1)
    wm, bm = forms(F, B, alpha[None, :], c)[0], forms(F, B, g.alpha()[None, :], c)[1]
    wv, bv = forms(F, B, V, c)
    ti.hold(dm, wm, bm + rows * da, "dmean")
    ti.hold(dv, -2 * wv, 2 * bv + 2 * rows * dvn[:, None], "dvar")
    before = g.solve_stats()
    m2, v2, dm2, dv2, info2 = g.predict_grad(Xt, want_var=False, want_var_grad=False, tol=-1.0)     # no solve: tol is not read
    assert v2 is None and dv2 is None and info2 is None and np.array_equal(m2, m) and g.solve_stats() == before
    ti.hold(dm2, wm, bm + rows * da, "dmean, no solve")


@pytest.mark.parametrize("fit,call,args", [
    (True, "predict_grad", lambda p, dm: (p, 3, 1, None, None, None, None, TOL, 10, 5, None)),
    (True, "input_grad", lambda p, dm: (p, 3, p, 2, dm)), (True, "input_grad", lambda p, dm: (p, 0, p, 1, dm)),
    (True, "predict_grad", lambda p, dm: (p, 0, 1, None, None, dm, None, TOL, 10, 5, None)),
    (False, "predict_grad", lambda p, dm: (p, 3, 1, None, None, dm, None, TOL, 10, 5, None)),
    (True, "predict_grad", lambda p, dm: (p, 3, 1, None, None, dm, dm, 0.0, 10, 5, None))])
def test_refusals_on_a_live_handle(fit, call, args):
    g = ti.handle("se", 65, 3)
    if fit:
        g.fit(TOL, 260, 7)
    buf, out = np.zeros(3 * 65), np.zeros(9)
    rc = getattr(capi.lib(), "cugp_iter_" + call)(g._h, *args(capi.ptr(buf), capi.ptr(out)))
    assert rc == capi.CUGP_ERR_INVALID and ("cugp_iter_" + call).encode() in capi.lib().cugp_last_error()
    assert g.input_grad(buf[:9].reshape(3, 3), buf[:65]).shape == (3, 3)                 # the handle stands
