"""GPU tests of the ARD x Matern kernels (one length scale per input dimension with nu = 3/2 | 5/2; cugp_create_ard_kernel,
kernel="matern32_ard" | "matern52_ard").

Accuracy is held to fp64 rounding against the extended-precision truth of tests/truth_ard_matern.py (truth.Truth with the
ARDMatern descriptor) through the harness of tests/accuracy.py:

    err_gpu(q) <= F_ARD * max(noise(q), floor(q))

F_ARD = 32 as it stands; the stand-in ratios of this family (tests/test_truth_ard_matern_cpu.py, docs/ACCURACY.md) ask for
no more.  Every figure is printed before it is asserted (run with -s).  One process, one device (test 14 starts one fresh
child process); nothing outside the tree is read.
"""
import ctypes as C
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import accuracy
import truth
import truth_append as ta
import truth_ard_matern as tam
import truth_predict_grad as tpg
import truth_targets as tt
from accuracy import Report
from conftest import ROOT, synth
from cugp_amd import capi

pytestmark = pytest.mark.gpu
extended = pytest.mark.skipif(not truth.EXTENDED, reason="numpy.longdouble is not an extended-precision type here")

LD = truth.LD
M32, M52 = truth.MATERN32, truth.MATERN52
KINDS = [pytest.param(k, id=tam.KIND_NAMES[k]) for k in tam.KINDS]
TUNE_GRAPHS = 5                                                  # kernels.h TUNE_*
INV = capi.CUGP_ERR_INVALID


@pytest.fixture(scope="module")
def gp_mod():
    import cugp_amd.gp as gp
    return gp


def handle(gp_mod, X, y, hp, kind, overlap=None, cap=0, tuning=None):
    g = gp_mod.Covsum(X.shape[0], X.shape[1], npad_min=cap, kernel=tam.FAMILY[kind])
    if overlap is not None:
        g.set_overlap(overlap)
    for k, v in (tuning or {}).items():
        g.set_tuning(k, v)
    g.set_data(X, y)
    g.set_loghyperparam(hp)
    return g


def same_bits(a, b):
    """Bit-equal; a NaN on both sides counts as equal (its payload is not part of any contract)."""
    a, b = [np.concatenate([np.atleast_1d(np.asarray(x, dtype=np.float64)).ravel() for x in v]) for v in (a, b)]
    return a.shape == b.shape and bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


# ------------------------------------------------------------------ 1. accuracy
SMALL = ("n65_d2", "n257_d3", "n257_d3_shift", "n300_d17", "n384_cond1e6", "n515_dense", "n515_d33")
ACCURACY_CASES = [(n, k) for n in SMALL for k in tam.KINDS] + [("n1025_dense", M52), ("n1300_d6", M52)]


@extended
@pytest.mark.parametrize("name, kind", ACCURACY_CASES, ids=["%s-%s" % (n, tam.KIND_NAMES[k]) for n, k in ACCURACY_CASES])
def test_accuracy_live(gp_mod, oracle, name, kind):
    """loglik_grad, the LL-only path, prediction at 64 points, alpha and 64 rows of K^-1 (F_SOLVE); n1025_dense also with
    the inverse streams off.  The two large cases exercise the host's sequencing, not the kernel function: nu = 5/2 only."""
    c = tam.live(oracle, name, kind)
    X, y, cov = c["X"], c["y"], c["cov"]

    def fresh(g):
        assert g.ard and g.get_param_dim() == X.shape[1] + 2 and g.kernel == tam.KIND_NAMES[kind]
    accuracy.hold_live_case(Report("%s/%s" % (name, tam.FAMILY[kind]), cov), c,
                            lambda overlap=None: handle(gp_mod, X, y, cov.hp, kind, overlap),
                            overlaps=(False, True) if name == "n1025_dense" else (True,), fresh=fresh)


# ------------------------------------------------------------------ 2. K and k_test
@extended
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["n65_d2", "n300_d17", "n515_d33"])
def test_K_and_k_test_entries(gp_mod, name, kind):
    """cugp_compute_K_train and cugp_compute_k_test entry by entry against the truth, inside the derived K-entry bound
    (truth_ard_matern.k_entry_bound; relative to the true entry); K exactly symmetric, its diagonal bit-equal to
    sf2 + sn2 as fp64 forms it."""
    X, y, Xt, cov = tam.inputs(name, kind)
    n = X.shape[0]
    g = handle(gp_mod, X, y, cov.hp, kind)
    K = g.compute_K_train()
    Ks = g.compute_k_test(Xt)
    g.close()
    assert np.array_equal(K, K.T)
    assert np.all(np.diag(K) == math.exp(cov.hp[-2] * 2) + math.exp(cov.hp[-1] * 2))
    Kf = K.copy()
    Kf[np.arange(n), np.arange(n)] = math.exp(cov.hp[-2] * 2)         # (the bound is on Kf: the true diagonal is sf2)
    worst = dict(K=tam.entry_excess(Kf, X, X, cov), k_test=tam.entry_excess(Ks, Xt, X, cov))
    print("ACC %s/%s largest |entry - truth| / bound: K %.3f  k_test %.3f" % (name, tam.FAMILY[kind], worst["K"], worst["k_test"]))
    assert worst["K"] <= 1.0 and worst["k_test"] <= 1.0, worst


# ------------------------------------------------------------------ 3. equal length scales meet the isotropic Matern handle
@extended
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["n257_d3", "n515_dense"])
def test_equal_length_scales_meet_the_isotropic_matern_handle(gp_mod, oracle, name, kind):
    """Both handles are within their bounds of the same truth, so they differ by at most (F_MATERN + F_ARD) yardsticks;
    sum_c g_c against the isotropic g0 (sum_c H u_c^2 = dk/dtheta_0)."""
    c = accuracy.live(oracle, tam.KIND_NAMES[kind], name)
    X, y, Xt, cov, hp = c["X"], c["y"], c["Xt"], c["cov"], c["cov"].hp
    d = X.shape[1]
    gi = gp_mod.Covsum(*X.shape, kernel=tam.KIND_NAMES[kind])
    gi.set_loghyperparam(hp)
    lli, gri = gi.loglik_grad(X, y)
    mi, vi = gi.compute_test_means_and_variances(X, y, Xt)
    gi.close()
    ga = handle(gp_mod, X, y, [hp[0]] * d + [hp[1], hp[2]], kind)
    lla, gra = ga.loglik_grad()
    ma, va = ga.compute_test_means_and_variances(X, y, Xt)
    ga.close()
    e = truth.errors(cov, lla, [gra[:d].sum(), gra[d], gra[d + 1]], ma, va, LD(lli), gri.astype(LD), mi.astype(LD), vi.astype(LD))
    rep = Report("%s/%s_iso" % (name, tam.FAMILY[kind]), cov)
    rep.add_all("", e, c["noise"], c["floor"], truth.F_MATERN + truth.F_ARD)
    rep.check()


# ------------------------------------------------------------------ 4. a dropped dimension drops out exactly
@pytest.mark.parametrize("kind", KINDS)
def test_dropped_dimension_is_exact(gp_mod, kind):
    """theta_2 = 800: w_2 = exp(-800) = 0.0, and adding 0.0 * 0.0 in index order changes no bit -- K, LL, the prediction
    and the other components equal those of a handle on the data without column 2 bit for bit, and g_2 == 0.0.  Every
    theta_c = 800: Kf == sf2 exactly.  theta_2 = -800 (w_2 overflows): NaN results with CUGP_OK, and the handle goes on
    working."""
    X, y = synth(200, d=4, seed=11, scale=3.0)
    Xt = synth(9, d=4, seed=7, scale=3.0)[0]
    keep = [0, 1, 3]
    hp = np.array([0.5, 0.7, 800.0, 0.9, 0.3, -1.0])
    g4 = handle(gp_mod, X, y, hp, kind)
    g3 = handle(gp_mod, np.ascontiguousarray(X[:, keep]), y, hp[[0, 1, 3, 4, 5]], kind)
    assert np.array_equal(g4.compute_K_train(), g3.compute_K_train())
    ll4, gr4 = g4.loglik_grad()
    ll3, gr3 = g3.loglik_grad()
    assert ll4 == ll3 and np.array_equal(gr4[[0, 1, 3, 4, 5]], gr3), (ll4, ll3, gr4, gr3)
    assert gr4[2] == 0.0
    p4 = g4.compute_test_means_and_variances(X, y, Xt)
    p3 = g3.compute_test_means_and_variances(None, None, np.ascontiguousarray(Xt[:, keep]))
    assert same_bits(p4, p3)
    g3.close()
    g4.set_loghyperparam([800.0] * 4 + [0.3, -1.0])
    K = g4.compute_K_train()
    assert np.all(K[~np.eye(200, dtype=bool)] == math.exp(0.3 * 2))
    ll, gr = g4.loglik_grad()
    assert np.all(gr[:4] == 0.0)
    g4.set_loghyperparam([0.5, 0.7, -800.0, 0.9, 0.3, -1.0])
    ll, gr = g4.loglik_grad()                                     # raises on any return code but CUGP_OK
    assert np.isnan(ll) and np.isnan(g4.compute_loglikelihood())
    g4.set_loghyperparam(hp)
    again = g4.loglik_grad()
    assert again[0] == ll4 and np.array_equal(again[1], gr4)
    g4.close()


# ------------------------------------------------------------------ 5. d across the feature-chunk boundary
CHUNK_TOL = 1e-11


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("d", [1, 15, 16, 17, 32, 33])
def test_feature_chunks_against_the_standin(gp_mod, d, kind):
    """A wiring test (the accuracy cases hold the rounding): LL and every gradient component against the CPU stand-in at
    1e-11 relative (gradient: to max|g|), tests/test_gpu_ard.py's tolerance and reasoning; the stand-in's own distance
    from the truth is asserted where the truth can be had."""
    n = 130
    X, y = synth(n, d=d, seed=100 + d, scale=2.0)
    hp = (0.5 * np.log(d) + np.linspace(0.9, 1.5, d)).tolist() + [0.3, -0.8]
    cov = tam.ARDMatern(hp, kind)
    sll, sg, _, _ = truth.standin(cov, X, y, X[:1])
    if truth.EXTENDED:
        t = truth.Truth(X, y, cov, keep=False)
        e = truth.errors_ll_grad(cov, sll, sg, t.ll, t.grad)
        print("d=%d stand-in against the truth: %s" % (d, e))
        assert max(e.values()) <= 1e-13, e
    g = handle(gp_mod, X, y, hp, kind)
    ll, gr = g.loglik_grad()
    K = g.compute_K_train()
    g.close()
    assert np.mean(np.abs(K) > 1e-3) > 0.5                        # far from diagonal
    el, eg = abs(ll - sll) / abs(sll), np.max(np.abs(gr - sg)) / np.max(np.abs(sg))
    print("d=%d kind %d: LL %.3e, gradient %.3e (of max|g|)" % (d, kind, el, eg))
    assert el <= CHUNK_TOL and eg <= CHUNK_TOL, (d, el, eg)


# ------------------------------------------------------------------ 6. replayed graphs see new length scales
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [300, 1025], ids=["graph-300", "launches-1025"])
def test_new_length_scales_reach_the_kernels(gp_mod, n, kind):
    """theta_A, theta_B, theta_A on one handle: the third evaluation equals the first bit for bit, the second a fresh
    handle's at theta_B -- also when only ONE theta_c differs.  300 rows replay a captured graph (the weights travel by
    the copy node at its head), 1025 rows are launched one by one."""
    d = 5
    X, y = synth(n, d=d, seed=n, scale=3.0)
    A = np.array([0.9, 0.5, 1.3, 0.7, 1.1, 0.2, -1.0])
    B1 = np.array([0.6, 1.2, 0.8, 1.0, 0.4, 0.3, -0.7])
    B2 = A.copy()
    B2[3] = 1.05

    def ev(g, hp, grad=True):
        g.set_loghyperparam(hp)
        return g.loglik_grad() if grad else (g.compute_loglikelihood(), np.zeros(0))
    for B in (B1, B2):
        for grad in (True, False):
            g = handle(gp_mod, X, y, A, kind)
            first, second, third = ev(g, A, grad), ev(g, B, grad), ev(g, A, grad)
            g.close()
            f = handle(gp_mod, X, y, B, kind)
            fresh = ev(f, B, grad)
            f.close()
            assert third[0] == first[0] and np.array_equal(third[1], first[1])
            assert second[0] == fresh[0] and np.array_equal(second[1], fresh[1])
            assert second[0] != first[0]


# ------------------------------------------------------------------ 7. reproducibility
@pytest.mark.parametrize("kind", KINDS)
def test_ten_evaluations_identical_bits(gp_mod, kind):
    X, y = synth(1300, d=6, seed=5, scale=2.5)
    g = handle(gp_mod, X, y, [0.6, 0.8, 0.9, 1.0, 1.1, 1.3, 0.2, -1.0], kind)
    ll0, gr0 = g.loglik_grad()
    for _ in range(9):
        g.set_data(X, y)                                          # invalidates what the handle holds: a full evaluation
        ll, gr = g.loglik_grad()
        assert ll == ll0 and np.array_equal(gr, gr0)
    g.close()


# ------------------------------------------------------------------ 8. joint covariance and draws
JOINT_CASES = [pytest.param("n65_d2", M52, id="n65_d2"), pytest.param("n257_d3", M52, id="n257_d3"),
               pytest.param("n300_d17", M32, id="n300_d17-matern32")]   # (the last: the nu = 3/2 instantiation of the epilogue)


@extended
@pytest.mark.parametrize("name, kind", JOINT_CASES)
def test_joint_covariance_and_draws(gp_mod, oracle, name, kind):
    """nu = 5/2, and nu = 3/2 once.  cugp_predict_cov with and without noise against the truth's joint covariance at the bound
    tests/test_gpu_matern.py holds it to (the variance's yardstick, the covariance floor; this family's factor); cov exactly
    symmetric, the mean cugp_predict's bits.  Draws: zero normals give the mean's bits, unit normals pick columns of the
    Cholesky factor of the library's own covariance (against LAPACK's factor of the same fp64 matrix: two backward-stable
    factorisations differ by about nt eps cond(cov) relative to the factor's scale)."""
    c = tam.live(oracle, name, kind)
    X, y, Xt, hp, t, noise, fl = c["X"], c["y"], c["Xt"], c["cov"].hp, c["t"], c["noise"], c["floor"]
    rep = Report("%s/%s" % (name, tam.FAMILY[kind]), c["cov"])
    g = handle(gp_mod, X, y, hp, kind)
    m, _ = g.compute_test_means_and_variances(X, y, Xt)
    for with_noise in (True, False):
        tmj, tcov = t.joint(Xt, with_noise)
        mj, cov = g.compute_test_joint(X, y, Xt, with_noise=with_noise)
        assert np.array_equal(cov, cov.T) and same_bits([mj], [m])
        tag = "joint_noise_" if with_noise else "joint_latent_"
        rep.add(tag + "mean", np.max(np.abs(mj.astype(LD) - tmj)), noise["mean"], fl["mean"])
        rep.add(tag + "cov", np.max(np.abs(cov.astype(LD) - tcov)), noise["var"], fl["cov"])
    nt = Xt.shape[0]
    mj, cov = g.compute_test_joint(X, y, Xt, with_noise=True)
    z0 = g.sample_posterior(X, y, Xt, 2, with_noise=True, normals=np.zeros((2, nt)))
    assert same_bits([z0[0], z0[1]], [mj, mj])
    units = np.eye(nt)[[0, nt // 2, nt - 1]]
    draws = g.sample_posterior(X, y, Xt, 3, with_noise=True, normals=units)
    Lc = np.linalg.cholesky(cov)
    sv = float(np.exp(2 * hp[-2]) + np.exp(2 * hp[-1]))
    for s, k in enumerate((0, nt // 2, nt - 1)):
        err = np.max(np.abs(draws[s] - mj - Lc[:, k]))
        print("draw along unit normal %d: |sample - mean - C[:, k]| %.3e" % (k, err))
        assert err <= nt * 2.0 ** -52 * np.linalg.cond(cov) * np.sqrt(sv), (k, err)
    g.close()
    rep.check()


# ------------------------------------------------------------------ 9. gradients with respect to the test inputs
GRAD_CASES = [("n65_d2", M32, None), ("n65_d2", M52, None), ("n257_d3_shift", M32, None), ("n257_d3_shift", M52, None),
              ("n300_d17", M52, None), ("n257_d3", M52, 129)]


@extended
@pytest.mark.parametrize("name, kind, nt", GRAD_CASES,
                         ids=["%s-%s-nt%s" % (n, tam.KIND_NAMES[k], t or 64) for n, k, t in GRAD_CASES])
def test_predict_grad(gp_mod, oracle, name, kind, nt):
    """cugp_predict_grad: dmean and dvar at the bound of tests/truth_predict_grad.py for the ARD family (F_ARD yardsticks of
    the oracle-order evaluation); mean / var carry cugp_predict's bits; the latent call has the same dmean and dvar bits;
    the mean-only call (no second triangular product) the same dmean bits."""
    c = tam.grad_case(oracle, name, kind, nt)
    tpg.assert_yardstick_is_sane(c, (name, kind, nt))
    X, y, Xt, cov = c["X"], c["y"], c["Xt"], c["cov"]
    rep = Report("grad/%s/%s/nt%d" % (name, tam.FAMILY[kind], len(Xt)), cov)
    g = handle(gp_mod, X, y, cov.hp, kind)
    try:
        m, v, dm, dv = g.predict_grad(Xt)
        assert np.all(np.isfinite(dm)) and np.all(np.isfinite(dv))
        tpg.hold(rep, c, dm, dv)
        assert same_bits([m, v], g.compute_test_means_and_variances(None, None, Xt))
        ml, vl, dml, dvl = g.predict_grad(Xt, with_noise=False)
        assert same_bits([dml, dvl], [dm, dv]) and same_bits([ml, vl], g.predict_latent(Xt))
        mo, vo, dmo, none = g.predict_grad(Xt, want_var_grad=False)
        assert none is None and same_bits([mo, vo, dmo], [m, v, dm])
    finally:
        g.close()
    rep.check()


# ------------------------------------------------------------------ 10. multi-target regression
TARGET_CASES = [pytest.param(M52, "n257_d3", 1, id="1"), pytest.param(M52, "n257_d3", 5, id="5"),
                pytest.param(M52, "n257_d3", 17, id="17"), pytest.param(M32, "n300_d17", 3, id="matern32-n300_d17-m3")]


@extended
@pytest.mark.parametrize("kind, name, m", TARGET_CASES)
def test_targets(gp_mod, oracle, kind, name, m):
    """n257_d3, nu = 5/2, through tests/truth_targets.py's truth and bound with this family's descriptor; m = 17 crosses the
    16-target staging chunk of the gradient pass.  n300_d17, nu = 3/2: the other instantiation of the gradient pass, across
    a tile and a feature-chunk boundary."""
    c = tt.case(oracle, tam.FAMILY[kind], name, m)
    cov = c["cov"]
    rep = Report("targets/%s/m%d" % (tam.FAMILY[kind], m), cov)
    g = handle(gp_mod, c["X"], c["y"], cov.hp, kind)
    try:
        g.set_targets(np.asarray(c["Y"]).T)
        assert g.num_targets == m
        ll, gr, each = g.loglik_grad_targets()
        mean, var = g.predict_targets(c["Xt"])
        A = g.get_alpha_targets()
        assert gr.shape == (len(cov.hp),) and each.shape == (m,) and mean.shape == (len(c["Xt"]), m)
        tt.hold(rep, c, ll, gr, mean, each)
        rep.add("alpha", tt.alpha_error(c, A.T), c["solve"]["alpha"], truth.U4, truth.F_SOLVE)
        assert same_bits([var], [g.compute_test_means_and_variances(None, None, c["Xt"])[1]])
    finally:
        g.close()
    rep.check()


# ------------------------------------------------------------------ 11. appending observations
@extended
def test_append(gp_mod, oracle):
    """nu = 5/2: 120 rows in a handle with room for 256, evaluated, then 1 row and then 10 rows appended (the second crosses
    the 128-row tile).  Everything at all 131 rows against their truth through tests/truth_append.py's bound for the ARD
    family (what a fresh handle on all rows is held to)."""
    n, d = 131, 3
    X, y = synth(n, d=d, seed=3 * n + d, scale=4.0)
    Xt = np.ascontiguousarray(truth.points(X, d, 4.0))
    cov = tam.ARDMatern([0.9, 0.3, 1.6, 0.2, -1.0], M52)
    c = accuracy.case_at(oracle, cov, X, y, Xt, truth.Truth(X, y, cov), truth.solve_rows(n))
    accuracy.assert_yardstick_is_sane(c, "append")
    rep = Report("append/%s/120+1+10" % tam.FAMILY[M52], cov)
    g = gp_mod.Covsum(120, d, npad_min=256, kernel=tam.FAMILY[M52])
    try:
        g.set_loghyperparam(cov.hp)
        g.set_data(X[:120], y[:120])
        g.loglik_grad()
        g.append(X[120], y[120])
        g.append(X[121:], y[121:])
        assert g.n == n and g.capacity == 256
        ll, gr = g.loglik_grad()
        m, v = g.compute_test_means_and_variances(None, None, Xt)
        Ki = g.get_K_inverse()
        assert np.array_equal(Ki, Ki.T)
        ta.hold(rep, c, "ard", ll, gr, m, v, g.get_alpha(), Ki)
    finally:
        g.close()
    rep.check()


# ------------------------------------------------------------------ 12. the product of experts
HP_BCM = [0.9, 0.3, 1.6, 0.2, -1.0]
BCM_CASES = [(3 * 300, 3, M32), (3 * 300, 3, M52), (5 * 261 + 2, 5, M52)]


def bcm_of(gp_mod, X, y, rows, kind):
    b = gp_mod.BCM(rows, X.shape[1], kernel=tam.FAMILY[kind])
    off = 0
    for k, r in enumerate(rows):
        b.set_expert_data(k, X[off: off + r], y[off: off + r])
        off += r
    return b


@extended
@pytest.mark.parametrize("N, K, kind", BCM_CASES, ids=["3x300-matern32", "3x300-matern52", "5-uneven-matern52"])
def test_bcm_against_the_truth(gp_mod, oracle, N, K, kind):
    """A 3-expert group of equal experts (cugp_bcm_create_ard_kernel + expert data) and an uneven 5-expert split
    (BCM.split), d = 3: summed LL, every gradient component and the product-of-experts prediction against the truth in
    tests/truth_ard_bcm.py's form at F_ARD.  predict(combine=) runs for all four rules."""
    d = 3
    X, y = synth(N, d=d, seed=N + K, scale=4.0)
    Xt = np.ascontiguousarray(truth.points(X, d, 4.0))
    cov = tam.ARDMatern(HP_BCM, kind)
    parts = truth.bcm_rows(N, K)
    c = tam.bcm_case_at(oracle, cov, X, y, parts, Xt)
    b = bcm_of(gp_mod, X, y, [r for _, r in parts], kind) if K == 3 else gp_mod.BCM.split(X, y, K, kernel=tam.FAMILY[kind])
    try:
        assert b.rows == [r for _, r in parts] and b.ard and b.nh == d + 2 and b.kernel == tam.KIND_NAMES[kind]
        assert all(b.expert(k).kernel == tam.KIND_NAMES[kind] and b.expert(k).ard for k in range(K))
        b.set_BCM_log_hyperparam(cov.hp)
        ll, gr, per = b.loglik_grad()
        m, v = b.compute_BCM_test_means_and_var(Xt)
        assert gr.shape == (d + 2,) and per.shape == (K,)
        tb = c["tb"]
        rep = Report("bcm%dx/%s" % (K, tam.FAMILY[kind]), cov)
        rep.add_all("", truth.errors(cov, ll, gr, m, v, tb["ll"], tb["grad"], tb["mean"], tb["var"]), c["noise"], c["floor"])
        for mode in ("poe", "gpoe", "bcm", "rbcm"):
            pm, pv = b.predict(Xt, combine=mode)
            assert pm.shape == (len(Xt),) and np.all(np.isfinite(pm)) and np.all(pv > 0), mode
    finally:
        b.close()
    rep.check()


def test_group_of_se_ard_and_matern_ard_is_refused(gp_mod):
    L = capi.lib()
    L.cugp_group_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_void_p)]
    L.cugp_group_destroy.argtypes = [C.c_void_p]
    L.cugp_group_destroy.restype = None
    gs = [gp_mod.Covsum(200, 3, ard=True), gp_mod.Covsum(200, 3, kernel="matern52_ard"),
          gp_mod.Covsum(200, 3, kernel="matern52_ard"), gp_mod.Covsum(200, 3, kernel="matern32_ard"),
          gp_mod.Covsum(200, 3, kernel="matern52")]
    grp = C.c_void_p()
    for pair, why in (((0, 1), b"kernel kinds"), ((1, 0), b"kernel kinds"), ((1, 3), b"kernel kinds"),
                      ((1, 4), b"ARD and isotropic"), ((4, 1), b"ARD and isotropic")):
        hs = (C.c_void_p * 2)(*[gs[i].handle.value for i in pair])
        assert L.cugp_group_create(hs, 2, C.byref(grp)) == INV, pair
        assert why in L.cugp_last_error() and not grp.value, (pair, L.cugp_last_error())
    hs = (C.c_void_p * 2)(gs[1].handle.value, gs[2].handle.value)
    capi.check(L.cugp_group_create(hs, 2, C.byref(grp)))
    L.cugp_group_destroy(grp)
    for g in gs:
        g.close()


def test_sharded_bcm_one_rank_has_bcm_bits(gp_mod):
    """ShardedBCM(kernel="matern52_ard") at one rank through the library's exchange (a world of one needs no RCCL): the bits
    of gp.BCM over the same experts."""
    import torch
    from cugp_amd.bcm import ShardedBCM
    X, y = synth(3 * 300, 3, seed=4, scale=4.0)
    experts = [(X[300 * k:300 * (k + 1)], y[300 * k:300 * (k + 1)]) for k in range(3)]
    Xt = np.random.default_rng(1).uniform(-4, 4, (70, 3))
    env = os.environ.pop("CUGP_BCM_EXCHANGE", None)
    try:
        sb = ShardedBCM(experts, rank=0, world=1, device=0, comm_device=torch.device("cuda", 0), kernel="matern52_ard")
    finally:
        if env is not None:
            os.environ["CUGP_BCM_EXCHANGE"] = env
    assert sb.exchange_form == "library" and sb.kernel == "matern52" and sb.ard and sb.nh == 5
    ref = bcm_of(gp_mod, X, y, [300, 300, 300], M52)
    sb.set_loghyper(HP_BCM)
    ref.set_BCM_log_hyperparam(HP_BCM)
    ll, g, per = sb.loglik_grad()
    ll0, g0, per0 = ref.loglik_grad()
    m, v = sb.predict(Xt)
    assert sb.predict_form == "library"
    m0, v0 = ref.compute_BCM_test_means_and_var(Xt)
    sb.close()
    ref.close()
    assert same_bits([ll, g, per, m, v], [ll0, g0, per0, m0, v0])


# ------------------------------------------------------------------ 13. the optimiser
def test_cg_solve_ard_finds_the_relevant_dimension(gp_mod):
    """tests/test_gpu_ard.py's scenario and sizes at nu = 5/2: y depends on x_0 only.  cg_solve (budget 60) against
    cugp_cg_minimize_n driven by the CPU stand-in: probe for probe while the objective still moves (5e-5), end point 5e-5
    (2e-3 where the run ended on the plateau), final objective 1e-7.  The final -LL is lower than the isotropic Matern
    cg_solve's on the same data, and theta_1, theta_2, theta_3 each end above theta_0 + 1."""
    X, y = synth(300, d=4, scale=3.0)
    start = [0.5] * 4 + [0.5, 0.5]

    def fn(th):
        try:
            ll, g, _, _ = truth.standin(tam.ARDMatern(th, M52), X, y, X[:1])
        except np.linalg.LinAlgError:
            return float("nan"), np.full(6, np.nan)
        return -ll, g
    th_cpu, tr_cpu = gp_mod.cg_minimize_n(fn, start, 60)
    g = handle(gp_mod, X, y, start, M52)
    tr = g.cg_solve(budget=60)
    th = g.get_loghyperparam()
    f_end = -g.compute_loglikelihood()
    g.close()
    assert tr.shape[1] == 7
    f_cpu = fn(th_cpu)[0]
    n = min(len(tr), len(tr_cpu))
    err = np.abs(tr[:n, :6] - tr_cpu[:n, :6]) / np.maximum(1.0, np.abs(tr_cpu[:n, :6]))
    moving = np.abs(tr_cpu[:n, 6] - f_cpu) > 1e-9 * abs(f_cpu)
    print("ARD Matern cg_solve: %d probes (CPU %d), %d while the objective moves, max rel. deviation there %.2e; end %s f %.10g (CPU %.10g)"
          % (len(tr), len(tr_cpu), moving.sum(), np.max(err[moving]), th, f_end, f_cpu))
    assert moving.sum() >= 20 and np.all(err[moving] <= 5e-5), (int(moving.sum()), float(np.max(err[moving])))
    assert len(tr) == len(tr_cpu) or not moving[-1], (len(tr), len(tr_cpu))
    assert np.allclose(th, th_cpu, atol=5e-5 if moving[-1] else 2e-3), (th, th_cpu)
    assert abs(f_end - f_cpu) <= 1e-7 * abs(f_cpu), (f_end, f_cpu)

    gi = gp_mod.Covsum(300, 4, kernel="matern52")
    gi.set_loghyperparam([0.5, 0.5, 0.5])
    tri = gi.cg_solve(X, y, budget=60)
    f_iso = -gi.compute_loglikelihood()
    gi.close()
    print("isotropic Matern cg_solve: %d probes, end f %.10g" % (len(tri), f_iso))
    assert f_end < f_iso - 50.0, (f_end, f_iso)
    assert np.all(th[1:4] > th[0] + 1.0), th


# ------------------------------------------------------------------ 14. existing results untouched
_ISOLATION = r"""
import json, sys
import numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import cugp_amd.gp as gp
from conftest import synth

def bits(n, d, hp, **kw):
    X, y = synth(n, d=d, seed=n, scale=3.0)
    g = gp.Covsum(n, d, **kw)
    g.set_data(X, y)
    g.set_loghyperparam(hp)
    ll, gr = g.loglik_grad()
    m, v = g.compute_test_means_and_variances(X, y, X[:7] * 0.5)
    g.close()
    return [float(ll).hex()] + [float(x).hex() for x in np.concatenate([gr, m, v])]

def existing():
    return dict(se_ard=bits(300, 5, [0.9, 0.5, 1.3, 0.7, 1.1, 0.2, -1.0], ard=True),
                se_ard_1025=bits(1025, 5, [0.9, 0.5, 1.3, 0.7, 1.1, 0.2, -1.0], ard=True),
                matern52=bits(300, 5, [0.9, 0.2, -1.0], kernel="matern52"),
                se=bits(300, 5, [0.9, 0.2, -1.0]))

before = existing()                      # no ARD Matern handle has existed in this process yet
for n, d in ((300, 5), (1025, 5), (200, 17), (1300, 3)):
    for kernel in ("matern32_ard", "matern52_ard"):
        bits(n, d, np.linspace(0.6, 1.2, d).tolist() + [0.2, -1.0], kernel=kernel)
after = existing()
print("ISOLATION " + json.dumps(dict(before=before, after=after)))
"""


def test_existing_bits_do_not_depend_on_ard_matern_handles():
    """An SE-ARD handle (300 rows: graph; 1025: launches), an isotropic Matern-5/2 handle and an SE handle evaluated before
    any ARD Matern handle exists in the process (a fresh child process), and new ones on the same data after ARD Matern
    handles of the same and of other sizes have run and been destroyed: identical bits (LL, gradient, prediction)."""
    script = _ISOLATION % dict(root=ROOT, tests=os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [s for s in r.stdout.splitlines() if s.startswith("ISOLATION ")][-1]
    out = json.loads(line[len("ISOLATION "):])
    assert out["before"] == out["after"]
    assert sorted(out["before"]) == ["matern52", "se", "se_ard", "se_ard_1025"]
    assert len(out["before"]["se_ard"]) == 1 + 7 + 14 and len(out["before"]["se"]) == 1 + 3 + 14


@pytest.mark.parametrize("n, graphs", [(300, 1), (1025, 0)], ids=["graph-300", "launches-1025"])
def test_kind_zero_is_cugp_create_ard(gp_mod, n, graphs):
    """Kind 0 through cugp_create_ard_kernel against cugp_create_ard: LL, gradient, prediction and joint covariance bit for
    bit, replaying a captured graph (300 rows) and launch by launch (1025 rows, tuning key 5 = 0)."""
    d = 5
    X, y = synth(n, d=d, seed=n, scale=3.0)
    Xt = synth(40, d=d, seed=7, scale=3.0)[0]
    ref = gp_mod.Covsum(n, d, ard=True)
    h = C.c_void_p()
    capi.check(capi.lib().cugp_create_ard_kernel(n, d, 0, 0, capi.CUGP_KERNEL_SE, C.byref(h)))
    new = gp_mod.Covsum.__new__(gp_mod.Covsum)
    new.n, new.d, new.device, new.ard, new.nh, new._kind, new._h, new._data_key = n, d, 0, True, d + 2, 0, h, None
    assert new.kernel == "se" and ref.kernel == "se" and new.get_param_dim() == d + 2
    out = []
    for g in (ref, new):
        g.set_tuning(TUNE_GRAPHS, graphs)
        g.set_data(X, y)
        g.set_loghyperparam([0.9, 0.5, 1.3, 0.7, 1.1, 0.2, -1.0])
        ll, gr = g.loglik_grad()
        m, v = g.compute_test_means_and_variances(X, y, Xt)
        mj, cov = g.compute_test_joint(X, y, Xt, with_noise=True)
        g.set_data(X, y)
        out.append([ll, gr, m, v, mj, cov, g.compute_loglikelihood()])
        g.close()
    assert same_bits(out[0], out[1])


# ------------------------------------------------------------------ 15. refusals
@pytest.mark.parametrize("kind", KINDS)
def test_refusals(gp_mod, kind):
    """The 3-entry calls on an ARD Matern handle and nh != d + 2 give CUGP_ERR_INVALID with the call to use; the handle's
    results afterwards have the bits from before."""
    L = capi.lib()
    X, y = synth(150, d=3, seed=8, scale=3.0)
    hp = [0.9, 0.5, 1.2, 0.2, -1.0]
    g = handle(gp_mod, X, y, hp, kind)
    want = g.loglik_grad()
    h = g.handle
    v, ll, ne, ng, nh, kk = np.zeros(8), C.c_double(), C.c_int(), C.c_int(), C.c_int(), C.c_int(-1)
    p = capi.ptr(v)
    S = np.empty((150, 150))
    assert L.cugp_num_hyper(h, C.byref(nh)) == 0 and nh.value == 5
    assert L.cugp_kernel_kind(h, C.byref(kk)) == 0 and kk.value == kind
    for name, call, use in [
            ("cugp_set_loghyper", lambda: L.cugp_set_loghyper(h, p), b"cugp_set_loghyper_ard"),
            ("cugp_get_loghyper", lambda: L.cugp_get_loghyper(h, p), b"cugp_get_loghyper_ard"),
            ("cugp_loglik_grad", lambda: L.cugp_loglik_grad(h, C.byref(ll), p), b"cugp_loglik_grad_ard"),
            ("cugp_grad", lambda: L.cugp_grad(h, p), b"cugp_loglik_grad_ard"),
            ("cugp_loglik_grad_fetch", lambda: L.cugp_loglik_grad_fetch(h, C.byref(ll), p), b"cugp_loglik_grad_fetch_ard"),
            ("cugp_cg_solve", lambda: L.cugp_cg_solve(h, 5, None, 0, C.byref(ne)), b"cugp_cg_solve_ard"),
            ("cugp_cg_solve_sparing", lambda: L.cugp_cg_solve_sparing(h, 5, None, 0, C.byref(ne), C.byref(ng)), b"cugp_cg_solve_ard"),
            ("cugp_rprop_solve", lambda: L.cugp_rprop_solve(h, 5, None, 0, C.byref(ne)), b"cugp_cg_solve_ard"),
            ("cugp_compute_squared_dist", lambda: L.cugp_compute_squared_dist(h, 1.0, capi.ptr(S)), b"cugp_compute_K_train")]:
        assert call() == INV, name
        msg = L.cugp_last_error()
        assert name.encode() in msg and use in msg, (name, msg)
        got = g.loglik_grad()
        assert got[0] == want[0] and np.array_equal(got[1], want[1]), name
    for bad in (4, 6, 3):
        assert L.cugp_set_loghyper_ard(h, p, bad) == INV and L.cugp_get_loghyper_ard(h, p, bad) == INV
        assert L.cugp_loglik_grad_ard(h, C.byref(ll), p, bad) == INV
        assert L.cugp_loglik_grad_fetch_ard(h, C.byref(ll), p, bad) == INV
    g.set_data(X, y)
    again = g.loglik_grad()
    assert again[0] == want[0] and np.array_equal(again[1], want[1])
    assert np.array_equal(g.get_loghyperparam(), hp)
    g.close()
