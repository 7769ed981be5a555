"""GPU tests of the rational quadratic kernel, with one length scale per dimension (kernel="rq_ard", nh = d + 3) and with
one tied length scale (kernel="rq", nh = 4); cugp_create_rq, cugp_bcm_create_rq.

Accuracy is held to fp64 rounding against the extended-precision truth of tests/truth_rq.py (truth.Truth with the RQ
descriptor) through the harness of tests/accuracy.py:

    err_gpu(q) <= F_RQ * max(noise(q), floor(q)),   alpha and 64 rows of K^-1 at F_SOLVE

F_RQ comes from the CPU stand-in (tests/test_truth_rq_cpu.py, docs/ACCURACY.md).  Every figure is printed before it is
asserted (run with -s).  One process, one device; nothing outside the tree is read.
"""
import ctypes as C
import math
import os

import numpy as np
import pytest

import accuracy
import truth
import truth_append as ta
import truth_ard_matern as tam
import truth_loo as tl
import truth_predict_grad as tpg
import truth_rq as trq
import truth_targets as tt
from accuracy import Report
from conftest import synth
from cugp_amd import capi

pytestmark = pytest.mark.gpu
extended = pytest.mark.skipif(not truth.EXTENDED, reason="numpy.longdouble is not an extended-precision type here")

LD = truth.LD
INV = capi.CUGP_ERR_INVALID
TUNE_GRAPHS = 5                                                  # kernels.h TUNE_*
FORMS = ["rq_ard", "rq"]
JOINT_CASES_TIED = ("n65", "n257_d3")              # the tied form shares the ARD epilogue: its two smallest cases


@pytest.fixture(scope="module")
def gp_mod():
    import cugp_amd.gp as gp
    return gp


def handle(gp_mod, X, y, hp, family, overlap=None, cap=0, tuning=None):
    g = gp_mod.Covsum(X.shape[0], X.shape[1], npad_min=cap, kernel=family)
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


def untied(hp, d):
    """theta of the "rq_ard" handle that is the "rq" handle's model: the length scale d times."""
    return [hp[0]] * d + list(hp[1:])


# ------------------------------------------------------------------ 1. accuracy
@extended
@pytest.mark.parametrize("family, name", trq.ALL_CASES, ids=["%s-%s" % c for c in trq.ALL_CASES])
def test_accuracy_live(gp_mod, oracle, family, name):
    """loglik_grad with all nh components, the LL-only path, prediction at 64 points (one a training row), alpha and 64 rows
    of K^-1 (F_SOLVE); the joint covariance with and without noise on JOINT_CASES_RQ and, tied, on JOINT_CASES_TIED."""
    c = trq.live(oracle, family, name)
    accuracy.assert_yardstick_is_sane(c, (family, name))
    X, y, cov = c["X"], c["y"], c["cov"]
    nh = 4 if family == "rq" else X.shape[1] + 3

    def fresh(g):
        assert g.ard == (family == "rq_ard") and g.nh == nh and g.get_param_dim() == nh and g.kernel == "rq"
    accuracy.hold_live_case(Report("%s/%s" % (name, family), cov), c,
                            lambda overlap=None: handle(gp_mod, X, y, cov.hp, family, overlap),
                            joint=name in (trq.JOINT_CASES_RQ if family == "rq_ard" else JOINT_CASES_TIED), fresh=fresh)


@extended
@pytest.mark.parametrize("family, name", trq.ALL_CASES, ids=["%s-%s" % c for c in trq.ALL_CASES])
def test_latent_variance(gp_mod, oracle, family, name):
    """predict_latent on every case of both forms: the mean's bits, and the variance without sn2 at the variance's yardstick."""
    c = trq.live(oracle, family, name)
    g = handle(gp_mod, c["X"], c["y"], c["cov"].hp, family)
    m, v = g.compute_test_means_and_variances(None, None, c["Xt"])
    ml, vl = g.predict_latent(c["Xt"])
    g.close()
    rep = Report("latent/%s/%s" % (name, family), c["cov"])
    rep.add("var_latent", np.max(np.abs(vl.astype(LD) - (c["tv"] - c["cov"].sn2))), c["noise"]["var"], c["floor"]["var"])
    assert same_bits([ml], [m])
    rep.check()


# ------------------------------------------------------------------ 2. K and k_test
@extended
@pytest.mark.parametrize("family, name", [("rq_ard", "n65_d2"), ("rq_ard", "n257_d3_shift"), ("rq_ard", "n300_d17"),
                                          ("rq_ard", "n515_d33"), ("rq", "n300_d17")])
def test_K_and_k_test_entries(gp_mod, family, name):
    """cugp_compute_K_train and cugp_compute_k_test entry by entry against the truth, inside the derived bound
    (truth_rq.k_entry_bound); K exactly symmetric, its diagonal bit-equal to sf2 + sn2 as fp64 forms it."""
    X, y, Xt, cov = trq.inputs(family, name)
    n = X.shape[0]
    g = handle(gp_mod, X, y, cov.hp, family)
    K = g.compute_K_train()
    Ks = g.compute_k_test(Xt)
    g.close()
    assert np.array_equal(K, K.T)
    assert np.all(np.diag(K) == math.exp(cov.hp[-2] * 2) + math.exp(cov.hp[-1] * 2))
    Kf = K.copy()
    Kf[np.arange(n), np.arange(n)] = math.exp(cov.hp[-2] * 2)
    worst = dict(K=trq.entry_excess(Kf, X, X, cov), k_test=trq.entry_excess(Ks, Xt, X, cov))
    print("ACC %s/%s largest |entry - truth| / bound: K %.3f  k_test %.3f" % (name, family, worst["K"], worst["k_test"]))
    assert worst["K"] <= 1.0 and worst["k_test"] <= 1.0, worst


# ------------------------------------------------------------------ 3. tied = ARD in bits
@pytest.mark.parametrize("n, d", [(65, 2), (300, 17)])
def test_tied_is_ard_at_equal_scales_in_bits(gp_mod, n, d):
    """LL, predictions and K entries identical; g_0 of the tied handle is the index-order sum of the ARD handle's length
    components, the other three components are identical -- bit for bit."""
    X, y = synth(n, d=d, seed=3 * n + d, scale=2.0)
    Xt = synth(70, d=d, seed=7, scale=2.0)[0]
    hp = [1.1, 0.4, 0.3, -0.8]
    gt, ga = handle(gp_mod, X, y, hp, "rq"), handle(gp_mod, X, y, untied(hp, d), "rq_ard")
    try:
        assert same_bits([gt.compute_K_train(), gt.compute_k_test(Xt)], [ga.compute_K_train(), ga.compute_k_test(Xt)])
        (llt, grt), (lla, gra) = gt.loglik_grad(), ga.loglik_grad()
        assert grt.shape == (4,) and gra.shape == (d + 3,)
        s = gra[0]
        for c in range(1, d):
            s = s + gra[c]
        assert same_bits([llt, grt[0], grt[1:]], [lla, s, gra[d:]]), (grt, gra)
        assert same_bits(gt.compute_test_means_and_variances(None, None, Xt), ga.compute_test_means_and_variances(None, None, Xt))
        assert same_bits([gt.compute_loglikelihood()], [ga.compute_loglikelihood()])
        assert same_bits(gt.predict_grad(Xt), ga.predict_grad(Xt))
        lt, la = gt.loo(), ga.loo()
        s = la[1][0]
        for c in range(1, d):
            s = s + la[1][c]
        assert same_bits([lt[0], lt[1][0], lt[1][1:]], [la[0], s, la[1][d:]])
    finally:
        gt.close()
        ga.close()


# ------------------------------------------------------------------ 4. extremes, n = 65 (two build tiles)
def test_duplicate_rows_give_exactly_sf2(gp_mod):
    X, y = synth(65, d=3, seed=9, scale=3.0)
    X[64] = X[0]
    X[33] = X[32]
    hp = [0.5, 0.9, 1.2, 0.4, 0.3, -1.0]
    g = handle(gp_mod, X, y, hp, "rq_ard")
    K = g.compute_K_train()
    g.close()
    sf2 = math.exp(0.3 * 2)
    assert K[64, 0] == sf2 and K[0, 64] == sf2 and K[33, 32] == sf2 and K[32, 33] == sf2


@pytest.mark.parametrize("family, n, d", [("rq_ard", 65, 2), ("rq", 65, 2), ("rq_ard", 300, 3)])
def test_overflowing_alpha_gives_nan_and_the_handle_recovers(gp_mod, family, n, d):
    """theta_alpha = 800: exp overflows, every result is NaN with CUGP_OK; the next evaluation at a healthy theta has a fresh
    handle's bits (300 rows replay a captured graph: the new alpha travels by the copy at its head)."""
    X, y = synth(n, d=d, seed=n, scale=3.0)
    Xt = synth(9, d=d, seed=7, scale=3.0)[0]
    nl = d if family == "rq_ard" else 1
    good = [0.7] * nl + [0.4, 0.3, -1.0]
    bad = [0.7] * nl + [800.0, 0.3, -1.0]
    g = handle(gp_mod, X, y, good, family)
    first = g.loglik_grad()
    g.set_loghyperparam(bad)
    ll, gr = g.loglik_grad()                                      # raises on any return code but CUGP_OK
    assert np.isnan(ll) and np.all(np.isnan(gr)) and np.isnan(g.compute_loglikelihood())
    K = g.compute_K_train()
    assert np.all(np.isnan(K[~np.eye(n, dtype=bool)]))
    g.set_loghyperparam(good)
    again = g.loglik_grad()
    p = g.compute_test_means_and_variances(None, None, Xt)
    g.close()
    f = handle(gp_mod, X, y, good, family)
    fresh = f.loglik_grad()
    pf = f.compute_test_means_and_variances(None, None, Xt)
    f.close()
    assert same_bits(again, fresh) and same_bits(again, first) and same_bits(p, pf)


def test_underflowing_weight_drops_its_dimension_exactly(gp_mod):
    X, y = synth(65, d=3, seed=11, scale=3.0)
    keep = [0, 2]
    hp = np.array([0.5, 800.0, 0.9, 0.4, 0.3, -1.0])
    g3 = handle(gp_mod, X, y, hp, "rq_ard")
    g2 = handle(gp_mod, np.ascontiguousarray(X[:, keep]), y, hp[[0, 2, 3, 4, 5]], "rq_ard")
    try:
        assert np.array_equal(g3.compute_K_train(), g2.compute_K_train())
        (ll3, gr3), (ll2, gr2) = g3.loglik_grad(), g2.loglik_grad()
        assert ll3 == ll2 and np.array_equal(gr3[[0, 2, 3, 4, 5]], gr2) and gr3[1] == 0.0, (gr3, gr2)
    finally:
        g3.close()
        g2.close()


# ------------------------------------------------------------------ 5. prediction beyond one test tile
@extended
@pytest.mark.parametrize("nt", [129, 200])
def test_prediction_beyond_one_test_tile(gp_mod, oracle, nt):
    c = accuracy.wide(oracle, "rq_ard", "n257_d3", nt)
    X, y, Xt, cov = c["X"], c["y"], c["Xt"], c["cov"]
    g = handle(gp_mod, X, y, cov.hp, "rq_ard")
    m, v = g.compute_test_means_and_variances(None, None, Xt)
    mj, cj = g.compute_test_joint(X, y, Xt, with_noise=False)
    g.close()
    rep = Report("wide/n257_d3/rq_ard/nt%d" % nt, cov)
    rep.add_all("", truth.errors_pred(m, v, c["tm"], c["tv"]), c["noise"], c["floor"])
    rep.add("joint_latent_cov", np.max(np.abs(cj.astype(LD) - c["tcov"])), c["noise"]["var"], c["floor"]["cov"])
    assert same_bits([mj], [m])
    rep.check()


# ------------------------------------------------------------------ 6. gradients with respect to the test inputs
_GRAD = {}


def grad_case(oracle, family, name, nt):
    if (family, name, nt) not in _GRAD:
        c = trq.live(oracle, family, name)
        Xt = truth.wide_inputs(name, nt, family)[2].copy()
        Xt[0] = Xt[0] + 50.0                                       # a far point: every G small
        _GRAD[family, name, nt] = tam.grad_case_at(oracle, c["cov"], c["X"], c["y"], Xt, c["t"])
    return _GRAD[family, name, nt]


@extended
@pytest.mark.parametrize("family, name", [("rq_ard", "n257_d3"), ("rq_ard", "n300_d17"), ("rq", "n257_d3")])
def test_predict_grad(gp_mod, oracle, family, name):
    """cugp_predict_grad at nt = 70 (two test tiles, a far point among them) against the longdouble gradient at the factor
    the ARD x Matern tests use (the family's own, truth_predict_grad.factor); the latent and the mean-only forms in bits."""
    c = grad_case(oracle, family, name, 70)
    tpg.assert_yardstick_is_sane(c, (family, name))
    X, y, Xt, cov = c["X"], c["y"], c["Xt"], c["cov"]
    rep = Report("grad/%s/%s/nt70" % (name, family), cov)
    g = handle(gp_mod, X, y, cov.hp, family)
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


# ------------------------------------------------------------------ 7. targets, append, leave-one-out
@extended
@pytest.mark.parametrize("family, name, m", [("rq_ard", "n257_d3", 3), ("rq_ard", "n257_d3", 17), ("rq", "n257_d3", 3),
                                             ("rq", "n300_d17", 17)])
def test_targets(gp_mod, oracle, family, name, m):
    """tests/truth_targets.py's truth and bound with this family's descriptor; m = 17 crosses the 16-target staging chunk."""
    c = tt.case(oracle, family, name, m)
    cov = c["cov"]
    rep = Report("targets/%s/%s/m%d" % (family, name, m), cov)
    g = handle(gp_mod, c["X"], c["y"], cov.hp, family)
    try:
        g.set_targets(np.asarray(c["Y"]).T)
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


@extended
@pytest.mark.parametrize("family, k", [("rq_ard", 1), ("rq_ard", 64), ("rq", 64)])
def test_append(gp_mod, oracle, family, k):
    """200 rows in a handle with room for 384, evaluated, then k rows appended (64 of them cross the 256-row tile edge);
    everything at all rows against their truth at tests/truth_append.py's form of the bound with the family's factor."""
    n0, d = 200, 3
    n = n0 + k
    X, y = synth(n, d=d, seed=3 * n + d, scale=4.0)
    Xt = np.ascontiguousarray(truth.points(X, d, 4.0))
    hp = [0.9, 0.3, 1.6, -0.7, 0.2, -1.0] if family == "rq_ard" else [0.9, -0.7, 0.2, -1.0]
    cov = trq.RQ(hp, tied=family == "rq")
    c = accuracy.case_at(oracle, cov, X, y, Xt, truth.Truth(X, y, cov), truth.solve_rows(n))
    accuracy.assert_yardstick_is_sane(c, "append")
    rep = Report("append/%s/200+%d" % (family, k), cov)
    g = gp_mod.Covsum(n0, d, npad_min=384, kernel=family)
    try:
        g.set_loghyperparam(hp)
        g.set_data(X[:n0], y[:n0])
        g.loglik_grad()
        g.append(X[n0] if k == 1 else X[n0:], y[n0] if k == 1 else y[n0:])
        assert g.n == n and g.capacity == 384
        ll, gr = g.loglik_grad()
        m, v = g.compute_test_means_and_variances(None, None, Xt)
        Ki = g.get_K_inverse()
        assert np.array_equal(Ki, Ki.T)
        e = truth.errors(cov, ll, gr, m, v, c["t"].ll, c["t"].grad, c["tm"], c["tv"])
        rep.add_all("", e, c["noise"], c["floor"])
        es = truth.solve_errors(g.get_alpha(), Ki, c["t"], c["rows"])
        for q in truth.SOLVE_QUANTITIES:
            rep.add(q, es[q], c["solve"][q], truth.U4, ta.F_SOLVE)
    finally:
        g.close()
    rep.check()


@extended
@pytest.mark.parametrize("family, name", [("rq_ard", "n65_d2"), ("rq_ard", "n300_d17"), ("rq", "n257_d3")])
def test_loo(gp_mod, oracle, family, name):
    """cugp_loo (objective, gradient with the alpha component) and cugp_loo_predict against tests/truth_loo.py's truth through
    the descriptor, yardstick: its textbook route with this family's derivative matrices (truth_rq.loo_case)."""
    c = trq.loo_case(oracle, family, name)
    tl.assert_yardstick_is_sane(c, (family, name))
    cov = c["cov"]
    rep = Report("loo/%s/%s" % (family, name), cov)
    g = handle(gp_mod, c["X"], c["y"], cov.hp, family)
    try:
        ll, gr = g.loo()
        mu, var, logp = g.loo_predict()
        assert gr.shape == (len(cov.hp),)
        trq.loo_hold(rep, c, ll, gr, mu, var, logp)
        assert same_bits([g.loo(want_grad=False)[0]], [ll])
    finally:
        g.close()
    rep.check()


# ------------------------------------------------------------------ 8. captured graph
@pytest.mark.parametrize("family", FORMS)
def test_new_alpha_weights_and_scalars_reach_a_replayed_graph(gp_mod, family):
    """theta_A, theta_B, theta_A on one 300-row handle (a captured graph, refreshed by ONE copy of scalars, weights and
    alpha): the third evaluation equals the first, the second a fresh handle's -- also when only alpha, one length scale,
    or sigma_f differs; the replay's bits are the launch-by-launch evaluation's (tuning key 5 = 0)."""
    d = 5
    X, y = synth(300, d=d, seed=300, scale=3.0)
    nl = d if family == "rq_ard" else 1
    A = np.array(list(np.linspace(0.7, 1.3, nl)) + [0.4, 0.2, -1.0])
    for k in (nl, 0, nl + 1):                                     # alpha, a length scale, sigma_f
        B = A.copy()
        B[k] += 0.37
        for grad in (True, False):
            def ev(g, hp):
                g.set_loghyperparam(hp)
                return g.loglik_grad() if grad else (g.compute_loglikelihood(), np.zeros(0))
            g = handle(gp_mod, X, y, A, family)
            first, second, third = ev(g, A), ev(g, B), ev(g, A)
            g.close()
            f = handle(gp_mod, X, y, B, family)
            fresh = ev(f, B)
            f.close()
            p = handle(gp_mod, X, y, B, family, tuning={TUNE_GRAPHS: 0})
            plain = ev(p, B)
            p.close()
            assert same_bits(third, first) and same_bits(second, fresh) and same_bits(second, plain)
            assert second[0] != first[0]


# ------------------------------------------------------------------ 9. the product of experts
HP_BCM = {"rq_ard": [0.9, 0.3, 1.6, 0.4, 0.2, -1.0], "rq": [0.9, 0.4, 0.2, -1.0]}
BCM_CASES = [(3 * 300, 3, f) for f in FORMS] + [(5 * 261 + 2, 5, f) for f in FORMS]


def bcm_of(gp_mod, X, y, rows, family):
    b = gp_mod.BCM(rows, X.shape[1], kernel=family)
    off = 0
    for k, r in enumerate(rows):
        b.set_expert_data(k, X[off: off + r], y[off: off + r])
        off += r
    return b


@extended
@pytest.mark.parametrize("N, K, family", BCM_CASES, ids=["%dx-%s" % (k, f) for _, k, f in BCM_CASES])
def test_bcm_against_the_truth(gp_mod, oracle, N, K, family):
    """3 x 300 equal experts (cugp_bcm_create_rq + expert data) and the uneven 5-way split of 1307 rows (BCM.split), d = 3:
    the group ran (predict_grad_form == 2); rows {LL, g[nh]}; summed LL, every gradient component and the product-of-experts prediction against the
    truth at F_RQ; the four combination rules; predict_grad batched equals expert by expert in bits; the world-of-one
    communicator forms of the three exchanges equal the in-process results in bits."""
    d = 3
    X, y = synth(N, d=d, seed=N + K, scale=4.0)
    Xt = np.ascontiguousarray(truth.points(X, d, 4.0))
    cov = trq.RQ(HP_BCM[family], tied=family == "rq")
    nh = len(cov.hp)
    parts = truth.bcm_rows(N, K)
    c = tam.bcm_case_at(oracle, cov, X, y, parts, Xt)
    b = bcm_of(gp_mod, X, y, [r for _, r in parts], family) if K == 3 else gp_mod.BCM.split(X, y, K, kernel=family)
    try:
        assert b.rows == [r for _, r in parts] and b.ard == (family == "rq_ard") and b.nh == nh and b.kernel == "rq"
        assert all(b.expert(k).kernel == "rq" and b.expert(k).nh == nh for k in range(K))
        b.set_BCM_log_hyperparam(cov.hp)
        ll, gr, per = b.loglik_grad()
        rows = b.loglik_grad_rows()
        assert rows.shape == (K, 1 + nh) and same_bits([rows[:, 0]], [per])
        s = rows[0, 1:].copy()
        for k in range(1, K):
            s = s + rows[k, 1:]
        assert same_bits([s], [gr])
        m, v = b.compute_BCM_test_means_and_var(Xt)
        assert gr.shape == (nh,) and per.shape == (K,)
        tb = c["tb"]
        rep = Report("bcm%dx/%s" % (K, family), cov)
        rep.add_all("", truth.errors(cov, ll, gr, m, v, tb["ll"], tb["grad"], tb["mean"], tb["var"]), c["noise"], c["floor"])
        for mode in ("poe", "gpoe", "bcm", "rbcm"):
            pm, pv = b.predict(Xt, combine=mode)
            assert pm.shape == (len(Xt),) and np.all(np.isfinite(pm)) and np.all(pv > 0), mode
        out = b.predict_grad(Xt)
        assert b.predict_grad_form == 2                           # every device set ran as ONE group of batched launches
        assert same_bits(out[:2], [m, v])
        b.expert(1).set_profiling(3)                              # a profiled expert: the set goes expert by expert
        one = b.predict_grad(Xt)
        assert b.predict_grad_form == 1
        b.expert(1).set_profiling(0)
        assert same_bits(out, one)
        comm = gp_mod.Comm(None, 0, 1, 0)                         # a world of one without an id: no collective library
        try:
            r = comm.loglik_grad_allgather(b, K, nh)
            assert r.shape == (K, 1 + nh) and same_bits([r], [rows])
            pm, pv = comm.predict_allgather(b, K, K, Xt)
            assert same_bits([pm, pv], [m, v])
            pg = comm.predict_grad_allgather(b, K, K, Xt, d)
            assert same_bits(pg, out)
        finally:
            comm.close()
    finally:
        b.close()
    rep.check()


@pytest.mark.parametrize("family", FORMS)
def test_bcm_create_split_rq_has_bcm_split_bits(gp_mod, family):
    """cugp_bcm_create_split_rq called directly (rows partitioned and data set inside the library) against BCM.split, which
    goes through cugp_bcm_create_rq and the experts' data calls: kind, nh, rows {LL, g[nh]} and the prediction in bits."""
    L = capi.lib()
    N, K, d = 5 * 261 + 2, 5, 3
    X, y = synth(N, d=d, seed=N + K, scale=4.0)
    Xt = np.ascontiguousarray(truth.points(X, d, 4.0))
    hp = HP_BCM[family]
    ref = gp_mod.BCM.split(X, y, K, kernel=family)
    dev = np.zeros(1, dtype=np.int32)
    h = C.c_void_p()
    capi.check(L.cugp_bcm_create_split_rq(capi.ptr(X), capi.ptr(y), N, d, K, 1, dev.ctypes.data_as(capi._ip),
                                          1 if family == "rq_ard" else 0, C.byref(h)))
    new = gp_mod.BCM.__new__(gp_mod.BCM)
    new.rows, new.d, new.device, new.devices = list(ref.rows), d, 0, [0]
    new._kind, new.ard, new.nh, new._h = ref._kind, ref.ard, ref.nh, h
    try:
        kk, nh = C.c_int(-1), C.c_int(-1)
        assert L.cugp_bcm_kernel_kind(h, C.byref(kk)) == 0 and kk.value == capi.CUGP_KERNEL_RQ
        assert L.cugp_bcm_num_hyper(h, C.byref(nh)) == 0 and nh.value == len(hp) and new.kernel == "rq"
        out = []
        for b in (ref, new):
            b.set_BCM_log_hyperparam(hp)
            out.append(list(b.loglik_grad()) + [b.loglik_grad_rows()] + list(b.compute_BCM_test_means_and_var(Xt)))
        assert same_bits(out[0], out[1])
    finally:
        ref.close()
        new.close()


@pytest.mark.parametrize("family", FORMS)
def test_sharded_bcm_one_rank_has_bcm_bits(gp_mod, family):
    """ShardedBCM at one rank through the library's exchange (a world of one needs no collective library): rows {LL, g[nh]},
    the prediction and its input gradients carry the in-process BCM's bits."""
    import torch
    from cugp_amd.bcm import ShardedBCM
    X, y = synth(3 * 300, 3, seed=4, scale=4.0)
    experts = [(X[300 * k:300 * (k + 1)], y[300 * k:300 * (k + 1)]) for k in range(3)]
    Xt = np.random.default_rng(1).uniform(-4, 4, (70, 3))
    env = os.environ.pop("CUGP_BCM_EXCHANGE", None)
    try:
        sb = ShardedBCM(experts, rank=0, world=1, device=0, comm_device=torch.device("cuda", 0), kernel=family)
    finally:
        if env is not None:
            os.environ["CUGP_BCM_EXCHANGE"] = env
    nh = len(HP_BCM[family])
    assert sb.exchange_form == "library" and sb.kernel == "rq" and sb.ard == (family == "rq_ard") and sb.nh == nh
    ref = bcm_of(gp_mod, X, y, [300, 300, 300], family)
    sb.set_loghyper(HP_BCM[family])
    ref.set_BCM_log_hyperparam(HP_BCM[family])
    ll, g, per = sb.loglik_grad()
    ll0, g0, per0 = ref.loglik_grad()
    m, v = sb.predict(Xt)
    assert sb.predict_form == "library"
    m0, v0 = ref.compute_BCM_test_means_and_var(Xt)
    sb.close()
    ref.close()
    assert same_bits([ll, g, per, m, v], [ll0, g0, per0, m0, v0])


def test_mixed_groups_are_refused(gp_mod):
    L = capi.lib()
    L.cugp_group_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_void_p)]
    L.cugp_group_destroy.argtypes = [C.c_void_p]
    L.cugp_group_destroy.restype = None
    gs = [gp_mod.Covsum(200, 3, kernel="rq_ard"), gp_mod.Covsum(200, 3, kernel="rq"), gp_mod.Covsum(200, 3, ard=True),
          gp_mod.Covsum(200, 3, kernel="rq_ard"), gp_mod.Covsum(200, 3, kernel="rq")]
    grp = C.c_void_p()
    for pair, why in (((0, 2), b"kernel kinds"), ((2, 1), b"kernel kinds"), ((0, 1), b"one length scale"),
                      ((1, 0), b"one length scale")):
        hs = (C.c_void_p * 2)(*[gs[i].handle.value for i in pair])
        assert L.cugp_group_create(hs, 2, C.byref(grp)) == INV, pair
        assert why in L.cugp_last_error() and not grp.value, (pair, L.cugp_last_error())
    for pair in ((0, 3), (1, 4)):
        hs = (C.c_void_p * 2)(*[gs[i].handle.value for i in pair])
        capi.check(L.cugp_group_create(hs, 2, C.byref(grp)))
        L.cugp_group_destroy(grp)
        grp = C.c_void_p()
    for g in gs:
        g.close()


# ------------------------------------------------------------------ 10. the optimiser
@pytest.mark.parametrize("family", FORMS)
def test_cg_solve(gp_mod, family):
    """cg_solve at 300 x 3 with budget 20: the trace (one row per evaluation) has nh + 1 columns, the end point lies below the
    first evaluation, and its LL equals a fresh handle's at that theta in bits.  cg_solve_loo records the optimiser's own iterates (the
    start and the point every line search ended at): along them the objective never rises."""
    X, y = synth(300, d=3, scale=3.0)
    nl = 3 if family == "rq_ard" else 1
    start = [0.5] * nl + [0.0, 0.5, 0.5]
    g = handle(gp_mod, X, y, start, family)
    tr = g.cg_solve(budget=20)
    th = g.get_loghyperparam()
    ll_end = g.compute_loglikelihood()
    g.close()
    assert tr.shape[1] == len(start) + 1 and len(tr) >= 3 and np.all(np.isfinite(tr))
    assert -ll_end < tr[0, -1] - 1.0, (tr[0], ll_end)
    fresh = handle(gp_mod, X, y, th, family)
    ll_fresh = fresh.compute_loglikelihood()
    fresh.close()
    print("%s cg_solve: %d probes, f %.6f -> %.6f, theta %s" % (family, len(tr), tr[0, -1], -ll_end, th))
    assert same_bits([ll_end], [ll_fresh])
    g = handle(gp_mod, X, y, start, family)
    it = g.cg_solve_loo(budget=20)
    end = g.get_loghyperparam()
    g.close()
    assert it.shape[1] == len(start) + 1 and len(it) >= 2 and np.all(np.isfinite(it))
    assert np.all(np.diff(it[:, -1]) <= 0) and it[-1, -1] < it[0, -1], it[:, -1]
    assert same_bits([it[0, :-1], it[-1, :-1]], [start, end])


# ------------------------------------------------------------------ 11. refusals
@pytest.mark.parametrize("family", FORMS)
def test_refusals(gp_mod, family):
    """The 3-entry calls on an RQ handle and a wrong nh give CUGP_ERR_INVALID with the call to use; the sparse create calls
    refuse the kind; the handle's results afterwards have the bits from before."""
    L = capi.lib()
    X, y = synth(150, d=3, seed=8, scale=3.0)
    hp = [0.9, 0.5, 1.2, 0.4, 0.2, -1.0] if family == "rq_ard" else [0.9, 0.4, 0.2, -1.0]
    g = handle(gp_mod, X, y, hp, family)
    want = g.loglik_grad()
    h = g.handle
    v, ll, ne, nh, kk = np.zeros(8), C.c_double(), C.c_int(), C.c_int(), C.c_int(-1)
    p = capi.ptr(v)
    assert L.cugp_num_hyper(h, C.byref(nh)) == 0 and nh.value == len(hp)
    assert L.cugp_kernel_kind(h, C.byref(kk)) == 0 and kk.value == capi.CUGP_KERNEL_RQ
    for name, call, use in [
            ("cugp_set_loghyper", lambda: L.cugp_set_loghyper(h, p), b"cugp_set_loghyper_ard"),
            ("cugp_get_loghyper", lambda: L.cugp_get_loghyper(h, p), b"cugp_get_loghyper_ard"),
            ("cugp_loglik_grad", lambda: L.cugp_loglik_grad(h, C.byref(ll), p), b"cugp_loglik_grad_ard"),
            ("cugp_loglik_grad_fetch", lambda: L.cugp_loglik_grad_fetch(h, C.byref(ll), p), b"cugp_loglik_grad_fetch_ard"),
            ("cugp_cg_solve", lambda: L.cugp_cg_solve(h, 5, None, 0, C.byref(ne)), b"cugp_cg_solve_ard"),
            ("cugp_rprop_solve", lambda: L.cugp_rprop_solve(h, 5, None, 0, C.byref(ne)), b"cugp_cg_solve_ard")]:
        assert call() == INV, name
        msg = L.cugp_last_error()
        assert name.encode() in msg and use in msg, (name, msg)
    for bad in (3, len(hp) - 1, len(hp) + 1):
        assert L.cugp_set_loghyper_ard(h, p, bad) == INV and L.cugp_get_loghyper_ard(h, p, bad) == INV
        assert L.cugp_loglik_grad_ard(h, C.byref(ll), p, bad) == INV
        assert L.cugp_loo(h, C.byref(ll), p, bad) == INV
    out = C.c_void_p()
    for ard in (0, 1):
        assert L.cugp_sparse_create(150, 20, 3, 0, capi.CUGP_KERNEL_RQ, ard, 1e-6, 0, C.byref(out)) == INV and not out.value
    assert L.cugp_create_kernel(150, 3, 0, 0, 3, C.byref(out)) == INV and not out.value
    assert L.cugp_create_ard_kernel(150, 3, 0, 0, 3, C.byref(out)) == INV and not out.value
    again = g.loglik_grad()
    assert same_bits(again, want) and np.array_equal(g.get_loghyperparam(), hp)
    g.close()
