"""Appending observations to a factored model on the GPU (include/cugp.h: cugp_append, cugp_capacity).

Accuracy: every case of tests/truth_append.py: CASES -- the LAST rows of a live case appended to a handle that has evaluated
the first n0 -- is held to the bound a fresh handle on all rows is held to, against the same longdouble truth:

    err <= F_APPEND[family] max(yardstick, floor)       (alpha and 64 rows of K^-1: F_SOLVE)

F_APPEND comes from the CPU stand-in of the update (tests/test_truth_append_cpu.py), never from the GPU's errors.  Every
figure is printed before it is asserted (run with -s).  The other tests are about state: what the old rows keep, what a
later evaluation sees (no stale n in a captured graph or a launch), determinism, the refusals, the not-positive-definite
path, and handles that never append.  Handles are created with npad_min = the live case's n.  One process, one device.
"""
import ctypes as C

import numpy as np
import pytest

import accuracy
import truth
import truth_append as ta
import truth_poe_modes as tpm
import truth_predict_grad as tpg
from accuracy import Report
from cugp_amd import capi
from cugp_amd.capi import ptr

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not truth.EXTENDED, reason="numpy.longdouble is not an extended-precision type here")]

LD = truth.LD
IDS = [ta.case_id(c) for c in ta.CASES]


@pytest.fixture(scope="module")
def gp_mod():
    import cugp_amd.gp as gp
    return gp


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def make(gp_mod, family, n, d, cap, hp):
    """A handle of the family for n rows with room for cap, its hyper-parameters set, no data."""
    g = gp_mod.Covsum(n, d, 0, npad_min=cap, ard=True) if family == "ard" else gp_mod.Covsum(n, d, 0, npad_min=cap, kernel=family)
    g.set_loghyperparam(hp)
    return g


def grown(gp_mod, family, X, y, hp, n0, chunks, evaluate=True):
    """cugp_append's subject: n0 rows set (and evaluated), then the chunks appended in order."""
    g = make(gp_mod, family, n0, X.shape[1], len(y), hp)
    g.set_data(X[:n0], y[:n0])
    if evaluate:
        g.loglik_grad()
    at = n0
    for k in chunks:
        if k == 1 and at % 2:
            g.append(X[at], y[at])                                   # one row as a 1-d X with a scalar y
        else:
            g.append(X[at: at + k], y[at: at + k])
        at += k
    assert g.n == at
    return g


def fresh(gp_mod, family, X, y, hp, cap=None):
    g = make(gp_mod, family, len(y), X.shape[1], cap or len(y), hp)
    g.set_data(X, y)
    return g


def dims(g):
    n, d, npad = C.c_int(), C.c_int(), C.c_int()
    capi.check(capi.lib().cugp_dims(g.handle, C.byref(n), C.byref(d), C.byref(npad)))
    return n.value, d.value, npad.value


def state(g, Xt):
    """Everything a caller can read, for bit comparisons: LL, gradient, prediction, factor (K^-1 and alpha apart)."""
    ll, gr = g.loglik_grad()
    m, v = g.compute_test_means_and_variances(None, None, Xt)
    return [np.array([ll]), gr, m, v, g.get_cholesky()]


# ------------------------------------------------------------------ 1. accuracy
@pytest.mark.parametrize("case", ta.CASES, ids=IDS)
def test_accuracy(gp_mod, oracle, case):
    """cugp_append on every case of the list: LL, gradient, means and variances at the 64 test points, alpha and 64 rows of
    K^-1 after the append against the live case's truth, at the bound of a fresh handle on all rows."""
    family, name, n0, chunks = case
    c = accuracy.live(oracle, family, name)
    X, y, Xt = c["X"], c["y"], c["Xt"]
    rep = Report("append/" + ta.case_id(case), c["cov"])
    g = grown(gp_mod, family, X, y, c["cov"].hp, n0, chunks)
    try:
        assert g.capacity >= len(y) and dims(g)[0] == len(y)
        ll, gr = g.loglik_grad()
        m, v = g.compute_test_means_and_variances(None, None, Xt)
        Ki = g.get_K_inverse()
        assert np.array_equal(Ki, Ki.T)
        ta.hold(rep, c, family, ll, gr, m, v, g.get_alpha(), Ki)
        quad, logdet = g.last_quad_logdet()                          # (what cugp_append left for cugp_last_quad_logdet)
        parts = (quad, logdet, len(y) * truth.LL_CONST)
        # (three roundings, each at most half an ulp of a partial sum, which is at most the sum of the parts' sizes)
        assert abs(ll + 0.5 * sum(parts)) <= 4 * np.spacing(sum(abs(p) for p in parts))
    finally:
        g.close()
    rep.check()


# ------------------------------------------------------------------ 2. the old rows
def test_old_rows_untouched(gp_mod):
    """cugp_append leaves the factor's old rows alone: get_cholesky()[:n0, :n0] carries the bits from before, through both
    passes of a chunk that straddles a tile boundary and a further full tile; d, the padded size and the capacity do not
    move, n grows.  (L^-1 has no accessor in the ABI: test_old_rows_of_the_inverse_untouched reads it through a prediction.
    K^-1 changes in every entry by design.)"""
    family, name, n0, chunks = ta.CASES[2]
    X, y, Xt, cov = truth.family_inputs(family, name)
    g = make(gp_mod, family, n0, X.shape[1], len(y), cov.hp)
    try:
        g.set_data(X[:n0], y[:n0])
        g.loglik_grad()
        L0, before, cap = g.get_cholesky(), dims(g), g.capacity
        assert before == (n0, X.shape[1], cap) and cap == 384
        at = n0
        for k in chunks:
            g.append(X[at: at + k], y[at: at + k])
            at += k
            L = g.get_cholesky()
            assert L.shape == (at, at) and same_bits(L[:n0, :n0], L0)
            assert not np.any(np.triu(L, 1)) and np.all(np.diag(L) > 0)
            assert dims(g) == (at, before[1], before[2]) and g.capacity == cap
    finally:
        g.close()


def test_old_rows_of_the_inverse_untouched(gp_mod):
    """The old rows of L^-1 (T) and of its transpose (U) keep their bits through cugp_append, read through a prediction:
    with W = k(Xt, X) L^-T and V = W L^-1, the variance is kss + sn2 - sum_i W_i^2 and its gradient sums V_j dk_j/dx.
    The training inputs form a chain along the first axis (unit length scale): test points at one end, the appended
    rows 42 and more length scales away at the other, so k(Xt, Xnew) = exp(-882 or less) underflows to an exact zero
    (asserted in numpy), while the new rows do correlate with their old neighbours (asserted: Q is not zero, every entry
    of K^-1 and alpha moves).  Then W_i for an old i reads only old rows of T, W_i for a new i is a sum of exact zeros,
    and V_j for an old j reads only old entries of U plus exact zeros: the variances and their gradients after the
    append carry the bits from before it if, and only if as far as these entries reach, the old rows were left alone.
    Adding exact zeros changes no bits in any order of summation.  A chunk across a tile boundary, then one more row."""
    rng = np.random.default_rng(19)
    n0, chunks, d = 127, (3, 1), 3
    n = n0 + sum(chunks)
    X = 0.3 * rng.standard_normal((n, d))
    X[:n0, 0] += np.linspace(0.0, 44.0, n0)
    X[n0:, 0] += 45.0
    y = np.sin(X[:, 0]) + 0.1 * rng.standard_normal(n)
    Xt = 0.3 * rng.standard_normal((16, d))
    hp = [0.0, 0.0, -2.0]
    r2 = ((Xt[:, None, :] - X[None, n0:, :]) ** 2).sum(-1)
    assert r2.min() > 2 * 882 and not np.any(np.exp(-0.5 * r2)), "k(Xt, Xnew) is not an exact zero"
    r2o = ((X[n0:, None, :] - X[None, :n0, :]) ** 2).sum(-1)
    assert np.exp(-0.5 * r2o).max() > 0.1, "the new rows do not correlate with the old ones"
    g = make(gp_mod, "se", n0, d, n, hp)
    try:
        g.set_data(X[:n0], y[:n0])
        g.loglik_grad()
        a0 = g.get_alpha()
        _, v0, _, dv0 = g.predict_grad(Xt)
        _, vl0 = g.predict_latent(Xt)
        # (the test's own inputs: the prior variance is 1 + sn2 = 1.018, so every test point has sum_i W_i^2 > 0.2)
        assert np.all(v0 < 0.8), "the test points are not explained by the old rows: W is (nearly) zero"
        at = n0
        for k in chunks:
            g.append(X[at: at + k], y[at: at + k])
            at += k
            _, v, _, dv = g.predict_grad(Xt)
            _, vl = g.predict_latent(Xt)
            assert same_bits(v, v0) and same_bits(dv, dv0) and same_bits(vl, vl0)
        assert not same_bits(g.get_alpha()[:n0], a0), "the append did not reach the old rows of alpha: Q is zero"
    finally:
        g.close()


# ------------------------------------------------------------------ 3. no stale n
@pytest.mark.parametrize("family", ["se", "ard"])
@pytest.mark.parametrize("name,n0,n", [("n257_d3", 127, 129), ("n1300_d6", 1290, 1300)], ids=["graph-127to129", "overlap-1290to1300"])
def test_no_stale_n_after_append(gp_mod, family, name, n0, n):
    """After cugp_append, other hyper-parameters and an ordinary evaluation: LL, gradient, predictions and the factor are
    bit-identical to a FRESH handle of the same capacity on the concatenated data -- at 129 rows through the captured graph
    (which had been captured for 127 rows), at 1300 rows with the inverse built beside the factorisation."""
    X, y, Xt, cov = truth.family_inputs(family, name)
    X, y = np.ascontiguousarray(X[:n]), np.ascontiguousarray(y[:n])
    hp2 = [h + 0.05 * (1 + i % 3) for i, h in enumerate(cov.hp)]
    g = grown(gp_mod, family, X, y, cov.hp, n0, (n - n0,))
    f = fresh(gp_mod, family, X, y, hp2)
    try:
        assert g.capacity == f.capacity
        g.set_loghyperparam(hp2)
        got, want = state(g, Xt), state(f, Xt)
        assert all(same_bits(a, b) for a, b in zip(got, want)), [same_bits(a, b) for a, b in zip(got, want)]
        assert same_bits(g.get_alpha(), f.get_alpha())
    finally:
        g.close()
        f.close()


# ------------------------------------------------------------------ 4. a stale handle
@pytest.mark.parametrize("family", ["se", "matern32"])
def test_append_to_a_stale_handle(gp_mod, family):
    """set_data, cugp_append without an evaluation in between, then evaluate: only the data grew; bit-identical to the fresh
    handle on all rows, and cugp_dims reports n0 + k.  The same after an append that follows a change of hyper-parameters."""
    _, name, n0, chunks = ta.CASES[2]
    X, y, Xt, cov = truth.family_inputs(family, name)
    g = grown(gp_mod, family, X, y, cov.hp, n0, chunks, evaluate=False)
    f = fresh(gp_mod, family, X, y, cov.hp)
    h = make(gp_mod, family, n0, X.shape[1], len(y), [p - 0.1 for p in cov.hp])
    try:
        assert dims(g)[0] == len(y) == g.n
        want = state(f, Xt)
        assert all(same_bits(a, b) for a, b in zip(state(g, Xt), want))
        h.set_data(X[:n0], y[:n0])
        h.loglik_grad()
        h.set_loghyperparam(cov.hp)                                  # the inverse it holds is for other hyper-parameters
        h.append(X[n0:], y[n0:])
        assert all(same_bits(a, b) for a, b in zip(state(h, Xt), want))
    finally:
        g.close()
        f.close()
        h.close()


# ------------------------------------------------------------------ 5. determinism
@pytest.mark.parametrize("case", [ta.CASES[2], ta.CASES[6]], ids=[IDS[2], IDS[6]])
def test_append_is_deterministic(gp_mod, case):
    """The same evaluate-and-append sequence on two handles: identical bits everywhere (fixed-order sums, no atomics)."""
    family, name, n0, chunks = case
    X, y, Xt, cov = truth.family_inputs(family, name)
    a = grown(gp_mod, family, X, y, cov.hp, n0, chunks)
    b = grown(gp_mod, family, X, y, cov.hp, n0, chunks)
    try:
        for u, w in zip(state(a, Xt) + [a.get_alpha(), a.get_K_inverse()] + list(a.predict_grad(Xt)),
                        state(b, Xt) + [b.get_alpha(), b.get_K_inverse()] + list(b.predict_grad(Xt))):
            assert same_bits(u, w)
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------ 6. the other predictions
@pytest.mark.parametrize("family", ["se", "matern52"])
def test_predictions_after_append(gp_mod, oracle, family):
    """predict_grad, predict_latent, compute_test_joint and sample_posterior on a handle grown by cugp_append, each at the
    bound its own GPU test holds a fresh handle to (tests/truth_predict_grad.py, truth_poe_modes.latent, accuracy's joint
    rows, truth.factor_bound_worst / draw_bound_worst).  The draws' factor C is recovered bit for bit from a twin grown the
    same way with all-zero targets (its alpha and mean are exactly zero, Sigma does not depend on y: both asserted)."""
    _, name, n0, chunks = ta.CASES[2]
    c = accuracy.live(oracle, family, name)
    cg = tpg.case(oracle, family, name)
    X, y, Xt, t, noise, fl = c["X"], c["y"], c["Xt"], c["t"], c["noise"], c["floor"]
    nt = len(Xt)
    rep = Report("append-predictions/%s/%s" % (family, name), c["cov"])
    g = grown(gp_mod, family, X, y, c["cov"].hp, n0, chunks)
    z = grown(gp_mod, family, X, np.zeros(len(y)), c["cov"].hp, n0, chunks)
    try:
        m, v, dm, dv = g.predict_grad(Xt)
        tpg.hold(rep, cg, dm, dv)
        mp, vp = g.compute_test_means_and_variances(None, None, Xt)
        assert same_bits(m, mp) and same_bits(v, vp)
        ml, vl = g.predict_latent(Xt)
        assert same_bits(ml, mp)
        e = truth.errors_pred(ml, vl, *tpm.latent(t, Xt))
        rep.add("latent_var", e["var"], noise["var"], fl["var"])
        for with_noise in (True, False):
            tmj, tcov = t.joint(Xt, with_noise)
            mj, cov = g.compute_test_joint(None, None, Xt, with_noise=with_noise)
            tag = "joint_noise_" if with_noise else "joint_latent_"
            rep.add(tag + "mean", np.max(np.abs(mj.astype(LD) - tmj)), noise["mean"], fl["mean"])
            rep.add(tag + "cov", np.max(np.abs(cov.astype(LD) - tcov)), noise["var"], fl["cov"])
        # draws with the noise term (jitter 0: Sigma_f is the returned covariance bit for bit)
        normals = np.random.default_rng(1000 * nt + 7).standard_normal((7, nt))
        _, cov = g.compute_test_joint(None, None, Xt, with_noise=True)
        draws = g.sample_posterior(None, None, Xt, 7, with_noise=True, jitter=0.0, normals=normals)
        m0, cov0 = z.compute_test_joint(None, None, Xt, with_noise=True)
        assert same_bits(cov0, cov), "the joint covariance depends on y"
        assert not np.any(m0) and not np.any(z.get_alpha()), "all-zero targets: alpha and the mean are not exactly zero"
        Cf = np.ascontiguousarray(z.sample_posterior(None, None, Xt, nt, with_noise=True, jitter=0.0, normals=np.eye(nt)).T)
        assert np.all(np.isfinite(Cf)) and not np.any(np.triu(Cf, 1))
        r, at, res, bnd = truth.factor_bound_worst(cov, Cf, nt + truth.POTRF_EXTRA_ULPS, 0.0)
        rep.add("draw_factor@%d,%d" % at, res, bnd, 0.0, 1)
        r, at, err, bnd = truth.draw_bound_worst(draws, mp, normals, Cf)
        rep.add("draws@%d,%d" % at, err, bnd, 0.0, 1)
    finally:
        g.close()
        z.close()
    rep.check()


# ------------------------------------------------------------------ 7. refusals
def test_refusals_leave_the_handle_usable(gp_mod):
    """Every refusal of cugp_append that needs a live handle: CUGP_ERR_INVALID with the cause in the message, dims unchanged,
    and the handle still answers with -- and re-evaluates to -- its previous bits.  (The members of a cugp_group: the next
    test.  The internal factor handle is refused too, but no call hands it out.)"""
    lib = capi.lib()
    family, name = "se", "n257_d3"
    X, y, Xt, cov = truth.family_inputs(family, name)
    n0, d = 200, X.shape[1]
    g = make(gp_mod, family, n0, d, 250, cov.hp)
    b = gp_mod.BCM.split(X[:240], y[:240], 2)
    try:
        Xn, yn = np.ascontiguousarray(X[n0: n0 + 60]), np.ascontiguousarray(y[n0: n0 + 60])

        def refused(handle, k, *words):
            assert lib.cugp_append(handle, ptr(Xn), ptr(yn), k) == capi.CUGP_ERR_INVALID
            msg = lib.cugp_last_error().decode()
            assert msg.startswith("cugp_append") and all(w in msg for w in words), msg

        refused(g.handle, 3, "cugp_set_data")                        # before any data
        g.set_data(X[:n0], y[:n0])
        before, shape = state(g, Xt), dims(g)
        assert g.capacity == 256
        refused(g.handle, 57, "capacity of 256", "npad_min")         # 200 + 57 > 256
        refused(g.handle, 0, "k must be positive")
        refused(g.handle, -5, "k must be positive")
        assert lib.cugp_append(g.handle, None, ptr(yn), 3) == capi.CUGP_ERR_INVALID
        assert lib.cugp_append(g.handle, ptr(Xn), None, 3) == capi.CUGP_ERR_INVALID
        with pytest.raises(capi.CugpError, match="capacity"):
            g.append(Xn[:57], yn[:57])
        with pytest.raises(ValueError):
            g.append(Xn[:3, :2], yn[:3])
        assert g.n == n0 and dims(g) == shape
        assert all(same_bits(u, w) for u, w in zip(state(g, Xt), before))
        g.set_targets(np.stack([y[:n0], 2 * y[:n0]], axis=1))
        refused(g.handle, 3, "targets")
        assert dims(g) == shape
        assert all(same_bits(u, w) for u, w in zip(state(g, Xt), before))
        g.set_loghyperparam([h + 0.5 for h in cov.hp])               # away and back: a fresh evaluation, the same bits
        g.loglik_grad()
        g.set_loghyperparam(cov.hp)
        assert all(same_bits(u, w) for u, w in zip(state(g, Xt), before))
        # an expert of a BCM
        b.set_BCM_log_hyperparam(cov.hp)
        ll0 = b.loglik_grad()
        e = b.expert(0)
        refused(e.handle, 1, "cugp_bcm")
        ll1 = b.loglik_grad()
        assert same_bits(ll0[0], ll1[0]) and same_bits(ll0[1], ll1[1])
    finally:
        g.close()
        b.close()


def test_group_members_are_refused(gp_mod):
    """Two stand-alone padded handles (no BCM: only the group's own mark can refuse them) given to cugp_group_create:
    cugp_append returns CUGP_ERR_INVALID naming the cugp_group, dims stay, and the group and both handles evaluate to
    their previous bits.  The mark lasts as long as the group: after cugp_group_destroy the handle takes the rows, and
    at other hyper-parameters it evaluates to the bits of a fresh handle on the concatenated data."""
    lib = capi.lib()
    lib.cugp_group_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_void_p)]
    lib.cugp_group_eval.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.cugp_group_destroy.argtypes = [C.c_void_p]
    lib.cugp_group_destroy.restype = None
    X, y, Xt, cov = truth.family_inputs("se", "n257_d3")
    n0, d = 100, X.shape[1]
    hs = [make(gp_mod, "se", n0, d, 128, cov.hp) for _ in range(2)]
    Xn, yn = np.ascontiguousarray(X[200:203]), np.ascontiguousarray(y[200:203])
    grp = C.c_void_p()
    f = None
    try:
        for i, g in enumerate(hs):
            g.set_data(X[i * n0: (i + 1) * n0], y[i * n0: (i + 1) * n0])
        before, shapes = [state(g, Xt) for g in hs], [dims(g) for g in hs]
        capi.check(lib.cugp_group_create((C.c_void_p * 2)(*[g.handle for g in hs]), 2, C.byref(grp)))

        def group_eval():
            ll, gr = (C.c_double * 2)(), (C.c_double * 6)()
            for g in hs:
                g.set_loghyperparam([h + 0.125 for h in cov.hp])     # (away and back: the group evaluates afresh)
            capi.check(lib.cugp_group_eval(grp, 1, ll, gr))
            for g in hs:
                g.set_loghyperparam(cov.hp)
            capi.check(lib.cugp_group_eval(grp, 1, ll, gr))
            return np.array(list(ll) + list(gr))
        g0 = group_eval()
        assert np.all(np.isfinite(g0))
        for g in hs:
            assert lib.cugp_append(g.handle, ptr(Xn), ptr(yn), 3) == capi.CUGP_ERR_INVALID
            msg = lib.cugp_last_error().decode()
            assert msg.startswith("cugp_append") and "cugp_group" in msg, msg
            with pytest.raises(capi.CugpError, match="cugp_group"):
                g.append(Xn, yn)
            assert g.n == n0
        assert [dims(g) for g in hs] == shapes
        assert same_bits(group_eval(), g0)
        for g, want in zip(hs, before):
            assert all(same_bits(u, w) for u, w in zip(state(g, Xt), want))
        lib.cugp_group_destroy(grp)
        grp = C.c_void_p()
        hs[0].append(Xn, yn)                                         # no group holds it any more
        assert dims(hs[0]) == (n0 + 3, d, 128) and dims(hs[1]) == shapes[1]
        hp2 = [h - 0.25 for h in cov.hp]
        f = fresh(gp_mod, "se", np.concatenate([X[:n0], Xn]), np.concatenate([y[:n0], yn]), hp2, cap=128)
        hs[0].set_loghyperparam(hp2)
        assert all(same_bits(u, w) for u, w in zip(state(hs[0], Xt), state(f, Xt)))
    finally:
        if grp.value:
            lib.cugp_group_destroy(grp)
        for g in hs + ([f] if f is not None else []):
            g.close()


# ------------------------------------------------------------------ 8. not positive definite
def test_append_not_positive_definite(gp_mod):
    """sigma_n = exp(-20) and a copy of training row 0 appended: the Schur complement is not positive definite to working
    precision.  cugp_append returns CUGP_OK with LL NaN or finite (an IEEE path, run once); the data stays extended; the
    live case's hyper-parameters and one ordinary evaluation then give the bits of a fresh handle on the same rows."""
    family, name = "se", "n65"
    X, y, Xt, cov = truth.family_inputs(family, name)
    n0 = len(y) - 1
    Xa, ya = np.concatenate([X[:n0], X[:1]]), np.concatenate([y[:n0], y[:1]])
    g = make(gp_mod, family, n0, X.shape[1], len(y), cov.hp[:2] + [-20.0])
    f = fresh(gp_mod, family, Xa, ya, cov.hp)
    try:
        g.set_data(X[:n0], y[:n0])
        g.loglik_grad()
        g.append(X[0], y[0])                                         # CUGP_OK, or this raises
        assert dims(g)[0] == n0 + 1
        ll, gr = g.loglik_grad()
        print("append of a duplicate row at sigma_n = exp(-20): LL %r" % ll)
        assert np.isnan(ll) or np.isfinite(ll)
        g.set_loghyperparam(cov.hp)
        assert all(same_bits(u, w) for u, w in zip(state(g, Xt), state(f, Xt)))
    finally:
        g.close()
        f.close()


# ------------------------------------------------------------------ 9. handles that never append
@pytest.mark.parametrize("name", ["n257_d3", "n1300_d6"])
def test_handles_that_never_append(gp_mod, name):
    """A plain handle (cugp_create's shapes: dX of n rows, no scratch of cugp_append) gives the hex of LL, gradient and
    prediction of a second plain handle, and of one whose only cugp_append was refused: nothing of the feature is on the path
    of a handle that does not use it.  (The kernels: profiles/append_isa_digest.txt.)

    What this cannot see: both handles come from this library, so a host-side change in how a handle that never appends is
    evaluated, relative to the library before cugp_append, would pass here.  Such changes are held by the suite's older
    tests against the oracle and the longdouble truth, not by a bit comparison; in particular the factor handle of the
    joint covariance, which cov_factor_handle now creates with tiles * 128 rows, is covered by the joint-covariance and
    posterior-sample tests alone."""
    X, y, Xt, cov = truth.family_inputs("se", name)

    def hexes(g):
        ll, gr = g.loglik_grad()
        m, v = g.compute_test_means_and_variances(None, None, Xt)
        return [float(ll).hex()] + [float(x).hex() for x in np.concatenate([gr, m, v])]
    a, b = gp_mod.Covsum(*X.shape), gp_mod.Covsum(*X.shape)
    try:
        for g in (a, b):
            g.set_loghyperparam(cov.hp)
            g.set_data(X, y)
        assert capi.lib().cugp_append(b.handle, ptr(X), ptr(y), 0) == capi.CUGP_ERR_INVALID
        assert a.capacity == b.capacity == -(-len(y) // 128) * 128
        ha = hexes(a)
        assert ha == hexes(b)
        a.set_loghyperparam([h + 0.25 for h in cov.hp])
        a.loglik_grad()
        a.set_loghyperparam(cov.hp)
        assert hexes(a) == ha
    finally:
        a.close()
        b.close()
