"""GPU tests of leave-one-out cross-validation (cugp_loo, cugp_loo_predict, cugp_cg_solve_loo).

Accuracy is held to fp64 rounding against the extended-precision truth of tests/truth_loo.py:

    err_gpu(q) <= F_LOO[family] * max(yardstick(q), 4 ulp of q's scale)

for L_LOO (relative), every gradient component (relative to max|g|), mu and logp (largest absolute error) and var (largest
absolute error, floored at 4 ulp of sf2 + sn2); the yardstick is the textbook route (GPML 5.12-5.13 with an explicit dK_j per
hyper-parameter) in fp64 through the CPU oracle's potri / potrs over the data as given and truth.permutations; F_LOO was
fixed on the CPU (tests/test_truth_loo_cpu.py, docs/ACCURACY.md), never from the GPU.  Every figure is printed before it is
asserted ("ACC <case> <quantity> err noise floor ratio"; run with -s).  Everything else is bit equality: consistency of the
three calls, determinism, the existing results of a handle that has answered a LOO call, staleness against fresh handles,
the first row of the optimiser's trace.  One process, one device; nothing outside the tree is read.

What the accuracy cases cover:
  se n65                one tile, mostly padding
  se n128               one tile, no padding
  se n257_d3            three tiles, a transposed off-diagonal tile, the 64x64 form of the product
  se n384_cond1e6       a full last tile; small kappa-dominated terms
  matern32 n65, matern52 n300_d17 (two feature chunks), ard n257_d3, matern52_ard n257_d3
  ard n300_d17          d + 2 = 19 components from one product; two feature chunks in the ARD second sweep
  se n1300_d6           11 tiles: the triangular indexing; the multi-stream evaluation in front of it
The 128x128 form of the product and its split last round only launch from 39 and 32 tile rows on (kernels.h:
TUNE_LAUUM_WM2_MAX, split_round); test_tile_forms_agree reaches them through the handle's tuning.
"""
import numpy as np
import pytest

import truth
import truth_loo as tl
from accuracy import Report
from conftest import synth
from cugp_amd import capi

pytestmark = pytest.mark.gpu
extended = pytest.mark.skipif(not truth.EXTENDED, reason="numpy.longdouble is not an extended-precision type here")

LD = truth.LD
TUNE_LAUUM_WM2_MAX = 0


@pytest.fixture(scope="module")
def gp_mod():
    import cugp_amd.gp as gp
    return gp


def make(gp_mod, family, X, y, hp, overlap=None, npad_min=0, data=True):
    """A handle of the family with hyper-parameters and (data=True) data set."""
    kernel = family if family.startswith("matern") else "se"
    g = gp_mod.Covsum(X.shape[0], X.shape[1], npad_min=npad_min, ard=family == "ard", kernel=kernel)
    if overlap is not None:
        g.set_overlap(overlap)
    if data:
        g.set_data(X, y)
    g.set_loghyperparam(hp)
    return g


def bits(*arrays):
    return [np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).copy() for a in arrays]


def same_bits(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(bits(*a), bits(*b)))


def loo_all(g):
    """Every output of the LOO calls, ready for bit comparison: (lpl, grad, mean, var, logp)."""
    lpl, gr = g.loo()
    return (np.float64(lpl), gr) + g.loo_predict()


def device_sum(logp, npad):
    """k_loo_sum's order restated in fp64: thread t adds the rows t, t + 256, ... ascending, the 64 lanes of a wave by the
    halving tree of wave_sum, the four waves as (w0 + w1) + (w2 + w3)."""
    lp = np.zeros((npad + 255) // 256 * 256)                    # (rows beyond n are zero; threads beyond npad add nothing)
    lp[: len(logp)] = logp
    s = np.zeros(256)
    for i0 in range(0, npad, 256):
        s = s + lp[i0: i0 + 256]
    w = s.reshape(4, 64).copy()
    o = 32
    while o:
        w[:, :o] = w[:, :o] + w[:, o: 2 * o]
        o //= 2
    return (w[0, 0] + w[1, 0]) + (w[2, 0] + w[3, 0])


# ------------------------------------------------------------------ 1. accuracy
@extended
@pytest.mark.parametrize("family, name", tl.CASES, ids=["%s-%s" % c for c in tl.CASES])
def test_accuracy(gp_mod, oracle, family, name):
    c = tl.case(oracle, family, name)
    cov = c["cov"]
    rep = Report("loo/%s/%s" % (family, name), cov)
    for overlap in ((True, False) if name == "n1300_d6" else (None,)):
        g = make(gp_mod, family, c["X"], c["y"], cov.hp, overlap)
        lpl, gr, mu, var, logp = loo_all(g)
        assert gr.shape == (len(cov.hp),) and mu.shape == var.shape == logp.shape == (len(c["y"]),)
        tl.hold(rep, c, lpl, gr, mu, var, logp, "nooverlap_" if overlap is False else "")
        g.close()
    rep.check()


# ------------------------------------------------------------------ 2. consistency of the three calls
@pytest.mark.parametrize("family, name", [("se", "n65"), ("se", "n257_d3"), ("ard", "n300_d17"), ("se", "n1300_d6")])
def test_consistency(gp_mod, family, name):
    X, y, _, cov = tl.inputs(family, name)
    g = make(gp_mod, family, X, y, cov.hp)
    only, none = g.loo(want_grad=False)
    assert none is None
    lpl, gr = g.loo()
    assert same_bits([only], [lpl])                            # the objective alone carries the bits of the full call
    mu, var, logp = g.loo_predict()
    assert same_bits([g.loo(want_grad=False)[0]], [lpl])
    # the per-point results are those behind lpl: its own fixed-order sum of them, restated on the host, to the bit ...
    assert same_bits([device_sum(logp, g.capacity)], [lpl])
    # ... and their sum in index order (in longdouble: the host adds no rounding of its own) to 4 ulp of |lpl|
    exact = LD(0)
    for v in logp:
        exact = exact + LD(v)
    err = float(abs(LD(lpl) - exact) / abs(exact))
    print("SUM %s %s  |lpl - sum logp| / |lpl| = %.2e  (4 ulp = %.2e)" % (family, name, err, truth.U4))
    assert err <= truth.U4
    assert mu.shape == var.shape == (len(y),) and np.all(var > 0)
    g.close()


# ------------------------------------------------------------------ 3. determinism
@pytest.mark.parametrize("family, name", [("se", "n257_d3"), ("ard", "n257_d3")])
def test_determinism(gp_mod, family, name):
    X, y, Xt, cov = tl.inputs(family, name)
    g = make(gp_mod, family, X, y, cov.hp)
    first = loo_all(g)
    for i in range(4):                                          # five calls, every one launches again
        assert same_bits(loo_all(g), first), i
    for i in range(2):                                          # interleaved with predictions
        g.compute_test_means_and_variances(None, None, Xt)
        assert same_bits(loo_all(g), first), i
    moved = np.asarray(cov.hp) + 0.25
    g.set_loghyperparam(moved)
    away = loo_all(g)
    assert not same_bits(away[:1], first[:1])
    g.set_loghyperparam(cov.hp)                                 # ... and moved back: a new evaluation, the same bits
    assert same_bits(loo_all(g), first)
    g.close()


# ------------------------------------------------------------------ 4. the existing results of the handle
def existing(g, Xt):
    """What the existing calls return, ready for bit comparison."""
    ll, gr = g.loglik_grad()
    m, v = g.compute_test_means_and_variances(None, None, Xt)
    mj, cov = g.compute_test_joint(None, None, Xt[:40])
    pm, pv, dm, dv = g.predict_grad(Xt[:40])
    return np.float64(ll), gr, m, v, mj, cov, pm, pv, dm, dv, g.get_K_inverse(), g.get_alpha()


@pytest.mark.parametrize("family, name", [("se", "n257_d3"), ("ard", "n257_d3"), ("se", "n65"), ("se", "n1300_d6")])
def test_existing_results_are_untouched(gp_mod, family, name):
    """cugp_loglik_grad, cugp_predict, cugp_predict_cov, cugp_predict_grad, cugp_get_K_inverse and cugp_get_alpha return the
    bits they returned before a LOO call: an SE and an ARD handle, a graph-replayed evaluation (n65) and a multi-stream one
    (n1300_d6)."""
    X, y, Xt, cov = tl.inputs(family, name)
    g = make(gp_mod, family, X, y, cov.hp)
    before = existing(g, Xt)
    loo_all(g)
    assert same_bits(existing(g, Xt), before)
    g.set_loghyperparam(np.asarray(cov.hp) + 0.125)             # a second evaluation of the same handle, scratch in place
    twin = make(gp_mod, family, X, y, np.asarray(cov.hp) + 0.125)
    assert same_bits(existing(g, Xt), existing(twin, Xt))
    loo_all(g)
    assert same_bits(existing(g, Xt), existing(twin, Xt))
    g.close()
    twin.close()


@pytest.mark.parametrize("family", ["se", "ard"])
@pytest.mark.parametrize("k", [1, 64])
def test_append_is_untouched_and_answers_for_all_rows(gp_mod, family, k):
    """n257_d3 with npad_min = 384, the last k rows appended to a handle that holds its inverse.  cugp_append after a LOO call
    leaves what it leaves without one (the twin never saw a LOO call before its append), and the LOO results of the
    extended handle are the twin's -- a fresh handle brought to the same rows the same way -- to the bit."""
    X, y, Xt, cov = tl.inputs(family, "n257_d3")
    n0 = len(y) - k
    hs = []
    for with_loo in (True, False):
        g = make(gp_mod, family, X[:n0], y[:n0], cov.hp, npad_min=384)
        g.loglik_grad()
        if with_loo:
            stale = loo_all(g)
        g.append(X[n0:], y[n0:])
        hs.append(g)
    g, twin = hs
    assert same_bits(existing(g, Xt), existing(twin, Xt))
    got = loo_all(g)
    assert got[2].shape == (len(y),) and not same_bits(got[:1], stale[:1])
    assert same_bits(got, loo_all(twin))
    assert same_bits(existing(g, Xt), existing(twin, Xt))
    g.close()
    twin.close()


# ------------------------------------------------------------------ 5. staleness
@pytest.mark.parametrize("family, name", [("se", "n257_d3"), ("matern52_ard", "n257_d3")])
def test_stale_handles_are_evaluated_first(gp_mod, family, name):
    X, y, _, cov = tl.inputs(family, name)
    hp2 = np.asarray(cov.hp) - 0.2
    fresh = make(gp_mod, family, X, y, hp2)
    want = loo_all(fresh)
    fresh.close()
    # new hyper-parameters without an evaluation, behind a LOO call at the old ones
    g = make(gp_mod, family, X, y, cov.hp)
    old = loo_all(g)
    g.set_loghyperparam(hp2)
    assert same_bits(loo_all(g), want) and not same_bits(old[:1], want[:1])
    # new data without an evaluation
    g.set_data(X, y[::-1].copy())
    g.set_data(X, y)
    assert same_bits(loo_all(g), want)
    g.close()
    # only cugp_loglik behind it: the factor is continued to K^-1 and alpha, as cugp_loglik_grad continues it
    a, b = make(gp_mod, family, X, y, hp2), make(gp_mod, family, X, y, hp2)
    a.compute_loglikelihood()
    b.compute_loglikelihood()
    b.loglik_grad()
    assert same_bits(loo_all(a), loo_all(b))
    a.close()
    b.close()


@pytest.mark.parametrize("k", [1, 64])
def test_append_without_an_inverse_is_a_fresh_handle(gp_mod, k):
    """n257_d3, npad_min = 384: rows appended to a handle that was never evaluated -- LOO factors all 257 rows, the bits of a
    fresh handle of 257 rows."""
    X, y, _, cov = tl.inputs("se", "n257_d3")
    n0 = len(y) - k
    g = make(gp_mod, "se", X[:n0], y[:n0], cov.hp, npad_min=384)
    g.append(X[n0:], y[n0:])
    fresh = make(gp_mod, "se", X, y, cov.hp, npad_min=384)
    assert same_bits(loo_all(g), loo_all(fresh))
    g.close()
    fresh.close()


# ------------------------------------------------------------------ 6. the tile forms of the product
@pytest.mark.parametrize("n", [1300, 4224])
def test_tile_forms_agree(gp_mod, n):
    """k_loo_product<2> (64x64 tiles; the default up to 768 tiles) against k_loo_product<4> on the same K^-1: at 1300 rows 66
    whole 128x128 tiles, at 4224 rows (33 tile rows, 561 tiles) 512 whole tiles and the 49 of the last round as 64x64
    quarters.  Every entry of P is the same sum in the same order in both forms: identical gradients."""
    X, y = synth(n, d=6, seed=3 * n + 6, scale=2.5 if n == 1300 else 6.0)
    g = make(gp_mod, "se", X, y, truth.HP_A)
    lpl2, g2 = g.loo()
    g.set_tuning(TUNE_LAUUM_WM2_MAX, 0)                          # (the evaluation is not repeated: K^-1 is the same)
    lpl4, g4 = g.loo()
    assert np.all(np.isfinite(g2)) and same_bits([lpl2, g2], [lpl4, g4])
    g.close()


# ------------------------------------------------------------------ 7. the optimiser
CG_START = 2.0          # the reference driver's start, {2, 2, 2} (train.py --hp), every entry
_SOLVES = {}


def solved(gp_mod, si128, family):
    """cg_solve_loo, budget 20, on the si128 fixture from CG_START, once per family -> (start, -lpl at the start, trace,
    end point, evaluations made)."""
    if family not in _SOLVES:
        import ctypes as C
        X, y = si128
        start = [CG_START] * (X.shape[1] if family == "ard" else 1) + [CG_START, CG_START]
        g = make(gp_mod, family, X, y, start)
        lpl0, _ = g.loo()
        tr = g.cg_solve_loo(budget=20)
        end = g.get_loghyperparam()
        # the C call itself from the same start: the row count by the NaN row behind the last one, and *nevals
        g.set_loghyperparam(start)
        raw, ne = np.full((4 * 20 + 8, len(start) + 1), 7.0), C.c_int()
        capi.check(capi.lib().cugp_cg_solve_loo(g.handle, 20, capi.ptr(raw), raw.shape[0], C.byref(ne)))
        _SOLVES[family] = (start, -lpl0, tr, end, ne.value, raw)
        g.close()
        print("CG-LOO %s objective along the trace (%d evaluations):" % (family, ne.value), " ".join("%.6f" % v for v in tr[:, -1]))
    return _SOLVES[family]


@extended
@pytest.mark.parametrize("family", ["se", "ard"])
def test_cg_solve_loo(gp_mod, si128, family):
    """The first trace row is -cugp_loo at the start, to the bit; the trace holds the iterates -- its last row is the end
    point, which stays set; the row behind the last is NaN and nothing beyond it is written; *nevals counts the evaluations
    (at most budget + 1); the end point's L_LOO, recomputed in longdouble by tests/truth_loo.py, is larger than the start's."""
    X, y = si128
    start, f0, tr, end, nevals, raw = solved(gp_mod, si128, family)
    assert tr.shape[1] == len(start) + 1 and 2 <= tr.shape[0] <= nevals <= 21
    assert np.array_equal(tr[0, :-1], np.asarray(start))
    assert same_bits([tr[0, -1]], [f0])
    assert np.all(np.isfinite(tr)) and np.array_equal(tr[-1, :-1], end)
    k = tr.shape[0]
    assert same_bits([raw[:k]], [tr]) and np.all(np.isnan(raw[k])) and np.all(raw[k + 1:] == 7.0)
    desc = truth.ARD if family == "ard" else truth.SE
    ll = [tl.truth_of(truth.Truth(X, y, desc(list(hp))), y)["ll"] for hp in (start, end)]
    print("CG-LOO %s L_LOO (truth) start %.6f end %.6f" % (family, float(ll[0]), float(ll[1])))
    assert ll[1] > ll[0]


@pytest.mark.parametrize("family", ["se", "ard"])
def test_cg_solve_loo_objective_never_increases_along_the_trace(gp_mod, si128, family):
    """Every trace row at or below the row before it.  The trace of cugp_cg_solve_loo holds the points the loop moves to,
    not its rejected line-search probes (one of which, an extrapolation, reads 4049 between 142 and 304 on this fixture)."""
    f = solved(gp_mod, si128, family)[2][:, -1]
    assert len(f) >= 2 and np.all(f[1:] <= f[:-1]) and f[-1] < f[0], f


# ------------------------------------------------------------------ 8. refusals, on the device
def test_refusals(gp_mod):
    import ctypes as C
    L = capi.lib()
    X, y, _, cov = tl.inputs("se", "n65")
    g = make(gp_mod, "se", X, y, cov.hp)
    a = make(gp_mod, "ard", X, y, cov.hp[:1] * 2 + cov.hp[1:])
    out, lpl, ne = np.zeros(8), C.c_double(7.0), C.c_int(7)

    def refused(rc, call):
        return rc == capi.CUGP_ERR_INVALID and call.encode() in L.cugp_last_error()
    assert refused(L.cugp_loo(None, C.byref(lpl), None, 3), "cugp_loo")
    assert refused(L.cugp_loo(g.handle, None, None, 3), "cugp_loo")
    assert refused(L.cugp_loo(g.handle, C.byref(lpl), capi.ptr(out), 4), "cugp_loo")           # an isotropic handle has 3
    assert refused(L.cugp_loo(a.handle, C.byref(lpl), capi.ptr(out), 3), "cugp_loo")           # this ARD handle 4
    assert refused(L.cugp_loo(a.handle, C.byref(lpl), None, 5), "cugp_loo")
    assert refused(L.cugp_loo_predict(None, capi.ptr(out), capi.ptr(out), None), "cugp_loo_predict")
    assert refused(L.cugp_loo_predict(g.handle, None, capi.ptr(out), None), "cugp_loo_predict")
    assert refused(L.cugp_cg_solve_loo(None, 5, None, 0, C.byref(ne)), "cugp_cg_solve_loo")
    for budget in (0, -1):
        assert refused(L.cugp_cg_solve_loo(g.handle, budget, None, 0, C.byref(ne)), "cugp_cg_solve_loo")
    empty = make(gp_mod, "se", X, y, cov.hp, data=False)
    assert refused(L.cugp_loo(empty.handle, C.byref(lpl), None, 3), "cugp_loo")                # no data yet
    assert (lpl.value, ne.value) == (7.0, 7) and not out.any()
    # logp is optional, and the refusals left the handles usable
    mu, var = np.empty(len(y)), np.empty(len(y))
    assert L.cugp_loo_predict(g.handle, capi.ptr(mu), capi.ptr(var), None) == capi.CUGP_OK
    assert same_bits([mu, var], g.loo_predict()[:2])
    assert a.loo()[1].shape == (4,)
    for h in (g, a, empty):
        h.close()
