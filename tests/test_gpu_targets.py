"""GPU tests of multi-target regression (cugp_set_targets and the _targets calls): m target vectors over the inputs and
hyper-parameters of one handle share its one factorisation.

Accuracy is held to fp64 rounding against the extended-precision truth of tests/truth_targets.py:

    err_gpu(q) <= F_family * max(yardstick(q), 4 ulp of q's scale)

with F, F_MATERN, F_ARD and F_SOLVE as they stand in tests/truth.py, the yardstick from the family's own fp64 evaluator
run per target and summed in target order, and the case list pinned on the CPU by tests/test_truth_targets_cpu.py -- never
from the GPU.  Every figure is printed before it is asserted ("ACC <case> <quantity> err noise floor ratio"; run with -s).
Everything else is bit equality: independence of the targets from each other, determinism, the existing single-target
results of a handle that has seen targets, staleness against fresh handles, the optimiser against the same loop driven
from Python.  One process, one device; nothing outside the tree is read.
"""
import ctypes as C

import numpy as np
import pytest

import accuracy
import golden_jobs
import truth
import truth_targets as tt
from accuracy import Report
from conftest import synth
from cugp_amd import capi

pytestmark = pytest.mark.gpu
extended = pytest.mark.skipif(not truth.EXTENDED, reason="numpy.longdouble is not an extended-precision type here")

LD = truth.LD


@pytest.fixture(scope="module")
def gp_mod():
    import cugp_amd.gp as gp
    return gp


def make(gp_mod, family, X, y, hp, overlap=None, Y=None):
    """A handle of the family with data, hyper-parameters and (Y [m][n] target-major) targets set."""
    g = gp_mod.Covsum(X.shape[0], X.shape[1], ard=family == "ard", kernel=family if family.startswith("matern") else "se")
    if overlap is not None:
        g.set_overlap(overlap)
    g.set_data(X, y)
    g.set_loghyperparam(hp)
    if Y is not None:
        g.set_targets(np.asarray(Y).T)
    return g


def everything(g, Xt):
    """Every output of the multi-target calls, ready for bit comparison: (ll, grad, ll_each, alpha [n, m], mean [nt, m], var)."""
    ll, gr, each = g.loglik_grad_targets()
    mean, var = g.predict_targets(Xt)
    return np.float64(ll), gr, each, g.get_alpha_targets(), mean, var


def same_bits(a, b):
    return all(np.array_equal(np.asarray(x).view(np.uint64), np.asarray(y).view(np.uint64)) for x, y in zip(a, b))


def single(g, Xt):
    """The existing single-target results of a handle as hex-comparable arrays."""
    ll, gr = g.loglik_grad()
    m, v = g.compute_test_means_and_variances(None, None, Xt)
    return np.float64(ll), gr, m, v, g.get_alpha()


# ------------------------------------------------------------------ 1. accuracy
@extended
@pytest.mark.parametrize("family, name, m", tt.CASES, ids=["%s-%s-m%d" % c for c in tt.CASES])
def test_accuracy(gp_mod, oracle, family, name, m):
    """LL, every LL_t, the gradient, the means and alpha of every target.  What the cases cover:
      se n65 m=3             one row into the second 64-row build tile
      se n257_d3 m=17        three ragged tiles; a second LDS chunk of 16 targets in the gradient pass
      se n257_d3 m=129       a third 64-row target tile of the products, mpad > 128
      matern32 n65 m=17, matern52 n300_d17 m=5 (two feature chunks), ard n257_d3 m=5
      ard n300_d17 m=3       two feature chunks in the ARD second sweep
      se n1300_d6 m=2        hand-over blocks of the inverse; the inverse streams on and off"""
    c = tt.case(oracle, family, name, m)
    cov = c["cov"]
    rep = Report("%s/%s/m%d" % (family, name, m), cov)
    var0 = None
    for overlap in ((True, False) if name == "n1300_d6" else (None,)):
        g = make(gp_mod, family, c["X"], c["y"], cov.hp, overlap, c["Y"])
        assert g.num_targets == m
        tag = "nooverlap_" if overlap is False else ""
        ll, gr, each, A, mean, var = everything(g, c["Xt"])
        assert gr.shape == (len(cov.hp),) and each.shape == (m,) and A.shape == (len(c["y"]), m)
        assert mean.shape == (len(c["Xt"]), m) and var.shape == (len(c["Xt"]),)
        tt.hold(rep, c, ll, gr, mean, each, tag)
        rep.add(tag + "alpha", tt.alpha_error(c, A.T), c["solve"]["alpha"], truth.U4, truth.F_SOLVE)
        v1 = g.compute_test_means_and_variances(None, None, c["Xt"])[1]
        assert same_bits([var], [v1])                  # the variance is cugp_predict's, launch for launch
        var0 = var if var0 is None else var0
        g.close()
    rep.check()


# ------------------------------------------------------------------ 2. one target
@extended
@pytest.mark.parametrize("family, name", [("se", "n257_d3"), ("ard", "n257_d3"), ("matern52", "n65")])
def test_one_target_is_the_handles_own_problem(gp_mod, oracle, family, name):
    """Y = y: log|K| is the handle's own, bit for bit; LL, the gradient and the mean meet the bound that cugp_loglik_grad
    and cugp_predict meet at that case."""
    c = accuracy.live(oracle, family, name)
    X, y, Xt, cov, t = c["X"], c["y"], c["Xt"], c["cov"], c["t"]
    g0 = make(gp_mod, family, X, y, cov.hp)
    g0.loglik_grad()
    logdet0 = g0.last_quad_logdet()[1]
    g0.close()
    g = make(gp_mod, family, X, y, cov.hp, Y=y[None, :])
    ll, gr, each = g.loglik_grad_targets()
    mean, _ = g.predict_targets(Xt)
    logdet = g.last_quad_logdet()[1]
    assert np.float64(logdet).view(np.uint64) == np.float64(logdet0).view(np.uint64)
    assert np.float64(ll).view(np.uint64) == each[0].view(np.uint64)
    rep = Report("%s/%s/m1" % (family, name), cov)
    rep.add_all("", truth.errors_ll_grad(cov, ll, gr, t.ll, t.grad), c["noise"], c["floor"])
    rep.add("mean", np.max(np.abs(mean[:, 0].astype(LD) - c["tm"])), c["noise"]["mean"], c["floor"]["mean"])
    g.close()
    rep.check()


# ------------------------------------------------------------------ 3. beyond the captured-graph sizes
def test_n3200_against_the_single_target_path(gp_mod):
    """25 tiles: launch by launch, the inverse beside the factorisation.  The sums against the library's own
    single-target path on the same handle, cugp_set_data(X, Y[t]) for each t in turn, at the project's parity tolerances."""
    n, d, m = 3200, 6, 3
    X, y = synth(n, d=d, seed=3 * n + d, scale=3.0)
    Xt = np.ascontiguousarray(truth.points(X, d, 3.0))
    Y = tt.targets(y, m)
    g = make(gp_mod, "se", X, y, truth.HP_A, Y=Y)
    ll, gr, each, A, mean, var = everything(g, Xt)
    ll1, g1 = 0.0, np.zeros(3)
    for t in range(m):
        g.set_data(X, Y[t])
        l, gt = g.loglik_grad()
        mt, vt = g.compute_test_means_and_variances(None, None, Xt)
        ll1, g1 = ll1 + l, g1 + gt
        print("N3200 target %d  LL %.17g  LL_t %.17g" % (t, l, each[t]))
        assert golden_jobs.ll_close(each[t], l)
        assert np.all(np.abs(mean[:, t] - mt) <= 1e-8 + 1e-8 * np.abs(mt))
        assert np.all(np.abs(A[:, t] - g.get_alpha()) <= 1e-8 + 1e-8 * np.abs(g.get_alpha()))
        assert same_bits([var], [vt])
    print("N3200 LL %.17g vs %.17g  grad %s vs %s" % (ll, ll1, gr, g1))
    assert golden_jobs.ll_close(ll, ll1)
    assert np.all(np.abs(gr - g1) <= 1e-6 * np.abs(g1) + 1e-9 * np.max(np.abs(g1)))
    g.close()


# ------------------------------------------------------------------ 4. independence and determinism
def test_targets_do_not_see_each_other_and_bits_repeat(gp_mod):
    X, y, Xt, hp = truth.live_inputs("n257_d3")
    Y = tt.targets(y, 17)
    g = make(gp_mod, "se", X, y, hp, Y=Y[:3])
    base = everything(g, Xt)

    def column(out, t):
        return out[2][t], out[3][:, t], out[4][:, t]
    for keep in ([1], [2, 0, 1], [2, 1], list(range(17)), [16, 3, 1, 0]):
        g.set_targets(Y[keep].T)
        out = everything(g, Xt)
        for pos, t in enumerate(keep):
            if t < 3:
                assert same_bits(column(out, pos), column(base, t)), (keep, t)
    # ten evaluations at one theta (the targets set again each time: a kept result would repeat trivially)
    g.set_targets(Y[:3].T)
    first = everything(g, Xt)
    assert same_bits(first, base)
    for _ in range(9):
        g.set_targets(Y[:3].T)
        assert same_bits(everything(g, Xt), first)
    # a changed theta, then the original one: a whole new evaluation reproduces the first bits
    g.set_loghyperparam([hp[0] + 0.1, hp[1], hp[2] - 0.2])
    other = everything(g, Xt)
    assert not np.array_equal(other[2], first[2])
    g.set_loghyperparam(hp)
    assert same_bits(everything(g, Xt), first)
    g.close()


# ------------------------------------------------------------------ 5. a zero target
@pytest.mark.parametrize("family", ["se", "ard"])
def test_zero_target(gp_mod, family):
    X, y, Xt, cov = truth.family_inputs(family, "n257_d3")
    Y = tt.targets(y, 3)
    g = make(gp_mod, family, X, y, cov.hp, Y=Y)
    full = everything(g, Xt)
    Y0 = Y.copy()
    Y0[1] = 0.0
    g.set_targets(Y0.T)
    ll, gr, each, A, mean, var = everything(g, Xt)
    assert np.all(A[:, 1] == 0.0) and np.all(mean[:, 1] == 0.0)
    logdet = g.last_quad_logdet()[1]
    want = -0.5 * (logdet + len(y) * truth.LL_CONST)
    assert abs(each[1] - want) <= 2 * np.spacing(abs(want)), (each[1], want)
    for t in (0, 2):
        assert same_bits((each[t], A[:, t], mean[:, t]), (full[2][t], full[3][:, t], full[4][:, t]))
    assert same_bits([var], [full[5]])
    g.close()


# ------------------------------------------------------------------ 6. existing behaviour
@pytest.mark.parametrize("family", ["se", "ard"])
def test_single_target_results_are_untouched(gp_mod, family):
    X, y, Xt, cov = truth.family_inputs(family, "n257_d3")
    hp2 = list(cov.hp)
    hp2[0] += 0.15
    hp2[-1] -= 0.1
    g = make(gp_mod, family, X, y, cov.hp)
    before = single(g, Xt)
    g.set_targets(tt.targets(y, 5).T)
    everything(g, Xt)
    assert same_bits(single(g, Xt), before)
    g.set_loghyperparam(hp2)
    moved = single(g, Xt)
    everything(g, Xt)
    assert same_bits(single(g, Xt), moved)
    fresh = make(gp_mod, family, X, y, hp2)           # never saw targets
    assert same_bits(moved, single(fresh, Xt))
    fresh.close()
    g.close()


# ------------------------------------------------------------------ 7. staleness
def test_results_follow_hyperparameters_data_and_targets(gp_mod):
    X, y, Xt, hp = truth.live_inputs("n257_d3")
    Y = tt.targets(y, 4)
    hp2 = [hp[0] - 0.2, hp[1] + 0.1, hp[2]]
    X2 = np.ascontiguousarray(X[::-1] * 0.9)
    Y2 = np.ascontiguousarray(Y[::-1] * 1.5)

    def fresh(Xa, hpa, Ya):
        f = make(gp_mod, "se", Xa, y, hpa, Y=Ya)
        out = everything(f, Xt)
        f.close()
        return out
    g = make(gp_mod, "se", X, y, hp, Y=Y)
    assert same_bits(everything(g, Xt), fresh(X, hp, Y))
    g.set_loghyperparam(hp2)
    mean, var = g.predict_targets(Xt)                 # the prediction first: a stale handle re-evaluates
    want = fresh(X, hp2, Y)
    assert same_bits((mean, var), want[4:])
    assert same_bits(everything(g, Xt), want)
    g.set_data(X2, y)
    assert same_bits(everything(g, Xt), fresh(X2, hp2, Y))
    g.set_targets(Y2.T)
    assert same_bits(everything(g, Xt), fresh(X2, hp2, Y2))
    g.set_targets(Y2[:2].T)                           # a second call may change m
    assert g.num_targets == 2
    assert same_bits(everything(g, Xt), fresh(X2, hp2, Y2[:2]))
    g.close()


# ------------------------------------------------------------------ 8. the optimiser
@pytest.mark.parametrize("family", ["se", "ard"])
def test_cg_solve_targets_is_the_python_driven_loop(gp_mod, family):
    X, y, _, cov = truth.family_inputs(family, "n257_d3")
    Y = tt.targets(y, 3)
    g = make(gp_mod, family, X, y, cov.hp, Y=Y)
    trace = g.cg_solve_targets(budget=15)
    end = g.get_loghyperparam()
    assert trace.shape[1] == len(cov.hp) + 1 and len(trace) >= 2
    assert trace[-1, -1] < trace[0, -1] and np.min(trace[:, -1]) < trace[0, -1]
    h = make(gp_mod, family, X, y, cov.hp, Y=Y)

    def objective(th):
        h.set_loghyperparam(th)
        ll, gr, _ = h.loglik_grad_targets()
        return -1.0 * ll, gr
    end2, trace2 = gp_mod.cg_minimize_n(objective, cov.hp, budget=15)
    assert same_bits([trace, end], [trace2, end2])
    f_end = -1.0 * g.loglik_grad_targets()[0]
    assert f_end <= trace[0, -1]
    g.close()
    h.close()


# ------------------------------------------------------------------ 9. refusals on a live handle
def test_refusals_and_the_nan_convention(gp_mod):
    X, y, Xt, hp = truth.live_inputs("n65")
    L = capi.lib()
    INV = capi.CUGP_ERR_INVALID
    out, ll, m = np.zeros(256), C.c_double(7.0), C.c_int(7)
    g = gp_mod.Covsum(X.shape[0], X.shape[1])
    Yt = tt.targets(y, 2)
    assert L.cugp_num_targets(g.handle, C.byref(m)) == capi.CUGP_OK and m.value == 0
    assert L.cugp_set_targets(g.handle, capi.ptr(Yt), 2) == INV and b"cugp_set_targets" in L.cugp_last_error()
    g.set_data(X, y)
    g.set_loghyperparam(hp)
    # evaluation, prediction, alpha and the optimiser before any targets
    assert L.cugp_loglik_grad_targets(g.handle, C.byref(ll), capi.ptr(out), 3, None) == INV
    assert b"cugp_loglik_grad_targets" in L.cugp_last_error()
    assert L.cugp_predict_targets(g.handle, capi.ptr(Xt), len(Xt), capi.ptr(out), None) == INV
    assert b"cugp_predict_targets" in L.cugp_last_error()
    assert L.cugp_get_alpha_targets(g.handle, capi.ptr(out)) == INV
    assert L.cugp_cg_solve_targets(g.handle, 3, None, 0, C.byref(m)) == INV
    g.set_targets(Yt.T)
    assert g.num_targets == 2
    for nh in (4, 5, 2):
        assert L.cugp_loglik_grad_targets(g.handle, C.byref(ll), capi.ptr(out), nh, None) == INV
        assert b"cugp_loglik_grad_targets" in L.cugp_last_error()
    assert ll.value == 7.0 and not out.any()
    a = gp_mod.Covsum(X.shape[0], X.shape[1], ard=True)
    a.set_data(X, y)
    a.set_targets(Yt.T)
    assert L.cugp_loglik_grad_targets(a.handle, C.byref(ll), capi.ptr(out), 3, None) == INV
    assert L.cugp_loglik_grad_targets(a.handle, C.byref(ll), capi.ptr(out), X.shape[1] + 2, None) == capi.CUGP_OK
    a.close()
    # a covariance that cannot be factored: NaN with CUGP_OK, the header's convention
    g.set_loghyperparam([-400.0, 0.0, 0.0])            # l^2 = exp(-800) = 0: the diagonal of K is 0 / 0
    assert np.isnan(g.loglik_grad()[0])
    ll2, gr, each = g.loglik_grad_targets()
    assert np.isnan(ll2) and np.all(np.isnan(gr)) and np.all(np.isnan(each))
    g.set_loghyperparam(hp)                           # ... and the handle recovers
    ll3, _, each3 = g.loglik_grad_targets()
    assert np.isfinite(ll3) and np.all(np.isfinite(each3))
    g.close()
