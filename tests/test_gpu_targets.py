"""GPU tests of multi-target regression (cugp_set_targets and the _targets calls): m target vectors over the inputs and
hyper-parameters of one handle share its one factorisation.

Accuracy is held to fp64 rounding against the extended-precision truth of tests/truth_targets.py:

    err_gpu(q) <= F_family * max(yardstick(q), 4 ulp of q's scale)

with F, F_MATERN, F_ARD and F_SOLVE as they stand in tests/truth.py, the yardstick from the family's own fp64 evaluator
run per target and summed in target order, and the case list pinned on the CPU by tests/test_truth_targets_cpu.py -- never
from the GPU.  Every figure is printed before it is asserted ("ACC <case> <quantity> err noise floor ratio"; run with -s).
The same bound holds beyond one 64-row test tile (test_wide_accuracy), on handles padded beyond their rows
(test_padded_handle) and, with truth_append.F_APPEND, on a handle that cugp_append has grown.
Everything else is bit equality: independence of the targets from each other and of the test points from each other, the
scratch of cugp_predict_targets growing, shrinking and running without a variance, determinism, the existing single-target
results of a handle that has seen targets, staleness against fresh handles, the optimiser against the same loop driven
from Python.  One process, one device; nothing outside the tree is read.
"""
import ctypes as C

import numpy as np
import pytest

import accuracy
import golden_jobs
import truth
import truth_append as ta
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


def make(gp_mod, family, X, y, hp, overlap=None, Y=None, npad_min=0):
    """A handle of the family with data, hyper-parameters and (Y [m][n] target-major) targets set; npad_min: room for
    that many rows (identity-padded beyond n)."""
    g = gp_mod.Covsum(X.shape[0], X.shape[1], npad_min=npad_min, ard=family == "ard",
                      kernel=family if family.startswith("matern") else "se")
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
      se n1300_d6 m=2        hand-over blocks of the inverse; the inverse streams on and off
      se n1 m=2, n2 m=3, n2 m=129, n63 m=17, matern32 n63 m=5, ard n63_d2 m=3
                             below one 64-row build tile: the lower tiles of the outer product all padding, more targets
                             than rows, two target tiles over two rows"""
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


@extended
@pytest.mark.parametrize("case", tt.WIDE_CASES, ids=[tt.wide_id(c) for c in tt.WIDE_CASES])
def test_wide_accuracy(gp_mod, oracle, case):
    """Prediction beyond one 64-row test tile (k_targets_mean's grid is m64 * nt64 * split, ntpad = nt rounded to 128):
      se n65 m=3 nt=129                nt > n; nt64 = 3, one row into the third test tile; ntpad 256
      se n257_d3 m=129 nt=257          m64 = 3 x nt64 = 5; ntpad 384; mpad 256
      se n515_d33 m=65 nt=129, subset  m64 = 2 x nt64 = 3 x split = 2 (npad 640: k chunks [0, 512) and [512, 640)): all
                                       three factors of the grid above 1.  The yardstick is that of targets (0, 1, 63, 64)
                                       and only the means are held -- every column of them (tests/truth_targets.py)
      ard n257_d3 m=5 nt=200           a ragged second 128-row tile on an ARD handle
      matern52 n300_d17 m=17 nt=200    two feature chunks through k_cross at width
      se n2 m=3 nt=129                 two test tiles over two training rows
    The last test point but one is a training row.  LL, the gradient and LL_t do not depend on nt and are held again."""
    family, name, m, nt, subset = case
    c = tt.wide_case(oracle, *case)
    cov = c["cov"]
    rep = Report("%s/%s/m%d/nt%d" % (family, name, m, nt), cov)
    g = make(gp_mod, family, c["X"], c["y"], cov.hp, Y=c["Y"])
    ll, gr, each, A, mean, var = everything(g, c["Xt"])
    assert mean.shape == (nt, m) and var.shape == (nt,) and each.shape == (m,)
    tt.hold(rep, c, ll, gr, mean, each)
    v1 = g.compute_test_means_and_variances(None, None, c["Xt"])[1]
    assert same_bits([var], [v1])                      # the variance is cugp_predict's, launch for launch
    g.close()
    rep.check()


@extended
@pytest.mark.parametrize("name, m, npad_min", [("n257_d3", 17, 640), ("n65", 3, 256)])
def test_padded_handle(gp_mod, oracle, name, m, npad_min):
    """A handle with room beyond its rows (npad_min > n): identity-padded tile rows in k_targets_alpha's k ranges and in
    k_finalize_targets' sums of squares; at npad 640 k_targets_mean's second k chunk [512, 640) is nothing but padding.
    The 64 test points and the yardstick of the unpadded case, the same bound."""
    c = tt.case(oracle, "se", name, m)
    cov = c["cov"]
    rep = Report("se/%s/m%d/npad%d" % (name, m, npad_min), cov)
    g = make(gp_mod, "se", c["X"], c["y"], cov.hp, Y=c["Y"], npad_min=npad_min)
    assert g.capacity == npad_min > len(c["y"])
    ll, gr, each, A, mean, var = everything(g, c["Xt"])
    assert A.shape == (len(c["y"]), m) and mean.shape == (len(c["Xt"]), m)
    tt.hold(rep, c, ll, gr, mean, each)
    rep.add("alpha", tt.alpha_error(c, A.T), c["solve"]["alpha"], truth.U4, truth.F_SOLVE)
    assert same_bits([var], [g.compute_test_means_and_variances(None, None, c["Xt"])[1]])
    g.close()
    rep.check()


@extended
def test_targets_on_a_grown_handle(gp_mod, oracle):
    """cugp_set_targets on a handle that cugp_append has grown: 127 rows with room for 257, evaluated, (2, 128) appended as
    in truth_append.CASES, then 5 targets over all 257 rows.  LL, the gradient, LL_t and the means against the case on
    all rows with truth_append.F_APPEND in place of F (the factor and the inverse are the bordered ones; the stand-in is
    pinned by tests/test_truth_targets_cpu.py), alpha with F_SOLVE.  A further append is then refused -- targets have no
    new rows -- and leaves every result as it was, bit for bit."""
    (family, name, n0, chunks), m = tt.GROWN_CASE
    c = tt.case(oracle, family, name, m)
    X, y, Xt, cov = c["X"], c["y"], c["Xt"], c["cov"]
    rep = Report("grown/%s/%s/m%d" % (family, name, m), cov)
    g = gp_mod.Covsum(n0, X.shape[1], npad_min=len(y))
    g.set_loghyperparam(cov.hp)
    g.set_data(X[:n0], y[:n0])
    g.loglik_grad()
    at = n0
    for k in chunks:
        g.append(X[at: at + k], y[at: at + k])
        at += k
    assert g.n == at == len(y) and g.num_targets == 0
    g.set_targets(c["Y"].T)
    out = everything(g, Xt)
    ll, gr, each, A, mean, var = out
    tt.hold(rep, c, ll, gr, mean, each, F=ta.F_APPEND[family])
    rep.add("alpha", tt.alpha_error(c, A.T), c["solve"]["alpha"], truth.U4, ta.F_SOLVE)
    assert same_bits([var], [g.compute_test_means_and_variances(None, None, Xt)[1]])
    assert g.capacity >= len(y) + 1                    # (room is not what refuses the next row)
    with pytest.raises(capi.CugpError, match="targets"):
        g.append(X[0], y[0])
    assert g.n == len(y)
    assert same_bits(everything(g, Xt), out)
    g.close()
    rep.check()


# ------------------------------------------------------------------ 2. one target
@extended
@pytest.mark.parametrize("family, name", [("se", "n257_d3"), ("ard", "n257_d3"), ("matern52", "n65"), ("se", "n2")])
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
    """At 129 test points (three 64-row test tiles) and up to 129 targets (m64 = 1, 2, 3 on either side of 64 and 128):
    a target's LL_t, alpha and means carry the same bits whatever other targets stand beside it and wherever it stands."""
    X, y, _, hp = truth.live_inputs("n257_d3")
    Xw = truth.wide_points(X, 257, truth.LIVE_CASES["n257_d3"][3])
    Xt = np.ascontiguousarray(Xw[:129])
    Y = tt.targets(y, 129)
    g = make(gp_mod, "se", X, y, hp, Y=Y[:3])
    base = everything(g, Xt)

    def column(out, t):
        return out[2][t], out[3][:, t], out[4][:, t]
    for keep in ([1], [2, 0, 1], [2, 1], list(range(17)), [16, 3, 1, 0], list(range(64)), list(range(65)),
                 [128, 2, 1, 0] + list(range(3, 127)), list(range(129))):
        g.set_targets(Y[keep].T)
        assert g.num_targets == len(keep)
        out = everything(g, Xt)
        for pos, t in enumerate(keep):
            if t < 3:
                assert same_bits(column(out, pos), column(base, t)), (len(keep), t)
    # 129 targets are set: nt = 64, then 257 (the scratch grows), then 64 and 257 again (it is reused as it stands)
    p64, p257 = g.predict_targets(Xw[:64]), g.predict_targets(Xw)
    assert p257[0].shape == (257, 129) and same_bits([p257[0][:129, :3]], [base[4]])
    assert same_bits(g.predict_targets(Xw[:64]), p64)
    assert same_bits(g.predict_targets(Xw), p257)
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


def test_rows_do_not_see_each_other(gp_mod):
    """n515_d33 (two k chunks), m = 65: a test point's means carry the same bits whether it is predicted among 257 points
    or in a slice of them that starts on a 128-row tile (Xt[128:257]), inside one (Xt[65:130]), or alone (Xt[256:257]).
    Every element of the mean matrix is one sum over k per chunk, in tile_nt's order: BK columns of k at a time from the
    chunk's k0, the MFMA's fixed order inside, whichever lane and 64 x 64 tile the element falls into; the chunks
    (TARGETS_MEAN_KSTEP wide, a function of npad alone) are added in chunk order.  Neither the tile position nor nt enters."""
    X, y, _, hp = truth.live_inputs("n515_d33")
    Xt = truth.wide_points(X, 257, truth.LIVE_CASES["n515_d33"][3])
    g = make(gp_mod, "se", X, y, hp, Y=tt.targets(y, 65))
    wide, _ = g.predict_targets(Xt)
    assert wide.shape == (257, 65) and np.all(np.isfinite(wide))
    for a, b in ((128, 257), (65, 130), (256, 257)):
        part, _ = g.predict_targets(Xt[a:b])
        assert part.shape == (b - a, 65)
        assert same_bits([part], [wide[a:b]]), (a, b)
    g.close()


def test_var_is_optional(gp_mod):
    """cugp_predict_targets with var = NULL, first on a fresh handle (it sizes the scratch): CUGP_OK and the means' bits
    of the call with var, at nt = 200; the handle's cugp_predict returns its earlier bits afterwards."""
    X, y, _, hp = truth.live_inputs("n257_d3")
    m, nt = 5, 200
    Xt = truth.wide_points(X, nt, truth.LIVE_CASES["n257_d3"][3])
    L = capi.lib()
    g = make(gp_mod, "se", X, y, hp, Y=tt.targets(y, m))
    before = g.compute_test_means_and_variances(None, None, Xt)
    mean0, mean1, var1 = np.full((m, nt), np.nan), np.full((m, nt), np.nan), np.full(nt, np.nan)
    assert L.cugp_predict_targets(g.handle, capi.ptr(Xt), nt, capi.ptr(mean0), None) == capi.CUGP_OK
    assert L.cugp_predict_targets(g.handle, capi.ptr(Xt), nt, capi.ptr(mean1), capi.ptr(var1)) == capi.CUGP_OK
    assert np.all(np.isfinite(mean0)) and same_bits([mean0], [mean1])
    assert same_bits([var1], [before[1]])
    assert L.cugp_predict_targets(g.handle, capi.ptr(Xt), nt, capi.ptr(mean1), None) == capi.CUGP_OK
    assert same_bits([mean0], [mean1])
    assert same_bits(g.compute_test_means_and_variances(None, None, Xt), before)
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
