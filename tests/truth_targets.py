"""The targets, the truth and the yardstick of the multi-target tests -- TEST INFRASTRUCTURE, CPU, a plain module beside
tests/truth.py and tests/accuracy.py.

m target vectors over the inputs and hyper-parameters of a live case of truth.FAMILIES share one factorisation:

  targets    Y[0] = the case's y; Y[t] = roll(y, 7 t) (1 + 0.25 t) + 0.3 N(0, 1) for t >= 1, ONE default_rng(11) drawn in
             target order -- so the first columns of a wider set are the narrower set
  truth      from the cached single-target truth of the case (accuracy.live: K^-1, L and T in longdouble; no second
             factorisation): A = K^-1 Y, LL_t = -1/2 (y_t'alpha_t + log|K| + n c), LL = sum_t LL_t in target order,
             W = m K^-1 - A A', the gradient through the family's cov.train(X)[1], the means Ks A
  yardstick  the family's own fp64 evaluator (cov.evaluator: the CPU oracle), run per target and summed in target order,
             over the data as given and truth.permutations -- truth.noise_level's procedure -- for LL, the gradient, the
             means (largest absolute error over the whole matrix) and every LL_t relative to |LL_t|
  stand-in   the fused formulation in fp64 (LAPACK Cholesky, Z = Y T', A = Z T, W = m K^-1 - A'A): its ratios
             (tests/test_truth_targets_cpu.py) ask for no factor beyond the families' existing ones
  bound      F_family max(yardstick, 4 ulp of the quantity's scale), F / F_MATERN / F_ARD of tests/truth.py as they stand
  wide       WIDE_CASES / wide_case: the same at nt > 64 test points (truth.wide_points), on the cached truth.  With a
             `subset` of the targets the yardstick and the floor of the means are taken over those targets only -- a
             maximum over fewer targets can only be smaller, so the bound only tightens -- and only `mean` is held; every
             column of an evaluation's mean matrix is still compared with the truth
  grown      standin_grown: the same formulas on the T, K^-1 and log|K| that truth_append.standin_append's bordering
             leaves (cugp_set_targets on a handle that cugp_append has grown), held to truth_append.F_APPEND
"""
import numpy as np

import accuracy
import truth
import truth_append

LD = truth.LD
U4 = truth.U4

# (family, case of the family's live cases, m): what each covers is in tests/test_gpu_targets.py
CASES = (
    ("se", "n65", 3),
    ("se", "n257_d3", 17),
    ("se", "n257_d3", 129),
    ("matern32", "n65", 17),
    ("matern52", "n300_d17", 5),
    ("ard", "n257_d3", 5),
    ("ard", "n300_d17", 3),
    ("se", "n1300_d6", 2),
    ("se", "n1", 2),                  # below one 64-row build tile: every off-diagonal sum empty,
    ("se", "n2", 3),                  # more targets than rows,
    ("se", "n2", 129),                # two target tiles over one mostly-padding tile,
    ("se", "n63", 17),
    ("matern32", "n63", 5),
    ("ard", "n63_d2", 3),
)
# the stand-in is pinned on the CPU at these (the issue's list: the cases above without the two that only add size)
STANDIN_CASES = (
    ("se", "n65", 3),
    ("se", "n257_d3", 17),
    ("se", "n257_d3", 129),
    ("se", "n384_cond1e6", 5),
    ("matern32", "n65", 17),
    ("matern52", "n300_d17", 5),
    ("ard", "n257_d3", 5),
    ("se", "n1", 2),
    ("se", "n2", 3),
    ("se", "n2", 129),
    ("se", "n63", 17),
    ("matern32", "n63", 5),
    ("ard", "n63_d2", 3),
)
# (family, case, m, nt, subset): prediction beyond one 64-row test tile.  What each reaches is in tests/test_gpu_targets.py
WIDE_CASES = (
    ("se", "n65", 3, 129, None),
    ("se", "n257_d3", 129, 257, None),
    ("se", "n515_d33", 65, 129, (0, 1, 63, 64)),
    ("ard", "n257_d3", 5, 200, None),
    ("matern52", "n300_d17", 17, 200, None),
    ("se", "n2", 3, 129, None),                      # two test tiles over two rows
)
# cugp_set_targets on a grown handle: (family, case, n0, chunks) of truth_append.CASES, m
GROWN_CASE = (("se", "n257_d3", 127, (2, 128)), 5)


def wide_id(case):
    family, name, m, nt, subset = case
    return "%s-%s-m%d-nt%d%s" % (family, name, m, nt, "-subset" if subset else "")


def held(c):
    """The quantities a case holds: all of them, or what a subset case names."""
    return c.get("held", c["cov"].quantities[:4] + ("mean", "ll_each"))


def targets(y, m):
    """-> Y [m][n], target-major."""
    y = np.asarray(y, dtype=np.float64)
    rng = np.random.default_rng(11)
    rows = [y.copy()]
    for t in range(1, m):
        rows.append(np.roll(y, 7 * t) * (1 + 0.25 * t) + 0.3 * rng.standard_normal(len(y)))
    return np.ascontiguousarray(np.stack(rows))


def truth_of(t, Y, Xt):
    """Every checked quantity in longdouble from the single-target truth t (kept: Kinv, L) -> dict(A [m][n], ll_each,
    ll, grad, mean [nt][m])."""
    Yl = np.asarray(Y, dtype=np.float64).astype(LD)
    m, n = Yl.shape
    A = truth._mm(Yl, t.Kinv)                                   # (K^-1 is symmetric: row t = K^-1 y_t)
    logdet = 2 * np.log(np.diag(t.L)).sum()
    ll_each = -LD(0.5) * ((Yl * A).sum(1) + logdet + n * LD(truth.LL_CONST))
    ll = LD(0)
    for v in ll_each:
        ll = ll + v
    W = m * t.Kinv - truth._mm(np.ascontiguousarray(A.T), A)
    _, terms = t.cov.train(t.X)
    grad = np.array(terms(W) + (t.sn2 * np.trace(W),), dtype=LD)
    return dict(A=A, ll_each=ll_each, ll=ll, grad=grad, mean=truth._mm(t.cross(Xt), np.ascontiguousarray(A.T)))


def errors(cov, tt, ll, grad, mean, ll_each):
    """Errors of one fp64 evaluation against truth_of's tt: truth.errors_ll_grad on the sums, the largest absolute error
    over the mean matrix [nt][m], and `ll_each` [m]: |LL_t - truth| / |truth| per target."""
    e = truth.errors_ll_grad(cov, ll, grad, tt["ll"], tt["grad"])
    e["mean"] = float(np.max(np.abs(np.asarray(mean).astype(LD) - tt["mean"])))
    e["ll_each"] = np.array([float(abs(LD(v) - w) / abs(w)) for v, w in zip(ll_each, tt["ll_each"])])
    return e


def yardstick(oracle, cov, X, Y, Xt, tt):
    """The family's fp64 evaluator per target, summed in target order, over the data as given and truth.permutations
    -> the largest error per quantity (`ll_each`: per target)."""
    Xe, evaluate = cov.evaluator(oracle, X, Xt)
    n = X.shape[0]

    def one(idx):
        Xp = np.ascontiguousarray(Xe[idx])
        ll, g, each, means = 0.0, 0.0, [], []
        for yt in Y:
            l, gr, mu, _ = evaluate(Xp, np.ascontiguousarray(yt[idx]))
            ll, g = ll + l, g + np.asarray(gr)
            each.append(l)
            means.append(mu)
        return errors(cov, tt, ll, g, np.stack(means, axis=1), each)
    E = list(truth._pool().map(one, truth.permutations(n)))
    out = {q: max(e[q] for e in E) for q in cov.quantities[:4] + ("mean",)}
    out["ll_each"] = np.max(np.stack([e["ll_each"] for e in E]), axis=0)
    return out


def floors(cov, tt):
    sc = truth.scales(cov, tt["ll"], tt["grad"], tt["mean"])
    fl = truth.floors(cov, sc)
    return {q: fl[q] for q in cov.quantities[:4] + ("mean",)}


_CASES = {}


def case(oracle, family, name, m):
    """Targets, truth, yardstick and floors of (family, case, m), computed once per process whichever test asks."""
    key = (family, name, m)
    if key not in _CASES:
        c = accuracy.live(oracle, family, name)
        Y = targets(c["y"], m)
        tt = truth_of(c["t"], Y, c["Xt"])
        _CASES[key] = dict(X=c["X"], y=c["y"], Y=Y, Xt=c["Xt"], cov=c["cov"], t=c["t"], tt=tt, rows=c["rows"],
                           solve=c["solve"], noise=yardstick(oracle, c["cov"], c["X"], Y, c["Xt"], tt),
                           floor=floors(c["cov"], tt))
    return _CASES[key]


def subset_yardstick(oracle, c, Y, Xt, subset):
    """Yardstick and floors over the targets `subset` of Y alone, against their own truth (truth_of on the cached
    single-target truth of the live case c: the sums LL and W are those of the subset) -> (noise, floor).  The evaluator
    runs target by target, so the mean's yardstick is a maximum over the subset's columns of what the whole set gives."""
    Ys = np.ascontiguousarray(Y[list(subset)])
    tts = truth_of(c["t"], Ys, Xt)
    return yardstick(oracle, c["cov"], c["X"], Ys, Xt, tts), floors(c["cov"], tts)


def wide_case(oracle, family, name, m, nt, subset=None):
    """case() at nt test points, the last but one a training row (truth.wide_points in the case's box), once per
    process.  The truth is truth_of on the live case's cached truth: no new factorisation.  subset (a tuple of target
    indices that contains the last two: targets() scales target t by 1 + 0.25 t, so the largest means are theirs): the
    yardstick and the floor come from those targets only and only `mean` is held."""
    key = (family, name, m, nt, subset)
    if key not in _CASES:
        c = accuracy.live(oracle, family, name)
        Y = targets(c["y"], m)
        Xt = truth.wide_points(c["X"], nt, truth.FAMILIES[family][2](name))
        tt = truth_of(c["t"], Y, Xt)
        out = dict(X=c["X"], y=c["y"], Y=Y, Xt=Xt, cov=c["cov"], t=c["t"], tt=tt, rows=c["rows"], solve=c["solve"])
        if subset is None:
            out.update(noise=yardstick(oracle, c["cov"], c["X"], Y, Xt, tt), floor=floors(c["cov"], tt))
        else:
            assert {m - 2, m - 1} <= set(subset) and len(set(subset)) == len(subset) and max(subset) < m
            noise, floor = subset_yardstick(oracle, c, Y, Xt, subset)
            assert floor["mean"] <= floors(c["cov"], tt)["mean"]
            out.update(noise=noise, floor=floor, held=("mean",), subset=subset)
        _CASES[key] = out
    return _CASES[key]


def hold(rep, c, ll, grad, mean, ll_each, tag="", F=None):
    """Adds LL, the gradient, the means and every LL_t of one evaluation to the accuracy.Report `rep` (a subset case:
    the means alone, every column of them); F: another factor than the family's."""
    e = errors(c["cov"], c["tt"], ll, grad, mean, ll_each)
    for q in c["cov"].quantities[:4] + ("mean",):
        if q in held(c):
            rep.add(tag + q, e[q], c["noise"][q], c["floor"][q], F)
    if "ll_each" not in held(c):
        return
    worst = int(np.argmax(e["ll_each"] / np.maximum(c["noise"]["ll_each"], U4)))
    rep.add(tag + "ll_each[%d]" % worst, e["ll_each"][worst], float(c["noise"]["ll_each"][worst]), U4, F)


def alpha_error(c, A):
    """alpha of every target (A [n][m] or [m][n] target-major given as rows) against the truth: the largest absolute
    error relative to the largest entry of that target's alpha (truth.solve_errors' scale), the worst over the targets."""
    tA = c["tt"]["A"]
    A = np.asarray(A).astype(LD)
    return float(np.max(np.max(np.abs(A - tA), axis=1) / np.max(np.abs(tA), axis=1)))


def standin(cov, X, Y, Xt, mutate=None):
    """The fused formulation in fp64, LAPACK / BLAS order: -> (ll, grad, mean [nt][m], ll_each, A [m][n]).
    mutate: a wrong indexing of the means' kernels, see standin_from."""
    import scipy.linalg as sl
    c = cov.fp64()
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0]
    L = np.linalg.cholesky(c.train(X)[0] + c.sn2 * np.eye(n))
    T = sl.solve_triangular(L, np.eye(n), lower=True)
    return standin_from(cov, X, Y, Xt, T, T.T @ T, 2 * np.log(np.diag(L)).sum(), mutate)


def standin_from(cov, X, Y, Xt, T, Ki, logdet, mutate=None):
    """The multi-target formulas in fp64 on a given T = L^-1, K^-1 and log|K| -> as standin.
    mutate "drop_chunk2": the means' k range stops at 512 (the second chunk of k_targets_mean is lost);
    "swap_tiles": the test rows [0, 64) and [64, 128) of the means change places (a wrong test-tile index)."""
    assert mutate in (None, "drop_chunk2", "swap_tiles")
    c = cov.fp64()
    X, Xt = np.asarray(X, dtype=np.float64), np.asarray(Xt, dtype=np.float64)
    m, n = Y.shape
    _, terms = c.train(X)
    Z = Y @ T.T
    A = Z @ T
    ll_each = -0.5 * ((Z * Z).sum(1) + logdet + n * truth.LL_CONST)
    ll = 0.0
    for v in ll_each:
        ll = ll + v
    W = m * Ki - A.T @ A
    g = np.array(terms(W) + (c.sn2 * np.trace(W),))
    Ks = c.k(Xt, X)
    mean = Ks[:, :512] @ A.T[:512] if mutate == "drop_chunk2" else Ks @ A.T
    if mutate == "swap_tiles":
        mean = np.concatenate([mean[64:128], mean[:64], mean[128:]])
    return ll, g, mean, ll_each, A


def standin_grown(cov, X, Y, Xt, n0, chunks):
    """cugp_set_targets on a handle grown by cugp_append: T, K^-1 and log|K| as truth_append.standin_append's bordering
    leaves them, fed into the multi-target formulas -> as standin."""
    T, Ki, logdet = truth_append.standin_append(cov, X, Y[0], Xt, n0, chunks, factors=True)
    return standin_from(cov, X, Y, Xt, T, Ki, logdet)


def ratios(c, ll, g, mean, each, A=None):
    """error / max(yardstick, floor) per held quantity of the case c (`ll_each`: the worst target); with A [m][n] also
    `alpha` against truth.F_SOLVE's yardstick."""
    e = errors(c["cov"], c["tt"], ll, g, mean, each)
    r = {q: e[q] / max(c["noise"][q], c["floor"][q]) for q in c["cov"].quantities[:4] + ("mean",) if q in held(c)}
    if "ll_each" in held(c):
        r["ll_each"] = float(np.max(e["ll_each"] / np.maximum(c["noise"]["ll_each"], U4)))
    if A is not None:
        r["alpha"] = alpha_error(c, A) / max(c["solve"]["alpha"], U4)
    return r


def standin_ratios(c, mutate=None):
    """Stand-in error / max(yardstick, floor) per held quantity (`ll_each`: the worst target)."""
    return ratios(c, *standin(c["cov"], c["X"], c["Y"], c["Xt"], mutate)[:4])
