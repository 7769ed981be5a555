"""The not-positive-definite contract of include/cugp.h on the GPU: a covariance matrix that cannot be factored is no
error -- every call returns CUGP_OK (cugp_amd.capi.check raises with cugp_last_error() in the message otherwise, which
fails the test) and the results are NaN; results that do not depend on what failed keep their bits; and a repaired handle
is a fresh handle.  docs/ACCURACY.md, "When the covariance cannot be factored", has the tables.

No tolerance anywhere: every assertion is NaN-ness, finiteness or bit equality.  tests/test_numerical_failure_cpu.py shows
that the fp64 reference of tests/numerical_failure.py satisfies every pattern asserted here.

  (a) test_pivot_sweep            explicit matrices that fail at a chosen pivot, every schedule of the factorisation
  (b) test_poisoned_row / _label  a failure placed by the data, every covariance family
  (c) test_bcm_confinement        one expert of a batched launch fails: the others keep their bits
  (d) test_sparse_failure         Kuu or B of the sparse model cannot be factored
  (e) test_singular_by_duplicates the exactly singular finite K an optimiser meets: all or nothing
"""
import functools

import numpy as np
import pytest

import numerical_failure as nf
import truth
import truth_sparse
from conftest import synth

pytestmark = pytest.mark.gpu

# kernels.h TUNE_*
LAUUM_WM2, TRTRI_WM2, BORDER_WM2, PANEL, NEAR, PANEL_MIN_NT, WAVES8 = 0, 1, 4, 8, 9, 10, 22
# the six keys test_gpu_waves8.py sets: the 128x128 launches and the two-speed factorisation at 13 tiles
WIDE = {LAUUM_WM2: 0, TRTRI_WM2: 0, BORDER_WM2: 0, PANEL: 4, NEAR: 8, PANEL_MIN_NT: 0}
SCHEDULES = {"default": {}, "waves4": {**WIDE, WAVES8: 0}, "waves8": {**WIDE, WAVES8: 1}}


@pytest.fixture(scope="module")
def gp():
    import cugp_amd.gp as gp
    return gp


class tuning:
    """The process defaults of some launch-shape keys for the length of a `with` block.  What the block ends with is what
    it began with, read from the library: a handle that owns no key reports the process default of each
    (cugp_get_handle_tuning), whatever the built-in value is or whoever set it."""

    def __init__(self, keys):
        self.keys, self.before = keys, {}

    def __enter__(self):
        from cugp_amd import capi
        import cugp_amd.gp as gp
        if self.keys:
            probe = gp.Covsum(1, 1)
            try:
                self.before = {k: probe.get_tuning(k) for k in self.keys}
            finally:
                probe.close()
        for k, v in self.keys.items():
            capi.check(capi.lib().cugp_set_tuning(k, v))

    def __exit__(self, *exc):
        from cugp_amd import capi
        for k, v in self.before.items():
            capi.check(capi.lib().cugp_set_tuning(k, v))


def test_tuning_block_restores_what_it_found(gp):
    probe = gp.Covsum(1, 1)
    try:
        before = [probe.get_tuning(k) for k in range(23)]
        with tuning(SCHEDULES["waves8"]):
            assert [probe.get_tuning(k) for k in SCHEDULES["waves8"]] == list(SCHEDULES["waves8"].values())
        assert [probe.get_tuning(k) for k in range(23)] == before
    finally:
        probe.close()


# ================================================================================================ (a) the pivot sweep
# rows -> (schedules, kinds): 200 two tiles, the 64x64 forms; 515 five tiles, ragged; 1300 eleven tiles, the hand-over
# blocks of the inverse; 1664 thirteen tiles under the forced 128x128 / two-speed launches, four and eight waves
SWEEP = {200: (("default",), nf.KINDS), 515: (("default",), nf.KINDS), 1300: (("default",), ("negative",)),
         1664: (("waves4", "waves8"), ("negative",))}
SWEEP_CASES = [(n, s, kind, p) for n, (scheds, kinds) in SWEEP.items() for s in scheds for kind in kinds
               for p in nf.positions(n)]


@functools.lru_cache(maxsize=None)
def _healthy(n):
    """(nf.healthy(n, seed=n), its fp64 factor), once per size and read-only: what nf.indefinite takes over a sweep of p."""
    good = nf.healthy(n, n)
    L = np.linalg.cholesky(good)
    good.setflags(write=False)
    L.setflags(write=False)
    return good, L


def _indefinite(n, p, kind):
    if kind != "negative":
        return nf.indefinite(n, p, kind)
    good, L = _healthy(n)
    return nf.indefinite(n, p, kind, seed=n, good=good, factor=L)


_GOOD_FACTOR = {}


def _good_factor(gp, n, sched, kind):
    """potrf(K_good) under the schedule, once (read-only afterwards)."""
    key = (n, sched, "negative" if kind == "negative" else "identity")
    if key not in _GOOD_FACTOR:
        with tuning(SCHEDULES[sched]):
            L = gp.potrf(_indefinite(n, 0, kind)[1])
        L.setflags(write=False)
        _GOOD_FACTOR[key] = L
    return _GOOD_FACTOR[key]


@pytest.mark.parametrize("n,sched,kind,p", SWEEP_CASES, ids=["n%d-%s-%s-p%d" % c for c in SWEEP_CASES])
def test_pivot_sweep(gp, n, sched, kind, p):
    """A finite matrix whose pivot p is -1 (or exactly 0) after p healthy pivots:
      potrf         L[i, i] is NaN for every i >= p (pivot p is NaN; every later pivot subtracts the square of a NaN entry
                    of column p), and the whole tiles strictly before the failing one, L[:r0, :r0] with r0 = 128
                    floor(p / 128), carry the bits of potrf(K_good): a failure does not travel backwards across a tile.
                    Nothing is asserted of the rows before p inside the failing tile, nor of the strict upper triangle.
      chol_and_det  quad AND logdet are NaN (the right-hand side is all ones: quad reads a row at or beyond p)
      potri         every entry is NaN (every entry of L^-T L^-1 sums over the last row, which is at or beyond p)
    An inf where the header says NaN -- the zero pivot's 1 / sqrt(0) -- fails the same assertions."""
    bad, good = _indefinite(n, p, kind)
    Lgood = _good_factor(gp, n, sched, kind)
    with tuning(SCHEDULES[sched]):
        L = gp.potrf(bad)
        quad, logdet = gp.chol_and_det(bad, np.ones(n))
        Ki = gp.potri(bad)
    print("SWEEP n=%d %s %s p=%d: diag NaN from p on %d/%d, quad %r, logdet %r, K^-1 NaN %d/%d" % (
        n, sched, kind, p, int(np.isnan(np.diag(L)[p:]).sum()), n - p, quad, logdet, int(np.isnan(Ki).sum()), Ki.size))
    d = np.diag(L)
    assert np.all(np.isnan(d[p:])), ("diagonal not NaN at", p + np.flatnonzero(~np.isnan(d[p:]))[:8], d[p:][~np.isnan(d[p:])][:8])
    r0 = nf.TILE * (p // nf.TILE)
    assert nf.same_bits(L[:r0, :r0], Lgood[:r0, :r0]), "the failure at %d reached the tiles before row %d" % (p, r0)
    assert np.isnan(quad) and np.isnan(logdet), (quad, logdet)
    assert Ki.shape == (n, n) and np.all(np.isnan(Ki)), ("finite entries of K^-1", int((~np.isnan(Ki)).sum()),
                                                         np.argwhere(~np.isnan(Ki))[:4])


# ================================================================================================ (b) a failure placed by the data
N_B, D_B, NT_B, M_B = 300, 3, 64, 3
_HP_SE = list(truth.LIVE_CASES["n257_d3"][2])
_ARD3 = truth.ARD_CASES["n257_d3"]
_HP_ARD = list(_ARD3[2]) + [_ARD3[3], _ARD3[4]]
FAMILIES = {"se": dict(kernel="se", ard=False, hp=_HP_SE), "matern32": dict(kernel="matern32", ard=False, hp=_HP_SE),
            "matern52": dict(kernel="matern52", ard=False, hp=_HP_SE), "se_ard": dict(kernel="se", ard=True, hp=_HP_ARD),
            "matern52_ard": dict(kernel="matern52_ard", ard=False, hp=_HP_ARD)}


@functools.lru_cache(maxsize=None)
def _data_b():
    X, y = synth(N_B, d=D_B, seed=3 * N_B + D_B, scale=4.0)
    Xt = np.ascontiguousarray(truth.points(X, D_B, 4.0, NT_B))
    rng = np.random.default_rng(11)
    Y = np.ascontiguousarray(np.sin(X @ rng.standard_normal((D_B, M_B))) + 0.1 * rng.standard_normal((N_B, M_B)))
    for a in (X, y, Xt, Y):
        a.setflags(write=False)
    return X, y, Xt, Y


def _covsum(gp, family):
    f = FAMILIES[family]
    g = gp.Covsum(N_B, D_B, kernel=f["kernel"], ard=f["ard"])
    g.set_loghyperparam(f["hp"])
    return g


def covsum_calls(g, X, y, Xt, Y):
    """Every call of part (b) on the handle, in one fixed order -> [(label, value)].  set_data comes twice: the LL-only
    schedule (no inverse) runs on a stale handle and the gradient then continues from its factor -- over a NaN factor
    when it failed: read_result_row sets factor_valid whatever the row holds --; after the second set_data the combined
    evaluation runs."""
    out = []

    def add(label, r):
        out.extend(zip(label.split(), r if isinstance(r, tuple) else (r,)))

    g.set_data(X, y)
    add("ll_only", g.compute_loglikelihood())
    add("ll_cont g_cont", g.loglik_grad())
    g.set_data(X, y)
    add("ll g", g.loglik_grad())
    add("quad logdet", g.last_quad_logdet())
    add("L", g.get_cholesky())
    add("Kinv", g.get_K_inverse())
    add("alpha", g.get_alpha())
    add("mean var", g.compute_test_means_and_variances(None, None, Xt))
    add("pg_mean pg_var pg_dmean pg_dvar", g.predict_grad(Xt))
    add("jmean jcov", g.compute_test_joint(None, None, Xt))
    add("loo loo_g", g.loo())
    g.set_targets(Y)
    add("tll tg teach", g.loglik_grad_targets())
    add("tmean tvar", g.predict_targets(Xt))
    return out


_FRESH_B = {}


def _fresh_b(gp, family):
    """covsum_calls on a handle that never saw a NaN, once per family."""
    if family not in _FRESH_B:
        g = _covsum(gp, family)
        try:
            _FRESH_B[family] = covsum_calls(g, *_data_b())
        finally:
            g.close()
        assert all(np.all(np.isfinite(v)) for _, v in _FRESH_B[family]), "the healthy case itself is not finite"
    return _FRESH_B[family]


def assert_same(got, want, only=None, tag=""):
    """Bit equality of [(label, value)] lists (of the labels in `only`)."""
    assert [l for l, _ in got] == [l for l, _ in want]
    bad = [l for (l, a), (_, b) in zip(got, want) if (only is None or l in only) and not nf.same_bits(a, b)]
    assert not bad, "%s: not the bits of the healthy handle: %s" % (tag, bad)


def assert_nan(got, labels=None, tag=""):
    bad = ["%s (%d of %d entries not NaN)" % (l, int((~np.isnan(np.asarray(v, dtype=float))).sum()), np.size(v))
           for l, v in got if (labels is None or l in labels) and not nf.all_nan(v)]
    assert not bad, "%s: not NaN: %s" % (tag, bad)


# what reads K alone, not y: the factor, the inverse, every variance and covariance
Y_FREE = ("L", "Kinv", "var", "pg_var", "pg_dvar", "jcov", "tvar", "logdet")


@pytest.mark.parametrize("j", [0, 127, 128, 299])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_poisoned_row(gp, family, j):
    """Row j of X is NaN, so row and column j of K are NaN: the factorisation fails at pivot j after j healthy pivots.
    Every result of every call is NaN -- each one sums over row j of L, of K^-1 or of k(Xt, X) -- except the factor's
    rows before j.  set_data with the healthy X then gives the bits of a handle that never saw the NaN."""
    X, y, Xt, Y = _data_b()
    fresh = _fresh_b(gp, family)
    g = _covsum(gp, family)
    try:
        got = covsum_calls(g, nf.poison_row(X, j), y, Xt, Y)
        assert_nan([(l, v) for l, v in got if l != "L"], tag="%s row %d" % (family, j))
        L = dict(got)["L"]
        assert np.all(np.isnan(np.diag(L)[j:])), "the factor's diagonal from %d on" % j
        assert_same(covsum_calls(g, X, y, Xt, Y), fresh, tag="%s after the repair of row %d" % (family, j))
    finally:
        g.close()


@pytest.mark.parametrize("j", [0, 299])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_poisoned_label(gp, family, j):
    """y[j] is NaN: LL, every gradient component, alpha (every entry of K^-1 y sums over y[j]) and the predictive mean are
    NaN; the factor, K^-1, the log-determinant and every variance and covariance read no y and keep their bits."""
    X, y, Xt, Y = _data_b()
    fresh = _fresh_b(gp, family)
    g = _covsum(gp, family)
    try:
        got = covsum_calls(g, X, nf.poison_label(y, j), Xt, Y)
        assert_nan(got, ("ll_only", "ll_cont", "g_cont", "ll", "g", "quad", "alpha", "mean", "pg_mean", "pg_dmean", "jmean"),
                   tag="%s label %d" % (family, j))
        assert_same(got, fresh, only=Y_FREE, tag="%s label %d" % (family, j))
        # the targets never read the handle's own y
        assert_same(got, fresh, only=("tll", "tg", "teach", "tmean"), tag="%s label %d, targets" % (family, j))
        assert_same(covsum_calls(g, X, y, Xt, Y), fresh, tag="%s after the repair of label %d" % (family, j))
    finally:
        g.close()


# ================================================================================================ (c) confinement across experts
# "grouped": three experts of three tiles each -- the BCM pads them to one size (bcm.cpp: bcm_create's pad_to) and they
# share every launch of an evaluation (blockIdx.y = expert, per-expert partials) and of predict_grad; that the group ran
# is asserted (predict_grad_form == 2).  "apart": tile counts 2, 1 and 3 differ by more than one tile, the experts keep
# their own sizes, no group is formed and each runs on its own handle and stream (predict_grad_form == 1): the same
# assertions hold there for a simpler reason, and the case stays as the one the issue names.
SHAPES_C = {"grouped": (300, 270, 257), "apart": (130, 65, 300)}
FORM_C = {"grouped": 2, "apart": 1}
NT_C = 65
COMBINE_C = (None, "gpoe", "bcm", "rbcm")


@functools.lru_cache(maxsize=None)
def _data_c(shape):
    parts = [synth(r, d=3, seed=900 + k, scale=4.0) for k, r in enumerate(SHAPES_C[shape])]
    Xt = np.ascontiguousarray(synth(NT_C, d=3, seed=77, scale=4.0)[0])
    return parts, Xt


def _bcm(gp, shape, ard, parts):
    b = gp.BCM(list(SHAPES_C[shape]), 3, kernel="se", ard=ard)
    for k, (X, y) in enumerate(parts):
        b.set_expert_data(k, X, y)
    b.set_BCM_log_hyperparam(_HP_ARD if ard else _HP_SE)
    return b


def bcm_calls(b, Xt):
    """-> [(label, value)].  "view<k>_*": what the evaluation left in expert k -- K^-1, alpha and the expert's own prediction,
    the row it contributes to predict_partial's sums (the C ABI reduces the experts' rows to the two product-of-experts
    sums before it returns them).  "form": how predict_grad ran."""
    out = []
    K = len(b.rows)

    def add(label, r):
        out.extend(zip(label.split(), r if isinstance(r, tuple) else (r,)))

    add("ll g each", b.loglik_grad())
    add("rows", b.loglik_grad_rows())
    for k in range(K):
        e = b.expert(k)
        add("view%d_Kinv" % k, e.get_K_inverse())
        add("view%d_alpha" % k, e.get_alpha())
    add("sum_prec sum_prec_mean", b.predict_partial(Xt))
    for k in range(K):
        add("view%d_mean view%d_var" % (k, k), b.expert(k).compute_test_means_and_variances(None, None, Xt))
    for c in COMBINE_C:
        add("mean_%s var_%s" % (c, c), b.predict(Xt, combine=c))
    add("pg_mean pg_var pg_dmean pg_dvar", b.predict_grad(Xt))
    add("form", b.predict_grad_form)
    return out


_FRESH_C = {}


def _fresh_c(gp, shape, ard):
    if (shape, ard) not in _FRESH_C:
        parts, Xt = _data_c(shape)
        b = _bcm(gp, shape, ard, parts)
        try:
            _FRESH_C[shape, ard] = bcm_calls(b, Xt)
        finally:
            b.close()
        assert all(np.all(np.isfinite(v)) for _, v in _FRESH_C[shape, ard])
    return _FRESH_C[shape, ard]


@pytest.mark.parametrize("row", ["first", "last"])
@pytest.mark.parametrize("k", range(3))
@pytest.mark.parametrize("ard", [False, True], ids=["se", "se_ard"])
@pytest.mark.parametrize("shape", list(SHAPES_C))
def test_bcm_confinement(gp, shape, ard, k, row):
    """Expert k cannot be factored: the first or the last row of its X is NaN, so it fails at its first pivot or after all
    the healthy ones, part-way through the launches it shares.  The sums are NaN: LL, the gradient, both product-of-experts
    sums and every combined prediction, whatever the rule.  Row k of loglik_grad_rows is NaN; every other expert's row,
    and the K^-1, the alpha and the prediction the evaluation left in every other expert, carry the bits of the healthy
    model: a launch that runs the experts side by side keeps them apart.  set_expert_data(k, healthy) then gives a fresh
    BCM's bits.  That the experts of "grouped" did share their launches is asserted."""
    parts, Xt = _data_c(shape)
    fresh = _fresh_c(gp, shape, ard)
    bad = list(parts)
    bad[k] = (nf.poison_row(parts[k][0], 0 if row == "first" else len(parts[k][1]) - 1), parts[k][1])
    b = _bcm(gp, shape, ard, bad)
    try:
        got = bcm_calls(b, Xt)
        res, ref = dict(got), dict(fresh)
        assert res["form"] == ref["form"] == FORM_C[shape], (res["form"], ref["form"])
        others = [j for j in range(3) if j != k]
        combined = [l for l, _ in got if l.split("_")[0] in ("mean", "var", "pg")]
        mine = ["view%d_%s" % (k, q) for q in ("Kinv", "alpha", "mean", "var")]
        assert_nan(got, ["ll", "g", "sum_prec", "sum_prec_mean"] + mine + combined, tag="expert %d" % k)
        assert np.isnan(res["each"][k]) and np.all(np.isnan(res["rows"][k])), res["rows"][k]
        assert nf.same_bits(res["each"][others], ref["each"][others])
        assert nf.same_bits(res["rows"][others], ref["rows"][others]), "another expert's row of loglik_grad_rows changed"
        for j in others:
            for q in ("Kinv", "alpha", "mean", "var"):
                assert nf.same_bits(res["view%d_%s" % (j, q)], ref["view%d_%s" % (j, q)]), (j, q)
        b.set_expert_data(k, *parts[k])
        assert_same(bcm_calls(b, Xt), fresh, tag="after the repair of expert %d" % k)
    finally:
        b.close()


# ================================================================================================ (d) the sparse model
_SP = truth_sparse.CASES["se_n300_m65"]
N_D, M_D, D_D, CHUNK_D, P_D = _SP[1], _SP[2], _SP[3], _SP[4], 3
# matern52_ard runs on the same two-dimensional data: the first two length scales of matern52_ard_n257_m64, its sf, sn
_HP_M52ARD = list(truth_sparse.CASES["matern52_ard_n257_m64"][5])
SPARSE_FAMILIES = {"se": ("se", list(_SP[5])), "matern52_ard": ("matern52_ard", _HP_M52ARD[:D_D] + _HP_M52ARD[-2:])}
SPARSE_POISON = {"z0": ("Z", 0), "z64": ("Z", 64), "x0": ("X", 0), "x299": ("X", 299)}


@functools.lru_cache(maxsize=None)
def _data_d():
    X, y = synth(N_D, d=D_D, seed=3 * N_D + D_D, scale=_SP[6])
    rows = np.sort(np.random.default_rng(1000 + M_D).choice(N_D, M_D, replace=False))      # truth_sparse.inputs' Z
    Z = np.ascontiguousarray(X[rows])
    Xt = np.ascontiguousarray(truth.points(X, D_D, _SP[6], 20))
    rng = np.random.default_rng(12)
    Y = np.ascontiguousarray(np.sin(X @ rng.standard_normal((D_D, P_D))) + 0.1 * rng.standard_normal((N_D, P_D)))
    normals = rng.standard_normal((2, len(Xt)))
    return X, y, Z, Xt, Y, normals


def sparse_calls(s, Xt, Y, normals):
    out = []

    def add(label, r):
        out.extend(zip(label.split(), r if isinstance(r, tuple) else (r,)))

    add("F", s.bound())
    add("F_g g", s.bound_grad())
    add("F_z g_z gZ", s.bound_grad_z())
    add("mean var", s.predict(Xt))
    add("jmean jcov", s.predict_joint(Xt))
    add("pg_mean pg_var pg_dmean pg_dvar", s.predict_grad(Xt))
    add("draws", s.sample_posterior(Xt, 2, with_noise=True, jitter=0.0, normals=normals))
    s.set_targets(Y)
    add("tF teach", s.bound_targets())
    add("tF_g tg teach_g", s.bound_grad_targets())
    add("tF_z tg_z tgZ teach_z", s.bound_grad_z_targets())
    add("tmean tvar", s.predict_targets(Xt))
    return out


def _sparse(gp, family, X, y, Z):
    kernel, hp = SPARSE_FAMILIES[family]
    s = gp.SparseGP(N_D, M_D, D_D, kernel=kernel, chunk_rows=CHUNK_D)
    s.set_data(X, y)
    s.set_inducing(Z)
    s.set_loghyperparam(hp)
    return s


_FRESH_D = {}


def _fresh_d(gp, family):
    if family not in _FRESH_D:
        X, y, Z, Xt, Y, normals = _data_d()
        s = _sparse(gp, family, X, y, Z)
        try:
            _FRESH_D[family] = sparse_calls(s, Xt, Y, normals)
        finally:
            s.close()
        assert all(np.all(np.isfinite(v)) for _, v in _FRESH_D[family])
    return _FRESH_D[family]


@pytest.mark.parametrize("where", list(SPARSE_POISON))
@pytest.mark.parametrize("family", list(SPARSE_FAMILIES))
def test_sparse_failure(gp, family, where):
    """A NaN row of Z (row 0; row 64, the last) makes Kuu = k(Z, Z) + eps I unfactorable; a NaN row of X (row 0 in the first
    chunk; row 299 in the last, ragged one) makes P = Kuf Kfu and with it B = I + P / s2.  Either way every result of
    every call, own side and targets, is NaN with CUGP_OK; set_inducing / set_data with the healthy array then gives a
    fresh handle's bits."""
    X, y, Z, Xt, Y, normals = _data_d()
    fresh = _fresh_d(gp, family)
    which, row = SPARSE_POISON[where]
    s = _sparse(gp, family, nf.poison_row(X, row) if which == "X" else X, y, nf.poison_row(Z, row) if which == "Z" else Z)
    try:
        assert_nan(sparse_calls(s, Xt, Y, normals), tag="%s %s" % (family, where))
        if which == "X":
            s.set_data(X, y)
        else:
            s.set_inducing(Z)
        assert_same(sparse_calls(s, Xt, Y, normals), fresh, tag="%s after the repair of %s" % (family, where))
    finally:
        s.close()


# ================================================================================================ (e) the optimiser's route
def test_singular_by_duplicates(gp):
    """200 rows of which 100 are exact copies of the other 100, theta_n = -20: sf2 + s2 == sf2 in fp64, so K has finite
    entries and is exactly singular.  Rounding decides the sign of the first duplicate's pivot, so either outcome is legal
    -- but it is all or nothing: a finite LL comes with finite quad and logdet and a gradient without NaN; a NaN LL with
    NaN in every gradient entry and both scalars.  A healthy theta then gives a fresh handle's bits."""
    import math
    X0, y0 = synth(100, d=3, seed=5, scale=4.0)
    X, y = np.concatenate([X0, X0]), np.concatenate([y0, y0])
    hp_bad, hp_good = [0.9, 0.2, -20.0], [0.9, 0.2, -1.0]
    assert math.exp(2 * hp_bad[1]) + math.exp(2 * hp_bad[2]) == math.exp(2 * hp_bad[1])
    g, f = gp.Covsum(200, 3), gp.Covsum(200, 3)
    try:
        g.set_data(X, y)
        g.set_loghyperparam(hp_bad)
        assert np.all(np.isfinite(g.compute_K_train()))
        ll, gr = g.loglik_grad()
        quad, logdet = g.last_quad_logdet()
        branch = "finite" if np.isfinite(ll) else "NaN" if np.isnan(ll) else "infinite"
        print("SINGULAR branch: LL %s (%r), quad %r, logdet %r, gradient %r" % (branch, ll, quad, logdet, gr.tolist()))
        if np.isfinite(ll):
            assert np.isfinite(quad) and np.isfinite(logdet) and not np.any(np.isnan(gr)), (ll, quad, logdet, gr)
        else:
            assert np.isnan(ll) and np.isnan(quad) and np.isnan(logdet) and np.all(np.isnan(gr)), (ll, quad, logdet, gr)
        g.set_loghyperparam(hp_good)
        f.set_data(X, y)
        f.set_loghyperparam(hp_good)
        Xt = np.ascontiguousarray(X[:7] * 0.5)
        outs = [[h.loglik_grad(), h.last_quad_logdet(), (h.get_K_inverse(),),
                 h.compute_test_means_and_variances(None, None, Xt)] for h in (g, f)]
        for a, b in zip(*outs):
            assert all(nf.same_bits(u, w) for u, w in zip(a, b))
        assert np.isfinite(outs[1][0][0])
    finally:
        g.close()
        f.close()
