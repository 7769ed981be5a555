"""The builders of tests/numerical_failure.py, checked without a GPU: the fp64 reference alone satisfies every pattern
tests/test_gpu_numerical_failure.py asserts of the library (docs/ACCURACY.md, "When the covariance cannot be factored").
"""
import numpy as np
import pytest

import numerical_failure as nf

SIZES = (40, 200)
CASES = [(n, p) for n in SIZES for p in nf.positions(n)]


def test_positions():
    assert nf.positions(40) == [0, 15, 16, 39]
    assert nf.positions(200) == [0, 15, 16, 63, 64, 127, 128, 199]
    assert nf.positions(515) == [0, 15, 16, 63, 64, 127, 128, 512, 514]
    assert nf.positions(1300) == [0, 15, 16, 63, 64, 127, 128, 1280, 1299]
    assert nf.positions(1664) == [0, 15, 16, 63, 64, 127, 128, 1536, 1663]        # an exact multiple: the last tile is whole
    assert nf.positions(1) == [0] and nf.positions(128) == [0, 15, 16, 63, 64, 127]


@pytest.mark.parametrize("n,p", CASES)
def test_negative_pivot_is_far_from_rounding_and_fails_exactly_at_p(n, p):
    bad, good = nf.indefinite(n, p, "negative", seed=n)
    diff = np.argwhere(bad != good)
    assert diff.tolist() == [[p, p]] and np.all(np.isfinite(bad)) and np.array_equal(bad, bad.T)
    piv = nf.schur_pivot(bad, p)
    assert piv.dtype == np.longdouble and piv <= -0.5, piv
    for q in range(0, p, max(1, p // 4)):                       # every leading minor before p is the healthy matrix's
        assert nf.schur_pivot(bad, q) == nf.schur_pivot(good, q) > 0
    L, Lgood = nf.nan_flow_cholesky(bad), nf.nan_flow_cholesky(good)
    assert np.all(np.isfinite(Lgood))
    i, j = np.indices((n, n))
    failed = (i >= j) & (j >= p)
    assert np.array_equal(np.isnan(L), failed), "NaN exactly on {(i, j): i >= j >= p}"
    assert nf.same_bits(L[~failed], Lgood[~failed]), "everything else carries the healthy factor's bits"
    # what the GPU tests assert of potrf, chol_and_det and potri follows from this factor alone
    assert np.all(np.isnan(np.diag(L)[p:]))
    r0 = nf.TILE * (p // nf.TILE)
    assert nf.same_bits(L[:r0, :r0], Lgood[:r0, :r0])
    with np.errstate(all="ignore"):
        z = _forward(L, np.ones(n))
        T = _forward(L, np.eye(n))
        assert np.isnan(z @ z) and np.isnan(2.0 * np.sum(np.log(np.diag(L))))          # quad and logdet
        assert np.all(np.isnan(T.T @ T))                                                 # every entry of K^-1


def _forward(L, B):
    """L^-1 B by substitution; nothing is skipped, so NaN flows as IEEE arithmetic has it."""
    Z = np.array(B, dtype=np.float64)
    for i in range(len(Z)):
        Z[i] = (Z[i] - L[i, :i] @ Z[:i]) / L[i, i]
    return Z


@pytest.mark.parametrize("kind", ["zero", "minus_one"])
@pytest.mark.parametrize("n,p", CASES)
def test_identity_kinds(n, p, kind):
    bad, good = nf.indefinite(n, p, kind)
    assert np.array_equal(good, np.eye(n)) and np.argwhere(bad != good).tolist() == [[p, p]]
    piv = nf.schur_pivot(bad, p)
    assert piv == (0.0 if kind == "zero" else -1.0)              # exactly: every product in front of it is 0 * 0
    L = nf.nan_flow_cholesky(bad)
    assert not np.any(np.isfinite(np.diag(L)[p:])), "no finite diagonal entry from p on"
    assert np.all(np.isnan(np.diag(L)[p:])), "the reciprocal-square-root form gives NaN, not inf, on the diagonal"
    assert nf.same_bits(L[:p, :p], np.eye(p))


def test_same_bits_nan():
    a = np.array([np.nan, 0.0, 1.0])
    b = a.copy()
    b.view(np.uint64)[0] ^= 1                                     # another NaN payload
    assert nf.same_bits_nan(a, b) and not nf.same_bits(a, b)
    assert nf.same_bits_nan(-a, a[[0, 1, 2]]) is False            # -0.0 against 0.0, -1 against 1
    assert not nf.same_bits_nan(np.array([0.0]), np.array([-0.0]))
    assert not nf.same_bits_nan(np.array([np.nan]), np.array([np.inf]))
    assert not nf.same_bits_nan(np.zeros(2), np.zeros(3))
    assert nf.all_nan(np.nan, np.full(3, np.nan), None) and not nf.all_nan(np.array([np.nan, np.inf]))


def test_poison_copies():
    X, y = np.arange(12.0).reshape(4, 3), np.arange(4.0)
    Xp, yp = nf.poison_row(X, 2), nf.poison_label(y, 3)
    assert np.all(np.isfinite(X)) and np.all(np.isfinite(y))
    assert np.isnan(Xp).tolist() == [[False] * 3, [False] * 3, [True] * 3, [False] * 3]
    assert np.isnan(yp).tolist() == [False, False, False, True]
    assert Xp.flags.c_contiguous and yp.flags.c_contiguous


# ---------------------------------------------------------------------------------------- the stand-in handles under poison
# tests/standin_handles.py under the poison steps of tests/handle_sequences.py: a failure yields NaN results, never an
# exception, and the repaired stand-in is a fresh one -- what tests/test_gpu_numerical_failure.py asserts of the library.
def _standin_subject(name):
    import handle_sequences as hs
    import standin_handles as sh
    sh.ACTIVE.clear()
    sub = hs.SUBJECTS[name]
    return hs, sh, sub, sub.model()


@pytest.mark.parametrize("how", ["row0", "row_last", "hp"])
def test_standin_covsum_fails_to_nan_and_recovers(how):
    hs, sh, sub, model = _standin_subject("covsum_se_n193_poison")
    X, y = sub.rows(0, sub.n0)
    Xt = sub.points(1, 5)

    def calls(g):
        out = [g.compute_loglikelihood()]
        out += list(g.loglik_grad()) + [g.get_K_inverse(), g.get_alpha()]
        out += list(g.compute_test_means_and_variances(None, None, Xt)) + list(g.predict_grad(Xt)) + list(g.loo())
        return out

    fresh = model.create(sh)
    fresh.set_data(X, y)
    fresh.set_loghyperparam(sub.hp_of(0))
    want = calls(fresh)
    assert all(np.all(np.isfinite(v)) for v in want)
    g = model.create(sh)
    if how == "hp":
        g.set_data(X, y)
        g.set_loghyperparam(sub.hp_bad)
    else:
        g.set_data(nf.poison_row(X, 0 if how == "row0" else sub.n0 - 1), y)
        g.set_loghyperparam(sub.hp_of(0))
    assert nf.all_nan(*calls(g))
    L = g.get_cholesky()
    assert np.all(np.isnan(np.diag(L)[(0 if how != "row_last" else sub.n0 - 1):]))
    g.set_data(X, y)
    g.set_loghyperparam(sub.hp_of(0))
    assert all(nf.same_bits(a, b) for a, b in zip(calls(g), want))


@pytest.mark.parametrize("how", ["z", "x", "hp"])
def test_standin_sparse_fails_to_nan_and_recovers(how):
    hs, sh, sub, model = _standin_subject("sparse_se_poison")
    X, y, Z = model.X, model.y, model.Z
    Xt = sub.points(1, 5)

    def calls(s):
        out = [s.bound()] + list(s.bound_grad()) + list(s.bound_grad_z()) + list(s.predict(Xt)) + list(s.predict_joint(Xt))
        return out + list(s.predict_grad(Xt))

    def make(X, Z, hp):
        s = model.create(sh)
        s.set_data(X, y)
        s.set_inducing(Z)
        s.set_loghyperparam(hp)
        return s

    want = calls(make(X, Z, sub.hp_of(0)))
    assert all(np.all(np.isfinite(v)) for v in want)
    s = make(nf.poison_row(X, 299) if how == "x" else X, nf.poison_row(Z, 64) if how == "z" else Z,
             sub.hp_bad if how == "hp" else sub.hp_of(0))
    assert nf.all_nan(*calls(s))
    s.set_data(X, y)
    s.set_inducing(Z)
    s.set_loghyperparam(sub.hp_of(0))
    assert all(nf.same_bits(a, b) for a, b in zip(calls(s), want))


def test_standin_bcm_confines_a_failed_expert():
    hs, sh, sub, model = _standin_subject("bcm_se_poison")
    Xt = sub.points(1, 5)

    def make(bad=None):
        b = model.create(sh)
        for k in range(model.K):
            b.set_expert_data(k, *model.data(k, (0, 0) if k == bad else 0))
        b.set_BCM_log_hyperparam(sub.hp_of(0))
        return b

    want = make().loglik_grad_rows()
    for k in range(model.K):
        b = make(bad=k)
        ll, g, each = b.loglik_grad()
        rows = b.loglik_grad_rows()
        others = [j for j in range(model.K) if j != k]
        assert np.isnan(ll) and np.all(np.isnan(g)) and np.all(np.isnan(rows[k]))
        assert nf.same_bits(rows[others], want[others])
        assert nf.all_nan(*b.predict(Xt), *b.predict(Xt, combine="rbcm"), *b.predict_grad(Xt))
        b.set_expert_data(k, *model.data(k, 0))
        assert nf.same_bits(b.loglik_grad_rows(), want)
