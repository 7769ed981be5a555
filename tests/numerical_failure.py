"""Builders for the tests of the not-positive-definite contract (docs/ACCURACY.md, "When the covariance cannot be
factored"; include/cugp.h: a covariance matrix that is not positive definite is no error -- results come back NaN with
CUGP_OK).

Plain numpy, no GPU import: tests/test_numerical_failure_cpu.py shows that the reference below satisfies every pattern
tests/test_gpu_numerical_failure.py asserts of the library.

  indefinite(n, p, kind, seed)   a finite symmetric matrix whose factorisation fails at pivot p and not before
  positions(n)                   the pivots worth failing at: both sides of every tile edge, the last tile, the last row
  nan_flow_cholesky(K)           the textbook factorisation in IEEE arithmetic that never raises
  same_bits_nan(a, b)            equal words, or NaN on both sides
  poison_row(X, j), poison_label(y, j)
"""
import numpy as np

MICRO, BUILD, TILE = 16, 64, 128            # chol_gfx950.h: the micro tile of panel_factor, the build tile, the MFMA tile
KINDS = ("negative", "zero", "minus_one")


def healthy(n, seed):
    """K = M M^T + n I, M standard normal: the matrices of test_gpu_parity.py::test_potrf_potri_vs_oracle."""
    M = np.random.default_rng(seed).standard_normal((n, n))
    return M @ M.T + n * np.eye(n)


def indefinite(n, p, kind="negative", seed=0, good=None, factor=None):
    """-> (K_bad, K_good), which differ in entry (p, p) alone.  good, factor: healthy(n, seed) and its fp64 factor where
    the caller has them already (a sweep over p), else computed here; K_good is returned as given, not copied.
    "negative":  K_good = healthy(n, seed); K_bad[p, p] is lower by L[p, p]^2 + 1, L the fp64 factor of K_good: the Schur
                 pivot at p is -1 against entries of order n -- far from rounding -- and every leading minor before p is
                 K_good's.
    "zero":      the identity with K_bad[p, p] = 0: every off-diagonal product is exactly zero, so the pivot at p is exactly
                 0 in any summation order.
    "minus_one": the identity with K_bad[p, p] = -1."""
    if not 0 <= p < n:
        raise ValueError("p must be a row of the matrix")
    if kind == "negative":
        good = healthy(n, seed) if good is None else good
        L = np.linalg.cholesky(good) if factor is None else factor
        bad = good.copy()
        bad[p, p] -= L[p, p] ** 2 + 1.0
    elif kind in ("zero", "minus_one"):
        good = np.eye(n)
        bad = good.copy()
        bad[p, p] = 0.0 if kind == "zero" else -1.0
    else:
        raise ValueError("kind must be one of %r" % (KINDS,))
    return bad, good


def positions(n):
    """Both sides of the 16-row micro tile, the 64-row build tile and the 128-row MFMA tile, the first row of the last
    (ragged) tile and the last row -- those that are rows of an n x n matrix, ascending, each once."""
    last_tile = TILE * (-(-n // TILE) - 1)
    cand = {0, MICRO - 1, MICRO, BUILD - 1, BUILD, TILE - 1, TILE, last_tile, n - 1}
    return sorted(p for p in cand if 0 <= p < n)


def nan_flow_cholesky(K):
    """The unblocked (left-looking, column by column) lower factor of K in fp64 under np.errstate(all="ignore"), which never
    raises.  Column j is scaled by r = 1 / sqrt(pivot), the diagonal entry included (pivot * r), as every implementation
    that multiplies by a reciprocal square root does (chol_gfx950.h: panel_factor): a negative pivot gives r = NaN, a zero
    pivot r = inf and 0 * inf = NaN on the diagonal and below it -- with a division by sqrt(pivot) instead, a zero pivot
    would leave a finite 0 on the diagonal.  NaN flows on through every later column.  The strict upper triangle is zero.
    The reference for what IEEE arithmetic alone gives."""
    A = np.array(K, dtype=np.float64)
    n = A.shape[0]
    L = np.zeros((n, n))
    with np.errstate(all="ignore"):
        for j in range(n):
            row = L[j, :j].copy()
            piv = A[j, j] - row @ row
            r = 1.0 / np.sqrt(piv)
            L[j, j] = piv * r
            if j + 1 < n:
                L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ row) * r
    return L


def schur_pivot(K, p):
    """The pivot the factorisation meets at p, K[p, p] - |L[p, :p]|^2, in numpy.longdouble."""
    A = np.asarray(K, dtype=np.float64).astype(np.longdouble)
    if p == 0:
        return A[0, 0]
    L = np.linalg.cholesky(np.asarray(K, dtype=np.float64)[:p, :p]).astype(np.longdouble)
    # forward substitution L w = K[:p, p] in longdouble
    w = np.zeros(p, dtype=np.longdouble)
    for i in range(p):
        w[i] = (A[i, p] - L[i, :i] @ w[:i]) / L[i, i]
    return A[p, p] - w @ w


def same_bits_nan(a, b):
    """The predicate of test_gpu_matern.py: equal uint64 words, or NaN on both sides (a NaN's sign and payload belong to no
    contract).  Shapes must agree."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    return bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


def same_bits(a, b):
    """Equal uint64 words everywhere (and equal shapes)."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all(a.view(np.uint64) == b.view(np.uint64)))


def all_nan(*values):
    """Every entry of every value (scalars, arrays, None skipped) is NaN."""
    return all(bool(np.all(np.isnan(np.asarray(v, dtype=np.float64)))) for v in values if v is not None)


def poison_row(X, j):
    """A copy of X with row j all NaN."""
    out = np.array(X, dtype=np.float64, copy=True)
    out[j, :] = np.nan
    return np.ascontiguousarray(out)


def poison_label(y, j):
    """A copy of y with y[j] NaN."""
    out = np.array(y, dtype=np.float64, copy=True)
    out[j] = np.nan
    return np.ascontiguousarray(out)
