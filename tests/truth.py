"""Extended-precision truth for the GP hot path -- TEST INFRASTRUCTURE, CPU, numpy only.

A plain numpy.longdouble (x86 80-bit, eps 1.08e-19) restatement of the formulas of SURVEY.md / k_finalize, written
for clarity.  The inputs (fp64 data, fp64 log-hyper-parameters) are exact; everything from exp(2 theta) on is
evaluated in longdouble, so the result is some 3 digits beyond anything an fp64 implementation can deliver and can
serve as the truth its rounding error is measured against (tests/test_truth_cpu.py checks that against mpmath).

    K    = sf2 exp(-|xi - xj|^2 / (2 l^2)) + sn2 I,   l^2 = exp(2 th0), sf2 = exp(2 th1), sn2 = exp(2 th2)
    K    = L L^T (right-looking, blocked), T = L^-1, K^-1 = T^T T, alpha = K^-1 y
    LL   = -1/2 (y^T alpha + 2 sum log L_ii + n c),   c = the fp64 value of the literal 1.83787 (not log 2 pi)
    grad = (1/2 sum W o Kf o S, sum W o Kf, sn2 tr W),   W = K^-1 - alpha alpha^T, Kf = K - sn2 I, S = |xi - xj|^2 / l^2
    mean = Ks alpha, var = sf2 + sn2 - |Ks T^T|^2 per test point, cov = k(Xt, Xt) (+ sn2 I) - (Ks T^T)(Ks T^T)^T

`noise_level` is the yardstick of tests/test_gpu_accuracy.py: what the reference-order fp64 arithmetic of the CPU
oracle delivers on the very same input, as the largest error against the truth over the data as given and 7
fixed-seed row permutations of it (every checked quantity is invariant under them; the rounding is not).
`standin` is an independent, differently ordered fp64 evaluation (LAPACK / BLAS) from which the factor F of the GPU
bound is set (docs/ACCURACY.md) -- never from the GPU's own errors.
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from conftest import HP_BCM, HP_DEFAULT, HP_DENSE, synth

LD = np.longdouble
EPS_LD = float(np.finfo(LD).eps)
EXTENDED = EPS_LD < 1e-18         # False where long double is fp64 or double-double: the accuracy tests skip there
U = 2.0 ** -53                    # fp64 unit roundoff
LL_CONST = 1.83787                # the fp64 value of the literal: what k_finalize and the oracle multiply n by
NB = 64
NPERM = 7
PERM_SEED = 20240601

WORKERS = max(1, min(8, os.cpu_count() or 1))
_POOL = []


def _pool():
    """The thread pool, created on first use."""
    if not _POOL:
        _POOL.append(ThreadPoolExecutor(WORKERS))
    return _POOL[0]


def require_extended():
    assert EXTENDED, "numpy.longdouble has eps %.3g here: no extended precision to serve as truth" % EPS_LD


def _mm(A, B):
    """A @ B in longdouble, row blocks of A on a few threads (numpy's longdouble product is a plain loop that
    releases the GIL; every output entry is the same dot product whatever the split, so the bits do not depend on it)."""
    m = A.shape[0]
    if m * A.shape[1] * B.shape[1] < 1 << 22:
        return A @ B
    out = np.empty((m, B.shape[1]), dtype=LD)
    step = max(16, -(-m // (4 * WORKERS)))

    def job(r):
        out[r: r + step] = A[r: r + step] @ B
    list(_pool().map(job, range(0, m, step)))
    return out


def hyper(hp):
    """(l^2, sf2, sn2) in longdouble from the fp64 log-hyper-parameters."""
    return tuple(np.exp(2 * LD(float(h))) for h in hp)


def sqdist(A, B):
    """|a_i - b_j|^2 in longdouble, one feature at a time (no n x n x d temporary)."""
    A, B = np.asarray(A, dtype=LD), np.asarray(B, dtype=LD)
    S = np.zeros((A.shape[0], B.shape[0]), dtype=LD)
    for k in range(A.shape[1]):
        D = A[:, k][:, None] - B[:, k][None, :]
        S += D * D
    return S


def cholesky(A):
    """Lower factor, right-looking: unblocked inside a panel of NB columns, one product per trailing update."""
    A = np.array(A, dtype=LD)
    n = A.shape[0]
    for k in range(0, n, NB):
        e = min(k + NB, n)
        for j in range(k, e):
            if not A[j, j] > 0:
                raise np.linalg.LinAlgError("not positive definite at column %d" % j)
            A[j, j] = np.sqrt(A[j, j])
            A[j + 1:, j] /= A[j, j]
            A[j + 1:, j + 1: e] -= np.outer(A[j + 1:, j], A[j + 1: e, j])
        if e < n:
            P = A[e:, k: e]
            A[e:, e:] -= _mm(P, np.ascontiguousarray(P.T))
    return np.tril(A)


def tri_inverse(L):
    """T = L^-1 (lower), block rows: the diagonal block by substitution, the rest as two products."""
    n = L.shape[0]
    T = np.zeros_like(L)
    for k in range(0, n, NB):
        e = min(k + NB, n)
        D = np.zeros((e - k, e - k), dtype=LD)
        for i in range(e - k):
            D[i, i] = 1 / L[k + i, k + i]
            D[i, :i] = -(L[k + i, k: k + i] @ D[:i, :i]) / L[k + i, k + i]
        T[k: e, k: e] = D
        if k:
            T[k: e, :k] = -(D @ _mm(L[k: e, :k], T[:k, :k]))
    return T


def gram_lower(T):
    """T^T T for lower-triangular T, column block by column block (rows above the block are zero)."""
    n = T.shape[0]
    out = np.empty((n, n), dtype=LD)
    for k in range(0, n, 4 * NB):
        e = min(k + 4 * NB, n)
        out[:, k: e] = _mm(np.ascontiguousarray(T[k:, :].T), T[k:, k: e])
    return out


class Truth:
    """Every checked quantity of one expert, in longdouble.  Attributes: n, l2, sf2, sn2, K, L, T (= L^-1), Kinv,
    alpha, ll, grad[3]; predict(Xt) / joint(Xt, with_noise) for the test points."""

    def __init__(self, X, y, hp, keep=True):
        require_extended()
        X = np.asarray(X, dtype=np.float64)
        self.X = X.astype(LD)
        yl = np.asarray(y, dtype=np.float64).astype(LD)
        n = self.n = X.shape[0]
        self.l2, self.sf2, self.sn2 = hyper(hp)
        S = sqdist(self.X, self.X) / self.l2
        Kf = self.sf2 * np.exp(-S / 2)
        K = Kf.copy()
        K[np.arange(n), np.arange(n)] += self.sn2
        L = cholesky(K)
        T = tri_inverse(L)
        Kinv = gram_lower(T)
        alpha = Kinv @ yl
        self.ll = -LD(0.5) * (yl @ alpha + 2 * np.log(np.diag(L)).sum() + n * LD(LL_CONST))
        W = Kinv - np.outer(alpha, alpha)
        WK = W * Kf
        self.grad = np.array([(WK * S).sum() / 2, WK.sum(), self.sn2 * np.trace(W)], dtype=LD)
        self.alpha, self.T = alpha, T
        if keep:
            self.K, self.L, self.Kinv = K, L, Kinv

    def _cross(self, Xt):
        Xt = np.asarray(Xt, dtype=np.float64).reshape(-1, self.X.shape[1]).astype(LD)
        Ks = self.sf2 * np.exp(-sqdist(Xt, self.X) / self.l2 / 2)
        return Xt, Ks, _mm(Ks, np.ascontiguousarray(self.T.T))

    def predict(self, Xt):
        _, Ks, Wt = self._cross(Xt)
        return Ks @ self.alpha, self.sf2 + self.sn2 - (Wt * Wt).sum(1)

    def joint(self, Xt, with_noise=True):
        Xt, Ks, Wt = self._cross(Xt)
        cov = self.sf2 * np.exp(-sqdist(Xt, Xt) / self.l2 / 2) - Wt @ Wt.T
        if with_noise:
            cov[np.arange(len(cov)), np.arange(len(cov))] += self.sn2
        return Ks @ self.alpha, cov


def bcm_rows(N, K):
    """Row partition of the reference's BCM constructor, as cugp_bcm_create_split: K - 1 parts of N // K rows, the
    last takes the rest.  -> [(offset, rows)]."""
    part = N // K
    return [(k * part, part if k < K - 1 else N - part * (K - 1)) for k in range(K)]


def bcm_truth(X, y, hp, K, Xt):
    """Product of experts over the row split: -> dict(ll, grad, mean, var): LL and gradient summed over the experts,
    var = 1 / sum 1/v_k, mean = var * sum m_k / v_k."""
    ll, grad, sp, spm = LD(0), np.zeros(3, dtype=LD), 0, 0
    for off, rows in bcm_rows(len(y), K):
        t = Truth(X[off: off + rows], y[off: off + rows], hp, keep=False)
        m, v = t.predict(Xt)
        ll, grad, sp, spm = ll + t.ll, grad + t.grad, sp + 1 / v, spm + m / v
    return dict(ll=ll, grad=grad, mean=spm / sp, var=1 / sp)


def potrf_residual_rows(K64, L64, rows):
    """For each chosen row i: (|K[i, :i+1] - L[i, :] L[:i+1, :]^T|, |L[i, :]| |L[:i+1, :]|^T) in longdouble -- the two
    sides of the componentwise bound on a computed Cholesky factor, O(n^2) per row, no full product."""
    Ll = np.asarray(L64).astype(LD)
    La = np.abs(Ll)

    def one(i):
        return (np.abs(K64[i, : i + 1].astype(LD) - Ll[: i + 1, : i + 1] @ Ll[i, : i + 1]),
                La[: i + 1, : i + 1] @ La[i, : i + 1])
    out = list(_pool().map(one, rows))
    return [o[0] for o in out], [o[1] for o in out]


def gamma(k):
    """Higham's gamma_k = k u / (1 - k u), u = 2^-53."""
    return k * U / (1 - k * U)


# ---------------------------------------------------------------------------------------- errors and the yardstick
QUANTITIES = ("ll", "g0", "g1", "g2", "mean", "var")
SOLVE_QUANTITIES = ("alpha", "kinv")


def scales(hp, ll, grad, mean):
    """The size each quantity's error is taken relative to / floored at: |LL|, max|g|, max|mean|, sf2 + sn2."""
    gs = float(np.max(np.abs(grad)))
    sv = float(np.exp(2 * hp[1]) + np.exp(2 * hp[2]))
    return dict(ll=float(abs(ll)), g0=gs, g1=gs, g2=gs, mean=float(np.max(np.abs(mean))), var=sv, cov=sv)


def errors_ll_grad(ll, grad, tll, tgrad):
    """LL relative to |LL|, each gradient component relative to max|g|; differences are taken in longdouble."""
    gs = np.max(np.abs(tgrad))
    e = dict(ll=abs(LD(ll) - tll) / abs(tll))
    for k in range(3):
        e["g%d" % k] = abs(LD(grad[k]) - tgrad[k]) / gs
    return {k: float(v) for k, v in e.items()}


def errors_pred(mean, var, tmean, tvar):
    """Means and variances: the largest absolute error."""
    return dict(mean=float(np.max(np.abs(np.asarray(mean).astype(LD) - tmean))),
                var=float(np.max(np.abs(np.asarray(var).astype(LD) - tvar))))


def errors(ll, grad, mean, var, tll, tgrad, tmean, tvar):
    """Errors of one fp64 evaluation against the truth, per quantity of QUANTITIES."""
    return dict(errors_ll_grad(ll, grad, tll, tgrad), **errors_pred(mean, var, tmean, tvar))


def floors(sc):
    """4 ulp of each quantity's scale, in the units of `errors` (LL and gradient are already relative)."""
    u4 = 4 * 2.0 ** -52
    return dict(ll=u4, g0=u4, g1=u4, g2=u4, mean=u4 * sc["mean"], var=u4 * sc["var"], cov=u4 * sc["cov"])


def permutations(n, parts=None):
    """The data as given, then NPERM fixed-seed row permutations; with `parts` [(offset, rows)] the rows move inside
    their own part only (a BCM's experts keep their rows)."""
    rng = np.random.default_rng(PERM_SEED)
    parts = parts or [(0, n)]
    return [np.arange(n)] + [np.concatenate([off + rng.permutation(r) for off, r in parts]) for _ in range(NPERM)]


def noise_level(oracle, X, y, hp, Xt, tll, tgrad, tmean, tvar, evaluate=None, parts=None):
    """-> (noise, first, rest): per quantity, the largest error of the fp64 oracle against the truth over the data as
    given and NPERM row permutations, the error on the data as given alone, the largest over the permutations alone.  `evaluate(X, y) -> (ll, grad, mean, var)`
    replaces the single-expert oracle and `parts` keeps the rows inside their expert (the BCM case)."""
    if evaluate is None:
        def evaluate(Xp, yp):
            ll, g = oracle.loglik_grad(Xp, yp, hp)
            return (ll, g) + tuple(oracle.predict(Xp, yp, hp, Xt))
    def one(idx):
        return errors(*evaluate(np.ascontiguousarray(X[idx]), np.ascontiguousarray(y[idx])), tll, tgrad, tmean, tvar)
    E = list(_pool().map(one, permutations(len(y), parts)))       # the oracle is serial C behind ctypes: one thread each
    return {q: max(e[q] for e in E) for q in QUANTITIES}, E[0], {q: max(e[q] for e in E[1:]) for q in QUANTITIES}


def noise_level_solve(oracle, X, y, hp, t, rows):
    """The same yardstick for alpha and for the chosen rows of K^-1 (largest absolute error relative to the largest
    entry), from the oracle's potri / potrs on its own K, on the data as given and under the permutations."""
    n = len(y)
    ta, tk = t.alpha, t.Kinv[rows]
    kmax = np.max(np.abs(t.Kinv))

    def one(idx):
        inv = np.empty(n, dtype=np.int64)
        inv[idx] = np.arange(n)
        Kp = oracle.K_train(np.ascontiguousarray(X[idx]), hp)
        a = oracle.Kinvy(Kp, np.ascontiguousarray(y[idx]))[inv]
        Ki = oracle.K_inverse(Kp)[np.ix_(inv[rows], inv)]
        return (float(np.max(np.abs(a.astype(LD) - ta)) / np.max(np.abs(ta))),
                float(np.max(np.abs(Ki.astype(LD) - tk)) / kmax))
    E = list(_pool().map(one, permutations(n)))
    return dict(alpha=max(e[0] for e in E), kinv=max(e[1] for e in E))


def standin(X, y, hp, Xt, solve=False):
    """The same quantities from an independent fp64 implementation in another order: LAPACK's blocked Cholesky, a
    triangular solve against I, BLAS products (blocked, FMA-contracted -- as the MFMA path is).
    -> (ll, grad, mean, var), with solve=True also (alpha, K^-1)."""
    import scipy.linalg as sl
    l2, sf2, sn2 = np.exp(2 * np.asarray(hp, dtype=np.float64))
    n = len(y)
    S = np.zeros((n, n))
    for k in range(X.shape[1]):
        D = X[:, k][:, None] - X[:, k][None, :]
        S += D * D
    S /= l2
    Kf = sf2 * np.exp(-S / 2)
    K = Kf + sn2 * np.eye(n)
    L = np.linalg.cholesky(K)
    T = sl.solve_triangular(L, np.eye(n), lower=True)
    Ki = T.T @ T
    a = Ki @ y
    ll = -0.5 * (y @ a + 2 * np.log(np.diag(L)).sum() + n * LL_CONST)
    W = Ki - np.outer(a, a)
    g = np.array([(W * Kf * S).sum() / 2, (W * Kf).sum(), sn2 * np.trace(W)])
    St = np.zeros((Xt.shape[0], n))
    for k in range(X.shape[1]):
        D = Xt[:, k][:, None] - X[:, k][None, :]
        St += D * D
    Ks = sf2 * np.exp(-St / l2 / 2)
    Wt = Ks @ T.T
    out = (ll, g, Ks @ a, sf2 + sn2 - (Wt * Wt).sum(1))
    return out + (a, Ki) if solve else out


def standin_bcm(X, y, hp, K, Xt):
    ll, g, sp, spm = 0.0, np.zeros(3), 0.0, 0.0
    for off, rows in bcm_rows(len(y), K):
        l, gr, m, v = standin(X[off: off + rows], y[off: off + rows], hp, Xt)
        ll, g, sp, spm = ll + l, g + gr, sp + 1 / v, spm + m / v
    return ll, g, spm / sp, 1 / sp


# ---------------------------------------------------------------------------------------- the cases
# err_gpu <= F max(noise, floor).  Both factors are the next power of two at or above twice the largest stand-in /
# yardstick ratio over the case list (docs/ACCURACY.md), never set from the GPU's errors.
F = 8             # LL, gradient, means, variances, joint covariance: largest stand-in ratio 3.16 (mean, n2049)
F_SOLVE = 32      # alpha and rows of K^-1: largest stand-in ratio 9.88 (K^-1, cond(K) ~ 1e6)
YARDSTICK_CAP = 1e-9
NT = 64
HP_A = [0.9, 0.2, -1.0]

# name -> (n, d, hyper-parameters, box half-width of synth: chosen so that K is far from diagonal)
LIVE_CASES = {
    "n2": (2, 2, HP_DEFAULT, 4.0),
    "n63": (63, 2, HP_DEFAULT, 4.0),                 # below / at / over one 64-row build tile; one 128 MFMA tile,
    "n64": (64, 2, HP_DEFAULT, 4.0),                 # identity padding
    "n65": (65, 2, HP_DEFAULT, 4.0),
    "n257_d3": (257, 3, HP_A, 4.0),                  # three tiles, ragged
    "n300_d17": (300, 17, [1.1, 0.3, -0.8], 1.8),    # two feature chunks through k_trace and k_cross
    "n515_d33": (515, 33, HP_BCM, 1.9),              # three feature chunks, ragged n
    "n515_dense": (515, 5, HP_DENSE, 10.0),          # dense K, long length scale
    "n384_cond1e6": (384, 2, [1.5, 0.5, -3.0], 2.0),  # cond(K) ~ 1e6: the yardstick moves to 1e-12 .. 1e-10
    "n1025_dense": (1025, 10, HP_DENSE, 10.0),       # nine tiles; overlap on and off
    "n1300_d6": (1300, 6, HP_A, 2.5),                # hand-over blocks of the inverse
}
JOINT_CASES = ("n2", "n63", "n64", "n1025_dense", "n1300_d6")     # the three smallest and the two largest


def live_inputs(name):
    """-> (X, y, Xt, hp): synth data of the case and 64 test points in the same box, one of them a training row."""
    n, d, hp, scale = LIVE_CASES[name]
    X, y = synth(n, d=d, seed=3 * n + d, scale=scale)
    Xt = synth(NT, d=d, seed=7, scale=scale)[0]
    Xt[5] = X[n // 2]
    return X, y, np.ascontiguousarray(Xt), list(hp)


def solve_rows(n):
    """The 64 fixed-seed rows of K^-1 that are compared."""
    return np.sort(np.random.default_rng(11).choice(n, min(64, n), replace=False))


def solve_errors(a, Ki, t, rows):
    """alpha and the chosen rows of K^-1 against the truth: largest absolute error relative to the largest entry."""
    return dict(alpha=float(np.max(np.abs(np.asarray(a).astype(LD) - t.alpha)) / np.max(np.abs(t.alpha))),
                kinv=float(np.max(np.abs(np.asarray(Ki)[rows].astype(LD) - t.Kinv[rows])) / np.max(np.abs(t.Kinv))))


# ---------------------------------------------------------------------------------------- beyond one test tile
# tests/test_gpu_predict_wide.py: the prediction side pads to 128-row tiles, and NT = 64 runs exactly one of them.  The
# wide cases predict at two and three test tiles; the draws and their factor are held to derived bounds.
WIDE_NTS = (129, 200, 257)        # two tiles, one row into the second; two tiles, ragged; three tiles
# case of LIVE_CASES -> the nt it runs at (small on purpose: truths and yardsticks are computed live)
WIDE_CASES = {
    "n65": WIDE_NTS,                   # nt > n; the covariance product's k range is one block
    "n300_d17": WIDE_NTS,              # two feature chunks through k_cross
    "n384_cond1e6": WIDE_NTS,
    "n515_dense": WIDE_NTS,            # the covariance product splits in two over k
    "n1025_dense": (200,),             # ... in four
}
WIDE_NT_FAMILY = 200                   # the one size of the ARD, Matern and BCM cases
WIDE_TRAINING_ROW = -2                 # the test row that is a training row: beyond the first tile at every size
POTRF_EXTRA_ULPS = 15                  # gamma_(n + 15) for the library's Cholesky: derived in test_gpu_accuracy.test_factor_residual,
                                       # the one constant behind every factor bound (GPU and CPU counterpart)


def wide_points(X, nt, scale):
    """nt test points in the box of the case (synth's seed 7, as live_inputs), the last but one a training row."""
    Xt = synth(nt, d=X.shape[1], seed=7, scale=scale)[0]
    Xt[WIDE_TRAINING_ROW] = X[len(X) // 2]
    return np.ascontiguousarray(Xt)


def wide_inputs(name, nt):
    """-> (X, y, Xt, hp): live_inputs' data and hyper-parameters with nt test points."""
    X, y, _, hp = live_inputs(name)
    return X, y, wide_points(X, nt, LIVE_CASES[name][3]), hp


def se_fp64(hp):
    """The stand-in's fp64 squared-exponential kernel function (no noise) -> kf(A, B)."""
    l2, sf2 = np.exp(2 * np.asarray(hp[:2], dtype=np.float64))

    def kf(A, B):
        S = np.zeros((A.shape[0], B.shape[0]))
        for k in range(A.shape[1]):
            D = A[:, k][:, None] - B[:, k][None, :]
            S += D * D
        return sf2 * np.exp(-S / l2 / 2)
    return kf


def standin_joint(kf, X, y, Xt, sf2, sn2):
    """`standin`'s prediction for any fp64 kernel function kf(A, B), with the joint covariance: LAPACK's Cholesky, a
    triangular solve against I, BLAS products.  -> (mean, var, latent covariance); with noise: + sn2 on the diagonal."""
    import scipy.linalg as sl
    n = len(y)
    L = np.linalg.cholesky(kf(X, X) + sn2 * np.eye(n))
    T = sl.solve_triangular(L, np.eye(n), lower=True)
    a = (T.T @ T) @ y
    Ks = kf(Xt, X)
    Wt = Ks @ T.T
    return Ks @ a, sf2 + sn2 - (Wt * Wt).sum(1), kf(Xt, Xt) - Wt @ Wt.T


def joint_errors(mean, var, cov_noise, cov_latent, tmean, tvar, tcov_latent, sn2):
    """Largest absolute error of the means, the variances, and of any entry of the joint covariance with and without
    noise (the true covariance with noise is the latent one + sn2 on its diagonal, added in longdouble)."""
    tcn = tcov_latent.copy()
    tcn[np.arange(len(tcn)), np.arange(len(tcn))] += sn2
    e = errors_pred(mean, var, tmean, tvar)
    e["cov_noise"] = float(np.max(np.abs(np.asarray(cov_noise).astype(LD) - tcn)))
    e["cov_latent"] = float(np.max(np.abs(np.asarray(cov_latent).astype(LD) - tcov_latent)))
    return e


def factor_rule(worst):
    """The project's rule for a factor F: the next power of two at or above twice the largest stand-in ratio."""
    F = 1
    while F < 2 * worst:
        F *= 2
    return F


def factor_bound_worst(S, C, index, diag_allow=0.0):
    """The componentwise bound on a computed Cholesky factor, on ALL rows of the lower triangle:
        |S - C C^T|_ij <= gamma_index (|C||C^T|)_ij   (+ diag_allow on diagonal entries)
    S: the matrix that was factored (fp64, or longdouble where it was never formed in fp64), C: its fp64 factor.
    -> (largest residual / bound, (i, j), that residual, that bound)."""
    nt = len(C)
    res, mag = potrf_residual_rows(S, C, range(nt))
    worst = (-1.0, None, 0.0, 0.0)
    for i in range(nt):
        b = gamma(index) * mag[i]
        b[i] += diag_allow
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(res[i] == 0, LD(0), res[i] / b)          # (0 <= 0 holds; anything over a zero bound is inf)
        j = int(np.argmax(r))
        if not float(r[j]) <= worst[0]:
            worst = (float(r[j]), (i, j), float(res[i][j]), float(b[j]))
    return worst


def draw_bound_worst(s, m, Z, C):
    """Draws s = m + Z C^T in fp64, any order of summation, with or without fma, plus the one rounding of the final sum:
        |s_st - (m_t + sum_k z_sk C_tk)| <= gamma_(nt+1) (|m_t| + sum_k |z_sk||C_tk|)
    with the right-hand sides in longdouble from the fp64 m, Z, C.  -> (largest error / bound, (s, t), error, bound)."""
    Zl, Cl, ml = np.asarray(Z).astype(LD), np.asarray(C).astype(LD), np.asarray(m).astype(LD)
    nt = len(ml)
    Ct = np.ascontiguousarray(Cl.T)
    err = np.abs(np.asarray(s).astype(LD) - (ml[None, :] + _mm(Zl, Ct)))
    bnd = gamma(nt + 1) * (np.abs(ml)[None, :] + _mm(np.abs(Zl), np.abs(Ct)))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, LD(0), err / bnd)
    k = np.unravel_index(int(np.argmax(r)), r.shape)
    return float(r[k]), (int(k[0]), int(k[1])), float(err[k]), float(bnd[k])
