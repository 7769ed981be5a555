"""Extended-precision truth for the GP hot path -- TEST INFRASTRUCTURE, CPU, numpy only.

A plain numpy.longdouble (x86 80-bit, eps 1.08e-19) restatement of the formulas of SURVEY.md / k_finalize, written
for clarity.  The inputs (fp64 data, fp64 log-hyper-parameters) are exact; everything from exp(2 theta) on is
evaluated in longdouble, so the result is some 3 digits beyond anything an fp64 implementation can deliver and can
serve as the truth its rounding error is measured against (tests/test_truth_cpu.py checks that against mpmath).

    K    = Kf + sn2 I,  Kf = k(xi, xj) of the covariance family (a descriptor: SE, ARD, Matern -- below)
    K    = L L^T (right-looking, blocked), T = L^-1, K^-1 = T^T T, alpha = K^-1 y
    LL   = -1/2 (y^T alpha + 2 sum log L_ii + n c),   c = the fp64 value of the literal 1.83787 (not log 2 pi)
    grad = (the family's length-scale terms, sum W o Kf, sn2 tr W),   W = K^-1 - alpha alpha^T
    mean = Ks alpha, var = sf2 + sn2 - |Ks T^T|^2 per test point, cov = k(Xt, Xt) (+ sn2 I) - (Ks T^T)(Ks T^T)^T

The families, each a small value that knows sf2, sn2, its quantity names and its factor F, and evaluates in
longdouble (the truth) or in fp64 (`fp64()`: the stand-in and the Matern yardstick) with the SAME order of operations:

    SE      theta = [log l, log sf, log sn]:  S = |xi - xj|^2 / l^2,  Kf = sf2 exp(-S / 2),  g0 = 1/2 sum (W o Kf) o S
    ARD     theta = [log l_1 .. log l_d, log sf, log sn] (GPML covSEard's order):  w_c = exp(-theta_c),
            Kf = sf2 exp(-1/2 sum_c ((x_ic - x_jc) w_c)^2),  g_c = 1/2 sum (W o Kf) o ((x_ic - x_jc) w_c)^2
    Matern  theta as SE, kind 1 (nu = 3/2) | 2 (nu = 5/2):  r = sqrt(S),
            a = sqrt(3) r:  Kf = sf2 (1 + a) exp(-a),            dK/dtheta_0 = sf2 a^2 exp(-a)
            a = sqrt(5) r:  Kf = sf2 (1 + a + a^2/3) exp(-a),    dK/dtheta_0 = sf2 (a^2/3) (1 + a) exp(-a);  g0 = 1/2 sum W o dK

`noise_level` is the yardstick of the GPU accuracy tests: what the reference-order fp64 arithmetic of the CPU oracle
delivers on the very same input, as the largest error against the truth over the data as given and 7 fixed-seed row
permutations of it (every checked quantity is invariant under them; the rounding is not).  The oracle has the
isotropic squared exponential only, so each family brings its `evaluator`: SE the oracle directly; ARD the oracle on
the scaled copy X / l with theta_0 = 0 (its g0 then evaluates sum_c g_c, and EVERY g_c is held to that yardstick: each
is a partial sum of the same terms on the same scale); Matern its fp64 K through the oracle's factorisation,
inverse and solve.
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
U4 = 4 * 2.0 ** -52               # 4 ulp: the floor of every relative quantity
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


# ---------------------------------------------------------------------------------------- the covariance families
# err_gpu <= F max(noise, floor).  Every factor is the next power of two at or above twice the largest stand-in /
# yardstick ratio over the family's case list (docs/ACCURACY.md; measured on the CPU by tests/test_truth_cpu.py,
# test_truth_ard_cpu.py, test_truth_matern_cpu.py), never set from the GPU's errors.
F = 8             # SE: LL, gradient, means, variances, joint covariance: largest stand-in ratio 3.16 (mean, n2049)
F_ARD = 32        # largest stand-in ratio: 8.70, the predictive mean at cond(K) ~ 1e6 (twice that is 17.4)
F_MATERN = 16     # largest stand-in ratio: 5.23, the predictive mean of n257_d3 at nu = 5/2 (twice that is 10.5)
F_SOLVE = 32      # alpha and rows of K^-1, every family: largest stand-in ratio 9.88 (K^-1, cond(K) ~ 1e6)
YARDSTICK_CAP = 1e-9

QUANTITIES = ("ll", "g0", "g1", "g2", "mean", "var")
QUANTITIES_ARD = ("ll", "gc", "gf", "gn", "mean", "var")     # gc: the largest error over the d per-dimension components
SOLVE_QUANTITIES = ("alpha", "kinv")

MATERN32, MATERN52 = 1, 2                   # the library's kernel kinds (0: SE)
KINDS = (MATERN32, MATERN52)
KIND_NAMES = {MATERN32: "matern32", MATERN52: "matern52"}
C2 = {MATERN32: 3, MATERN52: 5}             # a = sqrt(C2) r


def hyper(hp, dtype=LD):
    """(l^2, sf2, sn2) = exp(2 theta) in `dtype` from the fp64 log-hyper-parameters."""
    return tuple(np.exp(2 * dtype(float(h))) for h in hp)


def sqdist(A, B, dtype=LD):
    """|a_i - b_j|^2 in `dtype`, one feature at a time in index order (no n x n x d temporary)."""
    A, B = np.asarray(A, dtype=dtype), np.asarray(B, dtype=dtype)
    S = np.zeros((A.shape[0], B.shape[0]), dtype=dtype)
    for k in range(A.shape[1]):
        D = A[:, k][:, None] - B[:, k][None, :]
        S += D * D
    return S


def wsqdist(A, B, w, per_dim=None):
    """sum_c ((a_ic - b_jc) w_c)^2 in the dtype of w, one feature at a time; per_dim(c, D2) sees every term."""
    A, B = np.asarray(A, dtype=w.dtype), np.asarray(B, dtype=w.dtype)
    S = np.zeros((A.shape[0], B.shape[0]), dtype=w.dtype)
    for c in range(A.shape[1]):
        D = (A[:, c][:, None] - B[:, c][None, :]) * w[c]
        D *= D
        if per_dim is not None:
            per_dim(c, D)
        S += D
    return S


def matern_kernel(S, sf2, kind):
    """(Kf, dK/dlog l) from s = |x - x'|^2 / l^2, in the dtype of S: the textbook form (one sqrt of 3 s or 5 s, a^2 / 3
    by division)."""
    a = np.sqrt(C2[kind] * S)
    e = np.exp(-a)
    if kind == MATERN32:
        return sf2 * (1 + a) * e, sf2 * a * a * e
    t = a * a / 3
    return sf2 * (1 + a + t) * e, sf2 * t * (1 + a) * e


def oracle_evaluator(oracle, hp, Xt, solve=False):
    """-> evaluate(X, y) -> (ll, grad, mean, var) of the CPU oracle (isotropic SE); with solve also alpha and K^-1
    from its potrs / potri on its own K."""
    def evaluate(X, y):
        ll, g = oracle.loglik_grad(X, y, hp)
        out = (ll, g) + tuple(oracle.predict(X, y, hp, Xt))
        if solve:
            K = oracle.K_train(X, hp)
            out += (oracle.Kinvy(K, y), oracle.K_inverse(K))
        return out
    return evaluate


def poe(parts, evaluate):
    """-> evaluate_all(X, y): `evaluate` on every expert's rows [(offset, rows)], LL and gradient summed in expert
    order, product of experts: var = 1 / sum 1/v_k, mean = var * sum m_k / v_k."""
    def evaluate_all(X, y):
        ll, g, sp, spm = 0, 0, 0, 0
        for off, rows in parts:
            l, gr, m, v = evaluate(X[off: off + rows], y[off: off + rows])
            ll, g, sp, spm = ll + l, g + gr, sp + 1 / v, spm + m / v
        return ll, g, spm / sp, 1 / sp
    return evaluate_all


class SE:
    """The isotropic squared exponential at theta = [log l, log sf, log sn]."""
    quantities, F = QUANTITIES, F

    def __init__(self, hp, dtype=LD):
        self.hp, self.dtype = [float(h) for h in hp], dtype
        self.l2, self.sf2, self.sn2 = hyper(self.hp, dtype)

    def fp64(self):
        """The same covariance evaluated in fp64."""
        return SE(self.hp, np.float64)

    def train(self, X):
        """-> (Kf, terms): the training covariance without noise and terms(W) -> the gradient components other than
        the noise one.  (The terms are a function of W, not a dK matrix: each family keeps its own association.)"""
        S = sqdist(X, X, self.dtype) / self.l2
        Kf = self.sf2 * np.exp(-S / 2)

        def terms(W):
            WK = W * Kf
            return (WK * S).sum() / 2, WK.sum()
        return Kf, terms

    def k(self, A, B):
        return self.sf2 * np.exp(-sqdist(A, B, self.dtype) / self.l2 / 2)

    def evaluator(self, oracle, X, Xt, solve=False):
        """The yardstick's fp64 evaluation -> (the data whose rows are permuted, evaluate(Xp, yp))."""
        return X, oracle_evaluator(oracle, self.hp, Xt, solve)

    def bcm_evaluator(self, oracle, K, Xt):
        """The oracle's own BCM over the reference's row split into K experts."""
        def evaluate(X, y):
            b = oracle.bcm(X, y, K, self.hp)
            try:
                return (b.loglik()[0], b.grad()) + tuple(b.predict(Xt))
            finally:
                b.close()
        return evaluate


class Matern(SE):
    """Matern 3/2 (kind 1) and 5/2 (kind 2) at the isotropic three (GPML covMaterniso)."""
    F = F_MATERN

    def __init__(self, hp, kind, dtype=LD):
        assert kind in KINDS
        SE.__init__(self, hp, dtype)
        self.kind = kind

    def fp64(self):
        return Matern(self.hp, self.kind, np.float64)

    def train(self, X):
        Kf, dK = matern_kernel(sqdist(X, X, self.dtype) / self.l2, self.sf2, self.kind)
        return Kf, lambda W: ((W * dK).sum() / 2, (W * Kf).sum())

    def k(self, A, B):
        return matern_kernel(sqdist(A, B, self.dtype) / self.l2, self.sf2, self.kind)[0]

    def evaluator(self, oracle, X, Xt, solve=False):
        """The oracle evaluates the squared exponential only, but it factors, inverts and solves a caller's matrix in
        the reference's order of operations: the Matern K is formed in fp64 numpy and handed to that -- LL from
        chol_and_det, the traces from K_inverse and Kinvy, the mean from Ks Kinvy, the variance from Ks K^-1 Ks^T."""
        c = self.fp64()

        def evaluate(Xp, yp):
            n = len(yp)
            Kf, terms = c.train(Xp)
            K = Kf + c.sn2 * np.eye(n)
            quad, logdet = oracle.chol_and_det(K, yp)
            ll = -0.5 * (quad + logdet + n * LL_CONST)
            Ki = oracle.K_inverse(K)
            a = oracle.Kinvy(K, yp)
            W = Ki - np.outer(a, a)
            g = np.array(terms(W) + (c.sn2 * np.trace(W),))
            Ks = c.k(Xt, Xp)
            out = (ll, g, Ks @ a, c.sf2 + c.sn2 - ((Ks @ Ki) * Ks).sum(1))
            return out + (a, Ki) if solve else out
        return X, evaluate

    def bcm_evaluator(self, oracle, K, Xt):
        """Every expert through `evaluator`, combined in expert order."""
        def evaluate(X, y):
            return poe(bcm_rows(len(y), K), self.evaluator(oracle, X, Xt)[1])(X, y)
        return evaluate


class ARD:
    """The squared exponential with one length scale per input dimension at theta = [log l_1 .. log l_d, log sf,
    log sn]; differences are weighted before they are squared."""
    quantities, F = QUANTITIES_ARD, F_ARD

    def __init__(self, hp, dtype=LD):
        self.hp, self.dtype = [float(h) for h in hp], dtype
        th = np.asarray(self.hp[:-2], dtype=np.float64)
        self.w = np.exp(-th.astype(dtype))
        self.sf2, self.sn2 = np.exp(2 * dtype(self.hp[-2])), np.exp(2 * dtype(self.hp[-1]))

    def fp64(self):
        return ARD(self.hp, np.float64)

    def train(self, X):
        assert X.shape[1] == len(self.w)
        Kf = self.sf2 * np.exp(-wsqdist(X, X, self.w) / 2)

        def terms(W):
            WK = W * Kf
            g = [None] * len(self.w)

            def per_dim(c, D2):
                g[c] = (WK * D2).sum() / 2
            wsqdist(X, X, self.w, per_dim)           # the dimensions a second time, W o Kf fixed
            return tuple(g) + (WK.sum(),)
        return Kf, terms

    def k(self, A, B):
        return self.sf2 * np.exp(-wsqdist(A, B, self.w) / 2)

    def scaled(self, X):
        """X / l in fp64: with [0, theta_d, theta_{d+1}] the isotropic problem the oracle can evaluate."""
        return np.ascontiguousarray(np.asarray(X, dtype=np.float64) / np.exp(np.asarray(self.hp[:-2], dtype=np.float64)))

    def evaluator(self, oracle, X, Xt, solve=False):
        """The ARD model on X is the isotropic model with theta_0 = 0 on the scaled copy X / l.  The oracle's g0 there
        evaluates sum_c g_c (`errors_ll_grad` compares it with the sum of the true components)."""
        return self.scaled(X), oracle_evaluator(oracle, [0.0] + self.hp[-2:], self.scaled(Xt), solve)


class Truth:
    """Every checked quantity of one expert with covariance `cov`, in longdouble.  Attributes: n, cov, sf2, sn2, T
    (= L^-1), alpha, ll, grad[len(theta)], with keep also K, L, Kinv; cross(Xt) / predict(Xt) / joint(Xt, with_noise)
    for the test points."""

    def __init__(self, X, y, cov, keep=True):
        require_extended()
        X = np.asarray(X, dtype=np.float64)
        self.X = X.astype(LD)
        yl = np.asarray(y, dtype=np.float64).astype(LD)
        n = self.n = X.shape[0]
        self.cov, self.sf2, self.sn2 = cov, cov.sf2, cov.sn2
        Kf, terms = cov.train(self.X)
        K = Kf.copy()
        K[np.arange(n), np.arange(n)] += self.sn2
        L = cholesky(K)
        T = tri_inverse(L)
        Kinv = gram_lower(T)
        alpha = Kinv @ yl
        self.ll = -LD(0.5) * (yl @ alpha + 2 * np.log(np.diag(L)).sum() + n * LD(LL_CONST))
        W = Kinv - np.outer(alpha, alpha)
        self.grad = np.array(terms(W) + (self.sn2 * np.trace(W),), dtype=LD)
        self.alpha, self.T = alpha, T
        if keep:
            self.K, self.L, self.Kinv = K, L, Kinv

    def _cross(self, Xt):
        Xt = np.asarray(Xt, dtype=np.float64).reshape(-1, self.X.shape[1]).astype(LD)
        Ks = self.cov.k(Xt, self.X)
        return Xt, Ks, _mm(Ks, np.ascontiguousarray(self.T.T))

    def cross(self, Xt):
        return self._cross(Xt)[1]

    def predict(self, Xt):
        _, Ks, Wt = self._cross(Xt)
        return Ks @ self.alpha, self.sf2 + self.sn2 - (Wt * Wt).sum(1)

    def joint(self, Xt, with_noise=True):
        Xt, Ks, Wt = self._cross(Xt)
        cov = self.cov.k(Xt, Xt) - Wt @ Wt.T
        if with_noise:
            cov[np.arange(len(cov)), np.arange(len(cov))] += self.sn2
        return Ks @ self.alpha, cov


def bcm_rows(N, K):
    """Row partition of the reference's BCM constructor, as cugp_bcm_create_split: K - 1 parts of N // K rows, the
    last takes the rest.  -> [(offset, rows)]."""
    part = N // K
    return [(k * part, part if k < K - 1 else N - part * (K - 1)) for k in range(K)]


def bcm_truth(X, y, cov, K, Xt):
    """Product of experts over the row split, every expert with covariance `cov`: -> dict(ll, grad, mean, var)."""
    def expert(Xk, yk):
        t = Truth(Xk, yk, cov, keep=False)
        return (t.ll, t.grad) + t.predict(Xt)
    return dict(zip(("ll", "grad", "mean", "var"), poe(bcm_rows(len(y), K), expert)(X, y)))


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
def scales(cov, ll, grad, mean):
    """The size each quantity's error is taken relative to / floored at: |LL|, max|g|, max|mean|, sf2 + sn2."""
    gs = float(np.max(np.abs(grad)))
    sv = float(np.exp(2 * cov.hp[-2]) + np.exp(2 * cov.hp[-1]))
    ql, qa, qb, qc = cov.quantities[:4]
    return {ql: float(abs(ll)), qa: gs, qb: gs, qc: gs, "mean": float(np.max(np.abs(mean))), "var": sv, "cov": sv}


def floors(cov, sc):
    """4 ulp of each quantity's scale, in the units of `errors` (LL and gradient are already relative)."""
    fl = {q: U4 for q in cov.quantities[:4]}
    fl.update(mean=U4 * sc["mean"], var=U4 * sc["var"], cov=U4 * sc["cov"])
    return fl


def errors_ll_grad(cov, ll, grad, tll, tgrad):
    """LL relative to |LL|; the gradient relative to the largest true component: the worst of the length-scale
    components (one for SE and Matern, d for ARD), then the signal and the noise component.  A `grad` of three against
    an ARD truth carries the SUM of the length-scale components in its first entry (ARD.evaluator) and is compared
    with the sum of the true ones.  Differences are taken in longdouble."""
    gs = np.max(np.abs(tgrad))
    d = len(tgrad) - 2
    g = np.asarray(grad).astype(LD)
    lead = np.max(np.abs(g[:d] - tgrad[:d])) if len(g) == d + 2 else abs(g[0] - tgrad[:d].sum())
    e = (abs(LD(ll) - tll) / abs(tll), lead / gs, abs(g[-2] - tgrad[d]) / gs, abs(g[-1] - tgrad[d + 1]) / gs)
    return {q: float(v) for q, v in zip(cov.quantities, e)}


def errors_pred(mean, var, tmean, tvar):
    """Means and variances: the largest absolute error."""
    return dict(mean=float(np.max(np.abs(np.asarray(mean).astype(LD) - tmean))),
                var=float(np.max(np.abs(np.asarray(var).astype(LD) - tvar))))


def errors(cov, ll, grad, mean, var, tll, tgrad, tmean, tvar):
    """Errors of one fp64 evaluation against the truth, per quantity of cov.quantities."""
    return dict(errors_ll_grad(cov, ll, grad, tll, tgrad), **errors_pred(mean, var, tmean, tvar))


def solve_rows(n):
    """The 64 fixed-seed rows of K^-1 that are compared."""
    return np.sort(np.random.default_rng(11).choice(n, min(64, n), replace=False))


def solve_errors(a, Ki, t, rows):
    """alpha and the chosen rows of K^-1 against the truth: largest absolute error relative to the largest entry."""
    return dict(alpha=float(np.max(np.abs(np.asarray(a).astype(LD) - t.alpha)) / np.max(np.abs(t.alpha))),
                kinv=float(np.max(np.abs(np.asarray(Ki)[rows].astype(LD) - t.Kinv[rows])) / np.max(np.abs(t.Kinv))))


def permutations(n, parts=None):
    """The data as given, then NPERM fixed-seed row permutations; with `parts` [(offset, rows)] the rows move inside
    their own part only (a BCM's experts keep their rows)."""
    rng = np.random.default_rng(PERM_SEED)
    parts = parts or [(0, n)]
    return [np.arange(n)] + [np.concatenate([off + rng.permutation(r) for off, r in parts]) for _ in range(NPERM)]


def noise_level(cov, evaluate, X, y, tll, tgrad, tmean, tvar, parts=None, solve=None):
    """-> (noise, first, rest): per quantity of cov.quantities the largest error of the fp64 `evaluate(Xp, yp) -> (ll,
    grad, mean, var)` against the truth over the data as given and NPERM row permutations, the error on the data as
    given alone, the largest over the permutations alone.  `parts` keeps the rows inside their expert (the BCM case).
    With solve = (truth, rows) `evaluate` also returns (alpha, K^-1) of the permuted problem, and a fourth dictionary
    holds the same yardstick for alpha and the chosen rows of K^-1 (largest absolute error relative to the largest
    entry)."""
    n = len(y)

    def one(idx):
        out = evaluate(np.ascontiguousarray(X[idx]), np.ascontiguousarray(y[idx]))
        e = errors(cov, *out[:4], tll, tgrad, tmean, tvar)
        if solve:
            t, rows = solve
            inv = np.empty(n, dtype=np.int64)
            inv[idx] = np.arange(n)
            e.update(solve_errors(out[4][inv], out[5][np.ix_(inv, inv)], t, rows))
        return e
    E = list(_pool().map(one, permutations(n, parts)))            # the oracle is serial C behind ctypes: one thread each
    Q = cov.quantities
    out = {q: max(e[q] for e in E) for q in Q}, {q: E[0][q] for q in Q}, {q: max(e[q] for e in E[1:]) for q in Q}
    return out + ({q: max(e[q] for e in E) for q in SOLVE_QUANTITIES},) if solve else out


def yardstick(oracle, cov, X, y, Xt, t, tmean, tvar, rows=None):
    """`noise_level` of one expert with the family's evaluator; with `rows` also for alpha and those rows of K^-1."""
    Xe, evaluate = cov.evaluator(oracle, X, Xt, solve=rows is not None)
    return noise_level(cov, evaluate, Xe, y, t.ll, t.grad, tmean, tvar, solve=None if rows is None else (t, rows))


def bcm_yardstick(oracle, cov, X, y, K, Xt, tb):
    """`noise_level` of the product of K experts against bcm_truth's tb, the rows permuted inside their own expert."""
    return noise_level(cov, cov.bcm_evaluator(oracle, K, Xt), X, y, tb["ll"], tb["grad"], tb["mean"], tb["var"],
                       parts=bcm_rows(len(y), K))


def standin(cov, X, y, Xt, solve=False, joint=False):
    """The same quantities from an independent fp64 implementation in another order: LAPACK's blocked Cholesky, a
    triangular solve against I, BLAS products (blocked, FMA-contracted -- as the MFMA path is).
    -> (ll, grad, mean, var), with joint=True + (the latent joint covariance; with noise: + sn2 on the diagonal), with
    solve=True + (alpha, K^-1)."""
    import scipy.linalg as sl
    c = cov.fp64()
    X, Xt = np.asarray(X, dtype=np.float64), np.asarray(Xt, dtype=np.float64)
    n = len(y)
    Kf, terms = c.train(X)
    L = np.linalg.cholesky(Kf + c.sn2 * np.eye(n))
    T = sl.solve_triangular(L, np.eye(n), lower=True)
    Ki = T.T @ T
    a = Ki @ y
    ll = -0.5 * (y @ a + 2 * np.log(np.diag(L)).sum() + n * LL_CONST)
    W = Ki - np.outer(a, a)
    g = np.array(terms(W) + (c.sn2 * np.trace(W),))
    Ks = c.k(Xt, X)
    Wt = Ks @ T.T
    out = (ll, g, Ks @ a, c.sf2 + c.sn2 - (Wt * Wt).sum(1))
    if joint:
        out += (c.k(Xt, Xt) - Wt @ Wt.T,)
    return out + (a, Ki) if solve else out


def standin_bcm(cov, X, y, K, Xt):
    return poe(bcm_rows(len(y), K), lambda Xk, yk: standin(cov, Xk, yk, Xt))(X, y)


# ---------------------------------------------------------------------------------------- the cases
NT = 64
HP_A = [0.9, 0.2, -1.0]

# name -> (n, d, hyper-parameters, box half-width of synth: chosen so that K is far from diagonal)
LIVE_CASES = {
    "n1": (1, 2, HP_DEFAULT, 4.0),                   # one row: every off-diagonal sum is empty
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
JOINT_CASES = ("n1", "n2", "n63", "n64", "n1025_dense", "n1300_d6")     # the four smallest and the two largest
MATERN_CASES = tuple(LIVE_CASES)                     # every live case, both kinds

# name -> (n, d, theta_l, theta_f, theta_n, box half-width of synth, shift added to X and Xt)
ARD_CASES = {
    "n1_d2": (1, 2, [0.5, 1.2], 0.5, 0.5, 4.0, 0.0),                                    # below / at one 64-row build tile,
    "n2_d2": (2, 2, [0.5, 1.2], 0.5, 0.5, 4.0, 0.0),                                    # n65_d2's parameters
    "n63_d2": (63, 2, [0.5, 1.2], 0.5, 0.5, 4.0, 0.0),
    "n64_d2": (64, 2, [0.5, 1.2], 0.5, 0.5, 4.0, 0.0),
    "n65_d2": (65, 2, [0.5, 1.2], 0.5, 0.5, 4.0, 0.0),
    "n257_d3": (257, 3, [0.9, 0.3, 1.6], 0.2, -1.0, 4.0, 0.0),
    "n300_d17": (300, 17, np.linspace(0.7, 1.9, 17).tolist(), 0.3, -0.8, 1.8, 0.0),      # two feature chunks
    "n515_dense": (515, 5, [3.2, 3.8, 4.4, 3.5, 4.0], HP_DENSE[1], HP_DENSE[2], 10.0, 0.0),
    "n384_cond1e6": (384, 2, [1.2, 1.8], 0.5, -3.0, 2.0, 0.0),
    "n257_d3_shift": (257, 3, [0.9, 0.3, 1.6], 0.2, -1.0, 4.0, 100.0),                   # |x| >> |x - x'|
    "n515_d33": (515, 33, np.linspace(1.2, 1.8, 33).tolist(), 1.5, 1.5, 1.9, 0.0),       # three feature chunks
    "n1025_dense": (1025, 10, (HP_DENSE[0] + np.linspace(-0.4, 0.4, 10)).tolist(), HP_DENSE[1], HP_DENSE[2], 10.0, 0.0),
    "n1300_d6": (1300, 6, [0.6, 0.8, 0.9, 1.0, 1.1, 1.3], 0.2, -1.0, 2.5, 0.0),          # hand-over blocks
}
JOINT_CASES_ARD = ("n65_d2", "n257_d3", "n1025_dense", "n1300_d6")       # the two smallest and the two largest


def points(X, d, scale, nt=NT, row=5):
    """nt test points in the box of the data (synth's seed 7), row `row` of them a training row."""
    Xt = synth(nt, d=d, seed=7, scale=scale)[0]
    Xt[row] = X[len(X) // 2]
    return Xt


def live_inputs(name):
    """-> (X, y, Xt, hp): synth data of the case and 64 test points in the same box, one of them a training row."""
    n, d, hp, scale = LIVE_CASES[name]
    X, y = synth(n, d=d, seed=3 * n + d, scale=scale)
    return X, y, np.ascontiguousarray(points(X, d, scale)), list(hp)


def ard_inputs(name):
    """-> (X, y, Xt, hp): the same for a case of ARD_CASES, hp of d + 2 entries."""
    n, d, th, tf, tn, scale, shift = ARD_CASES[name]
    X, y = synth(n, d=d, seed=3 * n + d, scale=scale)
    Xt = points(X, d, scale)
    return np.ascontiguousarray(X + shift), y, np.ascontiguousarray(Xt + shift), list(th) + [tf, tn]


# family -> (the input builder of its live cases, hp -> its descriptor, case -> the box half-width of its data)
FAMILIES = {
    "se": (live_inputs, SE, lambda name: LIVE_CASES[name][3]),
    "ard": (ard_inputs, ARD, lambda name: ARD_CASES[name][5]),
    "matern32": (live_inputs, lambda hp: Matern(hp, MATERN32), lambda name: LIVE_CASES[name][3]),
    "matern52": (live_inputs, lambda hp: Matern(hp, MATERN52), lambda name: LIVE_CASES[name][3]),
}


def family_inputs(family, name):
    """-> (X, y, Xt, cov) of a live case of a family of FAMILIES."""
    X, y, Xt, hp = FAMILIES[family][0](name)
    return X, y, Xt, FAMILIES[family][1](hp)


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
WIDE_FAMILY_CASES = {"ard": "n257_d3", "matern52": "n300_d17"}     # family -> its one wide case
WIDE_BCM = ((3 * 300, 3), (5 * 261 + 2, 5))                         # (rows, experts): three equal experts, an uneven split
HP_BCM_WIDE = [0.9, 0.2, -1.0]
WIDE_TRAINING_ROW = -2                 # the test row that is a training row: beyond the first tile at every size
POTRF_EXTRA_ULPS = 15                  # gamma_(n + 15) for the library's Cholesky: derived in test_gpu_accuracy.test_factor_residual,
                                       # the one constant behind every factor bound (GPU and CPU counterpart)


def wide_points(X, nt, scale):
    """nt test points in the box of the case (synth's seed 7, as live_inputs), the last but one a training row."""
    return np.ascontiguousarray(points(X, X.shape[1], scale, nt, WIDE_TRAINING_ROW))


def wide_inputs(name, nt, family="se"):
    """-> (X, y, Xt, cov): family_inputs' data and covariance with nt test points."""
    X, y, _, cov = family_inputs(family, name)
    return X, y, wide_points(X, nt, FAMILIES[family][2](name)), cov


def wide_bcm_inputs(N, K):
    """-> (X, y, Xt, cov) of a BCM row of the wide tests."""
    X, y = synth(N, d=5, seed=N + K, scale=3.0)
    return X, y, wide_points(X, WIDE_NT_FAMILY, 3.0), SE(HP_BCM_WIDE)


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
