"""Extended-precision truth for the Matern 3/2 and 5/2 kernels -- TEST INFRASTRUCTURE, CPU, numpy only; the
factorisation pieces are those of tests/truth.py.

    theta = [log l, log sigma_f, log sigma_n]                                  (the isotropic three; GPML covMaterniso)
    s = |x - x'|^2 / l^2,  r = sqrt(s),  sf2 = exp(2 theta_1),  sn2 = exp(2 theta_2)
    kind 1 (nu = 3/2): a = sqrt(3) r,  Kf = sf2 (1 + a) exp(-a),            dK/dtheta_0 = sf2 a^2 exp(-a)
    kind 2 (nu = 5/2): a = sqrt(5) r,  Kf = sf2 (1 + a + a^2/3) exp(-a),    dK/dtheta_0 = sf2 (a^2/3) (1 + a) exp(-a)
    K = Kf + sn2 I;  grad = (1/2 sum W o dK, sum W o Kf, sn2 tr W)  (of -LL),  W = K^-1 - alpha alpha^T
    LL, mean, var, cov as in tests/truth.py with this K.

The yardstick (`noise_level_matern`): the CPU oracle evaluates the squared exponential only, but it factors, inverts
and solves a caller's matrix in the reference's order of operations.  So the Matern K is formed in fp64 numpy and
handed to the oracle's linear algebra: LL from chol_and_det, the traces from K_inverse and Kinvy, the mean from
Ks Kinvy, the variance from Ks K^-1 Ks^T -- on the data as given and on truth.permutations, largest error against the
truth.  `standin_matern` is the independent fp64 evaluation (LAPACK / BLAS) from which F_MATERN is set.
`entry_fp64` restates the kernels' per-entry arithmetic (kernels.hip: matern_entry) operation by operation in fp64
numpy; `k_entry_bound` is the rounding count it and the GPU's K entries are held to.
"""
import numpy as np

import truth
from truth import LD, LL_CONST, U, cholesky, gram_lower, permutations, tri_inverse

SE, MATERN32, MATERN52 = 0, 1, 2
KINDS = (MATERN32, MATERN52)
KIND_NAMES = {MATERN32: "matern32", MATERN52: "matern52"}
QUANTITIES = truth.QUANTITIES
C2 = {MATERN32: 3, MATERN52: 5}            # a = sqrt(C2) r


def kernel_ld(S, sf2, kind):
    """(Kf, dK/dlog l) from s = |x - x'|^2 / l^2, in the dtype of S (longdouble for the truth)."""
    a = np.sqrt(C2[kind] * S)
    e = np.exp(-a)
    if kind == MATERN32:
        return sf2 * (1 + a) * e, sf2 * a * a * e
    t = a * a / 3
    return sf2 * (1 + a + t) * e, sf2 * t * (1 + a) * e


class TruthMatern:
    """Every checked quantity of one Matern expert in longdouble: n, l2, sf2, sn2, K, L, T, Kinv, alpha, ll, grad[3];
    predict(Xt) / joint(Xt, with_noise)."""

    def __init__(self, X, y, hp, kind, keep=True):
        truth.require_extended()
        assert kind in KINDS
        X = np.asarray(X, dtype=np.float64)
        self.kind = kind
        self.X = X.astype(LD)
        yl = np.asarray(y, dtype=np.float64).astype(LD)
        n = self.n = X.shape[0]
        self.l2, self.sf2, self.sn2 = truth.hyper(hp)
        Kf, dK = kernel_ld(truth.sqdist(self.X, self.X) / self.l2, self.sf2, kind)
        K = Kf.copy()
        K[np.arange(n), np.arange(n)] += self.sn2
        L = cholesky(K)
        T = tri_inverse(L)
        Kinv = gram_lower(T)
        alpha = Kinv @ yl
        self.ll = -LD(0.5) * (yl @ alpha + 2 * np.log(np.diag(L)).sum() + n * LD(LL_CONST))
        W = Kinv - np.outer(alpha, alpha)
        self.grad = np.array([(W * dK).sum() / 2, (W * Kf).sum(), self.sn2 * np.trace(W)], dtype=LD)
        self.alpha, self.T = alpha, T
        if keep:
            self.K, self.L, self.Kinv = K, L, Kinv

    def kf(self, A, B):
        return kernel_ld(truth.sqdist(A, B) / self.l2, self.sf2, self.kind)[0]

    def _cross(self, Xt):
        Xt = np.asarray(Xt, dtype=np.float64).reshape(-1, self.X.shape[1]).astype(LD)
        Ks = self.kf(Xt, self.X)
        return Xt, Ks, truth._mm(Ks, np.ascontiguousarray(self.T.T))

    def cross(self, Xt):
        return self._cross(Xt)[1]

    def predict(self, Xt):
        _, Ks, Wt = self._cross(Xt)
        return Ks @ self.alpha, self.sf2 + self.sn2 - (Wt * Wt).sum(1)

    def joint(self, Xt, with_noise=True):
        Xt, Ks, Wt = self._cross(Xt)
        cov = self.kf(Xt, Xt) - Wt @ Wt.T
        if with_noise:
            cov[np.arange(len(cov)), np.arange(len(cov))] += self.sn2
        return Ks @ self.alpha, cov


def bcm_truth_matern(X, y, hp, K, Xt, kind):
    """truth.bcm_truth with the Matern truth: LL and gradient summed over the row split, product of experts."""
    ll, grad, sp, spm = LD(0), np.zeros(3, dtype=LD), 0, 0
    for off, rows in truth.bcm_rows(len(y), K):
        t = TruthMatern(X[off: off + rows], y[off: off + rows], hp, kind, keep=False)
        m, v = t.predict(Xt)
        ll, grad, sp, spm = ll + t.ll, grad + t.grad, sp + 1 / v, spm + m / v
    return dict(ll=ll, grad=grad, mean=spm / sp, var=1 / sp)


# ---------------------------------------------------------------------------------------- fp64 pieces
def sqdist64(A, B):
    """|a_i - b_j|^2 in fp64, one feature at a time in index order, no FMA: sqdist_4x4's sequence."""
    S = np.zeros((A.shape[0], B.shape[0]))
    for k in range(A.shape[1]):
        D = A[:, k][:, None] - B[:, k][None, :]
        S = S + D * D
    return S


SQRT3, SQRT5, THIRD = 1.7320508075688772, 2.23606797749979, 0.3333333333333333     # the kernels' fp64 constants


def entry_fp64(d2, l2, sf2, kind):
    """matern_entry of kernels.hip in fp64 numpy, one rounding per line as there: -> (kf, dk).  div_by is a correctly
    rounded quotient, numpy's sqrt is correctly rounded, every product and sum is its own ufunc call (no FMA)."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        s = d2 / l2
        a = (SQRT3 if kind == MATERN32 else SQRT5) * np.sqrt(s)
        e = np.exp(-a)
        p1 = 1.0 + a
        if kind == MATERN32:
            p, q = p1, a * a
        else:
            t = (a * a) * THIRD
            p, q = p1 + t, t * p1
        dead = e == 0.0
        return np.where(dead, 0.0, sf2 * (p * e)), np.where(dead, 0.0, sf2 * (q * e))


# The K-entry bound, relative to the true Kf entry, in units of u = 2^-53 (a correctly rounded operation: 1 u; exp of
# libm / the device library: 1 ulp = 2 u), counted along matern_entry:
#   d2   each term (x - y)^2: difference 1 u, square 2 u + 1 u; the d-term sum of positive terms adds d - 1       d + 2
#   l2   exp(2 theta_0) on the host                                                                                    2
#   s    one (correctly rounded) division                                                                              1
#   r    the square root halves the incoming (d + 5) u and adds its own rounding                         (d + 5) / 2 + 1
#   a    the constant RN(sqrt 3 | sqrt 5) and one multiply                                                             2
#        => eps_a = (d + 11) / 2 u
#   e    exp's argument error is amplified by a: a eps_a; its own error                                                2
#   p    no cancellation (all terms positive): propagated eps_a dlog p / dlog a, which is a / (1 + a) <= 1 for 3/2 and
#        (a + 2 a^2/3) / (1 + a + a^2/3) <= 2 for 5/2; own roundings: 3/2 one sum (1); 5/2 a a (1), the constant RN(1/3)
#        (1), its multiply (1), then two sums of positive terms (max of the parts' + 1 each: 3 + 1 = 4)            1 | 4
#   kf   p e (1), sf2 (...) (1), sf2 = exp(2 theta_1) on the host (2)                                                  4
# Sum: 3/2: (7 + (a + 1) (d + 11) / 2) u;  5/2: (10 + (a + 2) (d + 11) / 2) u <= (10 + (1 + a) (d + 11)) u.
# Form (c0 + c1 (1 + a) (d + c2)) u:
K_BOUND = {MATERN32: (7.0, 0.5, 11.0), MATERN52: (10.0, 1.0, 11.0)}


def k_entry_bound(a, d, kind):
    """Relative bound on an fp64 Kf entry at a = sqrt(3 | 5) r (array or scalar) with d features."""
    c0, c1, c2 = K_BOUND[kind]
    return (c0 + c1 * (1.0 + np.asarray(a, dtype=np.float64)) * (d + c2)) * U


def a_of(A, B, hp, kind):
    """a = sqrt(3 | 5) |x - x'| / l in fp64, for k_entry_bound."""
    return np.sqrt(C2[kind] * sqdist64(np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64))
                   / np.exp(2 * hp[0]))


def standin_matern(X, y, hp, Xt, kind, solve=False):
    """The quantities in fp64 through LAPACK / BLAS, the kernel function in its textbook form (one sqrt of 3 s or 5 s,
    a^2 / 3 by division).  -> (ll, grad, mean, var), with solve=True also (alpha, K^-1)."""
    import scipy.linalg as sl
    l2, sf2, sn2 = np.exp(2 * np.asarray(hp, dtype=np.float64))
    X = np.asarray(X, dtype=np.float64)
    n = len(y)
    Kf, dK = kernel_ld(sqdist64(X, X) / l2, sf2, kind)
    K = Kf + sn2 * np.eye(n)
    L = np.linalg.cholesky(K)
    T = sl.solve_triangular(L, np.eye(n), lower=True)
    Ki = T.T @ T
    a = Ki @ y
    ll = -0.5 * (y @ a + 2 * np.log(np.diag(L)).sum() + n * LL_CONST)
    W = Ki - np.outer(a, a)
    g = np.array([(W * dK).sum() / 2, (W * Kf).sum(), sn2 * np.trace(W)])
    Ks = kernel_ld(sqdist64(np.asarray(Xt, dtype=np.float64), X) / l2, sf2, kind)[0]
    Wt = Ks @ T.T
    out = (ll, g, Ks @ a, sf2 + sn2 - (Wt * Wt).sum(1))
    return out + (a, Ki) if solve else out


def standin_objective(X, y, kind):
    """theta -> (-LL, gradient) of the fp64 stand-in: the objective cugp_cg_minimize is driven by in the optimiser test."""
    Xt = np.asarray(X[:1], dtype=np.float64)

    def fn(th):
        try:
            ll, g, _, _ = standin_matern(X, y, list(th), Xt, kind)
        except np.linalg.LinAlgError:
            return float("nan"), np.full(3, np.nan)
        return -ll, g
    return fn


# ---------------------------------------------------------------------------------------- the yardstick
def oracle_eval(oracle, X, y, hp, Xt, kind, solve=False):
    """The Matern K in fp64 numpy through the oracle's linear algebra -> (ll, grad, mean, var) (+ alpha, K^-1)."""
    l2, sf2, sn2 = np.exp(2 * np.asarray(hp, dtype=np.float64))
    n = len(y)
    Kf, dK = kernel_ld(sqdist64(X, X) / l2, sf2, kind)
    K = Kf + sn2 * np.eye(n)
    quad, logdet = oracle.chol_and_det(K, y)
    ll = -0.5 * (quad + logdet + n * LL_CONST)
    Ki = oracle.K_inverse(K)
    a = oracle.Kinvy(K, y)
    W = Ki - np.outer(a, a)
    g = np.array([(W * dK).sum() / 2, (W * Kf).sum(), sn2 * np.trace(W)])
    Ks = kernel_ld(sqdist64(np.asarray(Xt, dtype=np.float64), X) / l2, sf2, kind)[0]
    out = (ll, g, Ks @ a, sf2 + sn2 - ((Ks @ Ki) * Ks).sum(1))
    return out + (a, Ki) if solve else out


def noise_level_matern(oracle, X, y, hp, Xt, kind, t, tmean, tvar, rows=None):
    """-> (noise, first, rest, solve): per quantity of QUANTITIES the largest error of `oracle_eval` against the truth t
    over the data as given and the 7 permutations, the error on the data as given alone, the largest over the
    permutations alone (as truth.noise_level); solve: the same yardstick for alpha and the chosen rows of K^-1 (as
    truth.noise_level_solve), from the same evaluations."""
    n = len(y)
    rows = truth.solve_rows(n) if rows is None else rows
    kmax, amax = np.max(np.abs(t.Kinv)), np.max(np.abs(t.alpha))

    def one(idx):
        inv = np.empty(n, dtype=np.int64)
        inv[idx] = np.arange(n)
        ll, g, m, v, a, Ki = oracle_eval(oracle, np.ascontiguousarray(X[idx]), np.ascontiguousarray(y[idx]), hp, Xt,
                                         kind, solve=True)
        e = truth.errors(ll, g, m, v, t.ll, t.grad, tmean, tvar)
        e["alpha"] = float(np.max(np.abs(a[inv].astype(LD) - t.alpha)) / amax)
        e["kinv"] = float(np.max(np.abs(Ki[np.ix_(inv[rows], inv)].astype(LD) - t.Kinv[rows])) / kmax)
        return e
    E = list(truth._pool().map(one, permutations(n)))
    return ({q: max(e[q] for e in E) for q in QUANTITIES}, E[0], {q: max(e[q] for e in E[1:]) for q in QUANTITIES},
            {q: max(e[q] for e in E) for q in truth.SOLVE_QUANTITIES})


# ---------------------------------------------------------------------------------------- the cases
# err_gpu <= F_MATERN max(noise, floor): the next power of two at or above twice the largest stand-in ratio over
# MATERN_CASES x KINDS and all eight orderings (tests/test_truth_matern_cpu.py measures it on the CPU; docs/ACCURACY.md
# holds the table) -- never from the GPU's errors.
F_MATERN = 16      # largest stand-in ratio: 5.23, the predictive mean of n257_d3 at nu = 5/2 (twice that is 10.5)
F_SOLVE = truth.F_SOLVE
YARDSTICK_CAP = truth.YARDSTICK_CAP
NT = truth.NT
MATERN_CASES = tuple(list(truth.LIVE_CASES)[list(truth.LIVE_CASES).index("n65"):])     # truth.LIVE_CASES from n65 up
JOINT_CASES = truth.JOINT_CASES
matern_inputs = truth.live_inputs
