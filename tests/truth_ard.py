"""Extended-precision truth for the ARD kernel (one length scale per input dimension) -- TEST INFRASTRUCTURE, CPU,
numpy only; the factorisation pieces are those of tests/truth.py.

    theta = [log l_1 .. log l_d, log sigma_f, log sigma_n]                    (GPML covSEard's order; nh = d + 2)
    K     = sf2 exp(-1/2 sum_c ((x_ic - x_jc) w_c)^2) + sn2 I,   w_c = exp(-theta_c), sf2 = exp(2 theta_d), sn2 = exp(2 theta_{d+1})
    g_c   = 1/2 sum_ij W_ij Kf_ij ((x_ic - x_jc) w_c)^2,  g_d = sum W o Kf,  g_{d+1} = sn2 tr W      (gradients of -LL)
    LL, mean, var, cov as in tests/truth.py with this K.

The yardstick (`noise_level_ard`): the CPU oracle has one length scale, but the ARD model on X is the isotropic model
with theta_0 = 0 on the scaled copy X / l, which the oracle evaluates in the reference's order of operations.  Its g0
is then an evaluation of sum_c g_c; EVERY g_c is held to that yardstick (each is a partial sum of the same terms on
the same scale).  All gradient errors are relative to the largest of the d + 2 true components.
`standin_ard` is the independent fp64 evaluation (LAPACK / BLAS, weighted differences) from which F_ARD is set.
"""
import numpy as np

import truth
from conftest import HP_DENSE, synth
from truth import LD, LL_CONST, cholesky, gram_lower, permutations, tri_inverse

QUANTITIES = ("ll", "gc", "gf", "gn", "mean", "var")     # gc: the largest error over the d per-dimension components


def split(hp):
    hp = np.asarray(hp, dtype=np.float64)
    return hp[:-2], float(hp[-2]), float(hp[-1])


def wsqdist(A, B, w, per_dim=None):
    """sum_c ((a_ic - b_jc) w_c)^2 in the dtype of w, one feature at a time; per_dim(c, D2) sees every term."""
    S = np.zeros((A.shape[0], B.shape[0]), dtype=w.dtype)
    for c in range(A.shape[1]):
        D = (A[:, c][:, None] - B[:, c][None, :]) * w[c]
        D *= D
        if per_dim is not None:
            per_dim(c, D)
        S += D
    return S


class TruthARD:
    """Every checked quantity of one ARD expert in longdouble: n, d, sf2, sn2, w, K, L, T, Kinv, alpha, ll, grad[d + 2];
    predict(Xt) / joint(Xt, with_noise)."""

    def __init__(self, X, y, hp):
        truth.require_extended()
        th, tf, tn = split(hp)
        X = np.asarray(X, dtype=np.float64)
        self.X = X.astype(LD)
        yl = np.asarray(y, dtype=np.float64).astype(LD)
        n, d = X.shape
        assert len(th) == d
        self.n, self.d = n, d
        self.w = np.exp(-th.astype(LD))
        self.sf2, self.sn2 = np.exp(2 * LD(tf)), np.exp(2 * LD(tn))
        S = wsqdist(self.X, self.X, self.w)
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
        g = np.zeros(d + 2, dtype=LD)

        def per_dim(c, D2):
            g[c] = (WK * D2).sum() / 2
        wsqdist(self.X, self.X, self.w, per_dim)
        g[d], g[d + 1] = WK.sum(), self.sn2 * np.trace(W)
        self.grad, self.alpha, self.T, self.K, self.L, self.Kinv = g, alpha, T, K, L, Kinv

    def _cross(self, Xt):
        Xt = np.asarray(Xt, dtype=np.float64).reshape(-1, self.d).astype(LD)
        Ks = self.sf2 * np.exp(-wsqdist(Xt, self.X, self.w) / 2)
        return Xt, Ks, truth._mm(Ks, np.ascontiguousarray(self.T.T))

    def predict(self, Xt):
        _, Ks, Wt = self._cross(Xt)
        return Ks @ self.alpha, self.sf2 + self.sn2 - (Wt * Wt).sum(1)

    def joint(self, Xt, with_noise=True):
        Xt, Ks, Wt = self._cross(Xt)
        cov = self.sf2 * np.exp(-wsqdist(Xt, Xt, self.w) / 2) - Wt @ Wt.T
        if with_noise:
            cov[np.arange(len(cov)), np.arange(len(cov))] += self.sn2
        return Ks @ self.alpha, cov


def standin_ard(X, y, hp, Xt=None, solve=False):
    """The same quantities in fp64 through LAPACK / BLAS, differences weighted before they are squared.
    -> (ll, grad[d + 2], mean, var) (mean, var None without Xt), with solve=True also (alpha, K^-1)."""
    import scipy.linalg as sl
    th, tf, tn = split(hp)
    X = np.asarray(X, dtype=np.float64)
    n, d = X.shape
    w, sf2, sn2 = np.exp(-th), np.exp(2 * tf), np.exp(2 * tn)
    Kf = sf2 * np.exp(-wsqdist(X, X, w) / 2)
    K = Kf + sn2 * np.eye(n)
    L = np.linalg.cholesky(K)
    T = sl.solve_triangular(L, np.eye(n), lower=True)
    Ki = T.T @ T
    a = Ki @ y
    ll = -0.5 * (y @ a + 2 * np.log(np.diag(L)).sum() + n * LL_CONST)
    WK = (Ki - np.outer(a, a)) * Kf
    g = np.zeros(d + 2)

    def per_dim(c, D2):
        g[c] = (WK * D2).sum() / 2
    wsqdist(X, X, w, per_dim)
    g[d], g[d + 1] = WK.sum(), sn2 * np.trace(Ki - np.outer(a, a))
    m = v = None
    if Xt is not None:
        Ks = sf2 * np.exp(-wsqdist(np.asarray(Xt, dtype=np.float64), X, w) / 2)
        Wt = Ks @ T.T
        m, v = Ks @ a, sf2 + sn2 - (Wt * Wt).sum(1)
    out = (ll, g, m, v)
    return out + (a, Ki) if solve else out


# ---------------------------------------------------------------------------------------- errors and the yardstick
def scales_ard(hp, ll, grad, mean):
    gs = float(np.max(np.abs(grad)))
    sv = float(np.exp(2 * hp[-2]) + np.exp(2 * hp[-1]))
    return dict(ll=float(abs(ll)), gc=gs, gf=gs, gn=gs, mean=float(np.max(np.abs(mean))), var=sv, cov=sv)


def floors_ard(sc):
    u4 = 4 * 2.0 ** -52
    return dict(ll=u4, gc=u4, gf=u4, gn=u4, mean=u4 * sc["mean"], var=u4 * sc["var"], cov=u4 * sc["cov"])


def errors_ll_grad_ard(ll, grad, tll, tgrad):
    """LL relative to |LL|; gradient components relative to the largest of the d + 2 true ones (gc: the worst of the d
    per-dimension components)."""
    gs = np.max(np.abs(tgrad))
    d = len(tgrad) - 2
    g = np.asarray(grad).astype(LD)
    return dict(ll=float(abs(LD(ll) - tll) / abs(tll)), gc=float(np.max(np.abs(g[:d] - tgrad[:d])) / gs),
                gf=float(abs(g[d] - tgrad[d]) / gs), gn=float(abs(g[d + 1] - tgrad[d + 1]) / gs))


def errors_ard(ll, grad, mean, var, tll, tgrad, tmean, tvar):
    return dict(errors_ll_grad_ard(ll, grad, tll, tgrad), **truth.errors_pred(mean, var, tmean, tvar))


def scaled_problem(X, hp):
    """(X / l in fp64, [0, theta_d, theta_{d+1}]): the isotropic problem the oracle can evaluate."""
    th, tf, tn = split(hp)
    return np.ascontiguousarray(np.asarray(X, dtype=np.float64) / np.exp(th)), [0.0, tf, tn]


def noise_level_ard(oracle, X, y, hp, Xt, tll, tgrad, tmean, tvar):
    """-> (noise, first, rest) per quantity of QUANTITIES, as truth.noise_level: the oracle's largest error against the
    ARD truth over the data as given and the 7 permutations, evaluated on the scaled copy.  Its g0 evaluates
    sum_c g_c: that error is the yardstick "gc" of every per-dimension component."""
    Xs, hpi = scaled_problem(X, hp)
    Xts = scaled_problem(Xt, hp)[0]
    d = len(tgrad) - 2
    gs = np.max(np.abs(tgrad))
    tsum = tgrad[:d].sum()

    def one(idx):
        Xp, yp = np.ascontiguousarray(Xs[idx]), np.ascontiguousarray(y[idx])
        ll, g = oracle.loglik_grad(Xp, yp, hpi)
        m, v = oracle.predict(Xp, yp, hpi, Xts)
        e = dict(ll=float(abs(LD(ll) - tll) / abs(tll)), gc=float(abs(LD(g[0]) - tsum) / gs),
                 gf=float(abs(LD(g[1]) - tgrad[d]) / gs), gn=float(abs(LD(g[2]) - tgrad[d + 1]) / gs))
        return dict(e, **truth.errors_pred(m, v, tmean, tvar))
    E = list(truth._pool().map(one, permutations(len(y))))
    return {q: max(e[q] for e in E) for q in QUANTITIES}, E[0], {q: max(e[q] for e in E[1:]) for q in QUANTITIES}


def noise_level_solve_ard(oracle, X, y, hp, t, rows):
    """alpha and rows of K^-1: the oracle's potrs / potri on its own K of the scaled copy (truth.noise_level_solve)."""
    Xs, hpi = scaled_problem(X, hp)
    return truth.noise_level_solve(oracle, Xs, y, hpi, t, rows)


# ---------------------------------------------------------------------------------------- the cases
# err_gpu <= F_ARD max(noise, floor): the next power of two at or above twice the largest stand-in ratio over ARD_CASES
# (tests/test_truth_ard_cpu.py measures it on the CPU; docs/ACCURACY.md holds the table) -- never from the GPU's errors.
F_ARD = 32        # largest stand-in ratio: 8.70, the predictive mean at cond(K) ~ 1e6 (twice that is 17.4)
F_SOLVE = truth.F_SOLVE
YARDSTICK_CAP = truth.YARDSTICK_CAP
NT = truth.NT

# name -> (n, d, theta_l, theta_f, theta_n, box half-width of synth, shift added to X and Xt)
ARD_CASES = {
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
JOINT_CASES = ("n65_d2", "n257_d3", "n1025_dense", "n1300_d6")       # the two smallest and the two largest


def ard_inputs(name):
    """-> (X, y, Xt, hp): synth data of the case, 64 test points in the same box, one of them a training row."""
    n, d, th, tf, tn, scale, shift = ARD_CASES[name]
    X, y = synth(n, d=d, seed=3 * n + d, scale=scale)
    Xt = synth(NT, d=d, seed=7, scale=scale)[0]
    Xt[5] = X[n // 2]
    return np.ascontiguousarray(X + shift), y, np.ascontiguousarray(Xt + shift), list(th) + [tf, tn]
