"""ARD x Matern 3/2 and 5/2 (GPML covMaternard; include/cugp.h: cugp_create_ard_kernel) -- TEST INFRASTRUCTURE, CPU, numpy
only; a plain module beside tests/truth.py, tests/accuracy.py and the truth_* modules, which it imports and leaves as
they are.

    theta = [log l_1 .. log l_d, log sf, log sn],  w_c = exp(-theta_c),  u_c = (x_c - x'_c) w_c,  s = sum_c u_c^2
    a = sqrt(3 s) | sqrt(5 s),  e = exp(-a)
    3/2:  Kf = sf2 (1 + a) e             H = 3 sf2 e
    5/2:  Kf = sf2 (1 + a + a^2/3) e     H = (5/3) sf2 (1 + a) e
    dk/dtheta_c = H u_c^2,   g_c = 1/2 sum W o H o u_c^2,   dk/dx*_c = -H (x*_c - x_c) w_c^2

  descriptor  ARDMatern(hp, kind): the interface of truth.ARD / truth.Matern (train, k, fp64, evaluator), the formulas in
              textbook form in the descriptor's dtype; quantities and factor are truth.ARD's (QUANTITIES_ARD, F_ARD).
  yardstick   as truth.Matern.evaluator: K formed in fp64 numpy, handed to the oracle's chol_and_det / K_inverse / Kinvy;
              the gradient has d + 2 entries, so truth.errors_ll_grad compares every g_c.
  per entry   `entry_fp64` restates the kernels' arithmetic (kernels.hip: matern_entry at s = the weighted distance,
              matern_entry's H) rounding by rounding; `k_entry_bound` is the count it and the GPU's K entries are
              held to.
  families    "matern32_ard" / "matern52_ard" are added to truth.FAMILIES when this module is imported (the cases are
              truth.ARD_CASES' data and theta), so accuracy.live, truth_targets.case and truth_append's helpers take them.
  predict-grad  tests/truth_predict_grad.py picks G and s_c by the descriptor's class; its helpers that do are restated here
              (`gradients` and what calls it), the rest (sums, errors, hold, ratios, the sanity check) is used as it is.
"""
import numpy as np

import accuracy
import truth
import truth_matern as tm
import truth_predict_grad as tpg
from truth import C2, KIND_NAMES, KINDS, LD, MATERN32, MATERN52, U  # noqa: F401

FAMILY = {MATERN32: "matern32_ard", MATERN52: "matern52_ard"}


def parts(S, sf2, kind):
    """(Kf, H) from the weighted squared distance S, in its dtype: the textbook form."""
    a = np.sqrt(C2[kind] * S)
    e = np.exp(-a)
    if kind == MATERN32:
        return sf2 * (1 + a) * e, 3 * sf2 * e
    T = S.dtype.type
    return sf2 * (1 + a + a * a / 3) * e, (T(5) / T(3)) * sf2 * (1 + a) * e


class ARDMatern:
    """Matern 3/2 (kind 1) and 5/2 (kind 2) with one length scale per input dimension at theta = [log l_1 .. log l_d,
    log sf, log sn]; differences are weighted before they are squared."""
    quantities, F = truth.QUANTITIES_ARD, truth.F_ARD

    def __init__(self, hp, kind, dtype=LD):
        assert kind in KINDS
        self.hp, self.kind, self.dtype = [float(h) for h in hp], kind, dtype
        th = np.asarray(self.hp[:-2], dtype=np.float64)
        self.w = np.exp(-th.astype(dtype))
        self.sf2, self.sn2 = np.exp(2 * dtype(self.hp[-2])), np.exp(2 * dtype(self.hp[-1]))

    def fp64(self):
        return ARDMatern(self.hp, self.kind, np.float64)

    def train(self, X, mutate=None):
        """-> (Kf, terms); mutate "kf_for_h": g_c from Kf in place of H (the CPU suite shows it leaves the bound)."""
        assert X.shape[1] == len(self.w)
        Kf, H = parts(truth.wsqdist(X, X, self.w), self.sf2, self.kind)
        if mutate == "kf_for_h":
            H = Kf

        def terms(W):
            WH = W * H
            g = [None] * len(self.w)

            def per_dim(c, D2):
                g[c] = (WH * D2).sum() / 2
            truth.wsqdist(X, X, self.w, per_dim)          # the dimensions a second time, W o H fixed
            return tuple(g) + ((W * Kf).sum(),)
        return Kf, terms

    def k(self, A, B):
        return parts(truth.wsqdist(A, B, self.w), self.sf2, self.kind)[0]

    def grad_factors(self, Xt, X):
        """-> (G [nt, n], s [d]) of dk/dx*_c = -G (x*_c - x_c) s_c."""
        T = self.dtype
        return parts(truth.wsqdist(np.asarray(Xt, dtype=T), np.asarray(X, dtype=T), self.w), self.sf2, self.kind)[1], \
            self.w * self.w

    def evaluator(self, oracle, X, Xt, solve=False):
        """truth.Matern.evaluator's construction: this family's K in fp64 numpy through the oracle's factorisation,
        inverse and solve (the reference's order of operations)."""
        c = self.fp64()

        def evaluate(Xp, yp):
            n = len(yp)
            Kf, terms = c.train(Xp)
            K = Kf + c.sn2 * np.eye(n)
            quad, logdet = oracle.chol_and_det(K, yp)
            ll = -0.5 * (quad + logdet + n * truth.LL_CONST)
            Ki = oracle.K_inverse(K)
            a = oracle.Kinvy(K, yp)
            W = Ki - np.outer(a, a)
            g = np.array(terms(W) + (c.sn2 * np.trace(W),))
            Ks = c.k(Xt, Xp)
            out = (ll, g, Ks @ a, c.sf2 + c.sn2 - ((Ks @ Ki) * Ks).sum(1))
            return out + (a, Ki) if solve else out
        return X, evaluate


class _Mutated(ARDMatern):
    """The descriptor with a mutation of `train` (for the CPU suite's stand-in runs)."""

    def __init__(self, hp, kind, mutate, dtype=LD):
        ARDMatern.__init__(self, hp, kind, dtype)
        self.mutate = mutate

    def fp64(self):
        return _Mutated(self.hp, self.kind, self.mutate, np.float64)

    def train(self, X, mutate=None):
        return ARDMatern.train(self, X, self.mutate)


# ---------------------------------------------------------------------------------------- the cases
CASES = tuple((name, kind) for name in truth.ARD_CASES for kind in KINDS)       # truth.ARD_CASES' data and theta, both kinds
for _kind, _fam in FAMILY.items():
    truth.FAMILIES.setdefault(_fam, (truth.ard_inputs, (lambda k: lambda hp: ARDMatern(hp, k))(_kind),
                                     lambda name: truth.ARD_CASES[name][5]))


def inputs(name, kind):
    """-> (X, y, Xt, cov) of a case of truth.ARD_CASES at a Matern kind."""
    return truth.family_inputs(FAMILY[kind], name)


def live(oracle, name, kind):
    """accuracy.live of the case: truth, predictions, yardsticks (alpha and K^-1 included) and floors, once per process."""
    return accuracy.live(oracle, FAMILY[kind], name)


# ---------------------------------------------------------------------------------------- per-entry arithmetic
FIVE_THIRDS = 1.6666666666666667       # the kernels' fp64 constant RN(5/3)


def wsqdist64(A, B, w):
    """sum_c ((a_ic - b_jc) w_c)^2 in fp64: the difference, weighted, squared, added in index order, no FMA --
    sqdist_4x4<true>'s sequence."""
    S = np.zeros((A.shape[0], B.shape[0]))
    for c in range(A.shape[1]):
        D = (A[:, c][:, None] - B[:, c][None, :]) * w[c]
        S = S + D * D
    return S


def entry_fp64(s, sf2, kind):
    """The kernels' entry from the weighted squared distance s, one rounding per line as there: -> (kf, hh).  kf is
    matern_entry's (no division: s is used directly), hh = sf2 (3 e) | sf2 ((RN(5/3) (1 + a)) e); e == 0 selects exact
    zeros for both."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        a = (tm.SQRT3 if kind == MATERN32 else tm.SQRT5) * np.sqrt(s)
        e = np.exp(-a)
        p1 = 1.0 + a
        if kind == MATERN32:
            p, q = p1, 3.0
        else:
            p, q = p1 + (a * a) * tm.THIRD, FIVE_THIRDS * p1
        dead = e == 0.0
        return np.where(dead, 0.0, sf2 * (p * e)), np.where(dead, 0.0, sf2 * (q * e))


# The K-entry bound, relative to the true Kf entry, in units of u = 2^-53 -- truth_matern.K_BOUND's count with the
# weighted distance in place of |x - x'|^2 / l^2:
#   u_c  the difference 1 u, w_c = exp(-theta_c) on the host 2 u, their product 1 u                                   4
#   s    each term u_c^2: 2 * 4 u + 1 u; the d-term sum of positive terms adds d - 1                              d + 8
#        (isotropic: d + 2 for the sum, 2 for l^2, 1 for the division = d + 5; there is no division here)
#   r    the square root halves the incoming error and adds its own rounding                           (d + 8) / 2 + 1
#   a    the constant RN(sqrt 3 | sqrt 5) and one multiply                                                           2
#        => eps_a = (d + 14) / 2 u
#   e, p, kf  as truth_matern: a eps_a + 2;  eps_a (<= 1 | <= 2) + (1 | 4);  4
# Sum: 3/2: (7 + (a + 1) (d + 14) / 2) u;  5/2: (10 + (a + 2) (d + 14) / 2) u <= (10 + (1 + a) (d + 14)) u.
K_BOUND = {MATERN32: (7.0, 0.5, 14.0), MATERN52: (10.0, 1.0, 14.0)}


def k_entry_bound(a, d, kind):
    """Relative bound on an fp64 Kf entry at a = sqrt(3 | 5 s) (array or scalar) with d features."""
    c0, c1, c2 = K_BOUND[kind]
    return (c0 + c1 * (1.0 + np.asarray(a, dtype=np.float64)) * (d + c2)) * U


def a_of(A, B, cov):
    """a = sqrt(3 | 5 s) of the weighted distance in fp64, for k_entry_bound."""
    w = np.asarray(cov.w, dtype=np.float64)
    return np.sqrt(C2[cov.kind] * wsqdist64(np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64), w))


def entry_excess(Kf, A, B, cov):
    """Largest |Kf - truth| / (truth * k_entry_bound) over the entries of an fp64 Kf = k(A, B) without noise (true entries
    of 0 -- an exp that underflowed -- must be met exactly)."""
    t = ARDMatern(cov.hp, cov.kind).k(np.asarray(A, dtype=np.float64).astype(LD), np.asarray(B, dtype=np.float64).astype(LD))
    err = np.abs(np.asarray(Kf).astype(LD) - t)
    bnd = t * k_entry_bound(a_of(A, B, cov), np.asarray(A).shape[1], cov.kind)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, LD(0), err / bnd)
    return float(np.max(r))


# ---------------------------------------------------------------------------------------- gradients w.r.t. test inputs
def gradients(cov, Xt, X, alpha, V, coordinate=False):
    """truth_predict_grad.gradients with the descriptor's own (G, s_c)."""
    T = cov.dtype
    Xt, X = np.asarray(Xt, dtype=T), np.asarray(X, dtype=T)
    G, s = cov.grad_factors(Xt, X)
    return -tpg.sums(G * alpha[None, :], Xt, X, s, coordinate), 2 * tpg.sums(G * V, Xt, X, s, coordinate)


def grad_case_at(oracle, cov, X, y, Xt, t):
    """truth_predict_grad.case_at restated on `gradients` above: truth from the kept K^-1 in longdouble, the yardstick
    over truth.permutations (alpha from the evaluator, V by two substitutions with the oracle's factor), 4-ulp floors."""
    import scipy.linalg as sl
    Xl = np.asarray(Xt, dtype=np.float64).astype(LD)
    tdm, tdv = gradients(t.cov, Xl, t.X, t.alpha, truth._mm(t.cov.k(Xl, t.X), t.Kinv))
    Xe, evaluate = cov.evaluator(oracle, X, Xt, solve=True)
    c64 = cov.fp64()
    X64, Xt64 = np.asarray(X, dtype=np.float64), np.asarray(Xt, dtype=np.float64)

    def one(idx):
        Xp = np.ascontiguousarray(X64[idx])
        a = evaluate(np.ascontiguousarray(Xe[idx]), np.ascontiguousarray(y[idx]))[4]
        Kf, _ = c64.train(Xp)
        L = np.asarray(oracle.cholesky(Kf + c64.sn2 * np.eye(len(idx))))
        Ks = c64.k(Xt64, Xp)
        V = sl.solve_triangular(L.T, sl.solve_triangular(L, Ks.T, lower=True), lower=False).T
        return tpg.errors(*gradients(c64, Xt64, Xp, np.asarray(a), V), tdm, tdv)
    E = list(truth._pool().map(one, truth.permutations(len(y))))
    Q = tpg.QUANTITIES
    floor = dict(dmean=truth.U4 * float(np.max(np.abs(tdm))), dvar=truth.U4 * float(np.max(np.abs(tdv))))
    return dict(X=X, y=y, Xt=Xt, cov=cov, t=t, tdm=tdm, tdv=tdv, noise={q: max(e[q] for e in E) for q in Q},
                first={q: E[0][q] for q in Q}, rest={q: max(e[q] for e in E[1:]) for q in Q}, floor=floor)


_GRAD_CASES = {}


def grad_case(oracle, name, kind, nt=None):
    """Gradients of the prediction of a live case at its 64 test points, or at nt points (truth.wide_inputs), once per
    process."""
    key = (name, kind, nt)
    if key not in _GRAD_CASES:
        c = live(oracle, name, kind)
        Xt = c["Xt"] if nt is None else truth.wide_inputs(name, nt, FAMILY[kind])[2]
        _GRAD_CASES[key] = grad_case_at(oracle, c["cov"], c["X"], c["y"], Xt, c["t"])
    return _GRAD_CASES[key]


def grad_standin(cov, X, y, Xt):
    """truth_predict_grad.standin with `gradients` above: alpha = T^T (T y), V = (Ks T^T) T in LAPACK / BLAS order."""
    import scipy.linalg as sl
    c64 = cov.fp64()
    X, Xt = np.asarray(X, dtype=np.float64), np.asarray(Xt, dtype=np.float64)
    Kf, _ = c64.train(X)
    L = np.linalg.cholesky(Kf + c64.sn2 * np.eye(len(y)))
    T = sl.solve_triangular(L, np.eye(len(y)), lower=True)
    Ks = c64.k(Xt, X)
    return gradients(c64, Xt, X, T.T @ (T @ y), (Ks @ T.T) @ T)


# ---------------------------------------------------------------------------------------- the product of experts
def bcm_case_at(oracle, cov, X, y, parts_, Xt):
    """truth_ard_bcm.case_at's form with this family's evaluator (that module scales the data for the oracle's isotropic
    SE, which has no Matern): truth expert by expert in longdouble, truth.noise_level of the experts' fp64 yardstick
    evaluations combined by truth.poe, the rows permuted inside their own expert."""
    def expert(Xk, yk):
        t = truth.Truth(Xk, yk, cov, keep=False)
        return (t.ll, t.grad) + t.predict(Xt)
    tb = dict(zip(("ll", "grad", "mean", "var"), truth.poe(parts_, expert)(X, y)))
    evaluate = truth.poe(parts_, cov.evaluator(oracle, X, Xt)[1])
    noise, first, rest = truth.noise_level(cov, evaluate, X, y, tb["ll"], tb["grad"], tb["mean"], tb["var"], parts=parts_)
    return dict(X=X, y=y, Xt=Xt, cov=cov, parts=parts_, tb=tb, noise=noise, first=first, rest=rest,
                floor=truth.floors(cov, truth.scales(cov, tb["ll"], tb["grad"], tb["mean"])))
