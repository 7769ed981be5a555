"""Leave-one-out cross-validation (cugp_loo, cugp_loo_predict): the truth, the yardstick, the stand-in and the factors of
its tests -- TEST INFRASTRUCTURE, CPU, numpy only; a plain module beside tests/truth.py and tests/accuracy.py, which it
imports and leaves as they are.

With kappa_i = [K^-1]_ii (Rasmussen & Williams, GPML 5.10-5.13) and c = truth.LL_CONST:

    mu_i = y_i - alpha_i / kappa_i,  var_i = 1 / kappa_i,  logp_i = 1/2 log kappa_i - alpha_i^2 / (2 kappa_i) - c / 2
    L_LOO = sum_i logp_i
    a = alpha / kappa,  c_i = (1 + alpha_i^2 / kappa_i) / kappa_i,  b = K^-1 a,  P = K^-1 diag(c) K^-1
    W_loo = P - b alpha' - alpha b',   grad(-L_LOO) = (the family's terms(W_loo), sn2 tr W_loo)

  truth      `truth_of`: in longdouble from the cached truth of a case (accuracy.live: Kinv, alpha, cov.train(X) and its
             terms(W)), the convention of truth_targets.truth_of.  tests/test_truth_loo_cpu.py checks it against actually
             deleting each point (`brute`) and against central differences of that objective.
  yardstick  `textbook`: GPML 5.12-5.13 in fp64 with an explicit dK_j per hyper-parameter (one N^3 product each), K^-1 and
             alpha from the CPU oracle's potri / potrs, over the data as given and truth.permutations.
  stand-in   `standin`: the fused formulation in fp64, LAPACK / BLAS order (B = K^-1 diag(sqrt c), P = B B', b, W_loo, the
             family's terms) -- what the library computes, on another arithmetic.
  errors     L_LOO relative; every gradient component relative to max|g| (truth.errors_ll_grad's quantities); mu and logp
             the largest absolute error; var the largest absolute error, floored at 4 ulp of sf2 + sn2
  bound      F_LOO[family] max(yardstick, 4 ulp of the quantity's scale); F_LOO is fixed below from the stand-in's ratios
             measured on the CPU (docs/ACCURACY.md has the table), never from the GPU's errors.
"""
import numpy as np

import accuracy
import truth
import truth_ard_matern as tam  # noqa: F401  (adds "matern52_ard" to truth.FAMILIES)
from conftest import HP_DEFAULT, synth

LD = truth.LD
U4 = truth.U4

# (family, case): what each covers is in tests/test_gpu_loo.py
CASES = (
    ("se", "n65"),
    ("se", "n128"),
    ("se", "n257_d3"),
    ("se", "n384_cond1e6"),
    ("matern32", "n65"),
    ("matern52", "n300_d17"),
    ("ard", "n257_d3"),
    ("ard", "n300_d17"),
    ("matern52_ard", "n257_d3"),
    ("se", "n1300_d6"),
    ("se", "n1"),                     # below / at one 64-row build tile: whole tiles of the padded matrix are padding
    ("se", "n2"),
    ("se", "n63"),
    ("se", "n64"),
    ("matern32", "n63"),
    ("ard", "n1_d2"),
    ("ard", "n2_d2"),
    ("ard", "n63_d2"),
    ("matern52_ard", "n63_d2"),
)
POINT_QUANTITIES = ("mu", "var", "logp")

# The larger of the family's existing factor and truth.factor_rule of the largest stand-in / yardstick ratio over CASES
# (tests/test_truth_loo_cpu.py measures and asserts; docs/ACCURACY.md: the table).
EXISTING = {"se": truth.F, "matern32": truth.F_MATERN, "matern52": truth.F_MATERN, "ard": truth.F_ARD,
            "matern52_ard": truth.F_ARD}
# Largest stand-in ratios measured: se 9.53 (mu of n384_cond1e6; factor_rule 32, above the family's 8), matern32 0.82,
# matern52 1.08, ard 1.82, matern52_ard 1.22 (factor_rule 2 to 4: the existing factors stand).
F_LOO = dict(EXISTING, se=32)

N128 = (128, 2, HP_DEFAULT, 4.0)      # a live case of 128 rows, built as truth.LIVE_CASES' n65: one tile, no padding
_LIVE = {}


def inputs(family, name):
    """-> (X, y, Xt, cov) of a case: truth.family_inputs, and "n128" (se) built here as n65 is there."""
    if name != "n128":
        return truth.family_inputs(family, name)
    assert family == "se"
    n, d, hp, scale = N128
    X, y = synth(n, d=d, seed=3 * n + d, scale=scale)
    return X, y, np.ascontiguousarray(truth.points(X, d, scale)), truth.SE(list(hp))


def live(oracle, family, name):
    """accuracy.live of the case (for "n128" the same construction on `inputs`)."""
    if name != "n128":
        return accuracy.live(oracle, family, name)
    if (family, name) not in _LIVE:
        X, y, Xt, cov = inputs(family, name)
        _LIVE[family, name] = accuracy.case_at(oracle, cov, X, y, Xt, truth.Truth(X, y, cov), truth.solve_rows(len(y)))
    return _LIVE[family, name]


# ---------------------------------------------------------------------------------------- the formulas, any dtype
def point_quantities(kap, alpha, y, const):
    """-> (mu, var, logp) from kappa = diag K^-1, alpha and y, in their dtype."""
    return y - alpha / kap, 1 / kap, np.log(kap) / 2 - alpha * alpha / (2 * kap) - const / 2


def fused(Kinv, alpha, mutate=None, product=None):
    """W_loo of the fused formulation.  product(B) -> B B' (default: B @ B.T).  mutate: "c_without_alpha" drops the
    alpha_i^2 / kappa_i term of c_i; "one_outer_product" keeps b alpha' and drops alpha b'."""
    kap = np.diag(Kinv).copy()
    a = alpha / kap
    c = (1 + alpha * a) / kap if mutate != "c_without_alpha" else 1 / kap
    b = Kinv @ a
    B = Kinv * np.sqrt(c)[None, :]
    P = product(B) if product is not None else B @ B.T
    W = P - np.outer(b, alpha)
    if mutate != "one_outer_product":
        W = W - np.outer(alpha, b)
    return W


def truth_of(t, y):
    """Every checked quantity in longdouble from the single-target truth t (kept: Kinv) -> dict(mu, var, logp, ll, grad)."""
    yl = np.asarray(y, dtype=np.float64).astype(LD)
    kap = np.diag(t.Kinv).copy()
    mu, var, logp = point_quantities(kap, t.alpha, yl, LD(truth.LL_CONST))
    ll = LD(0)
    for v in logp:
        ll = ll + v
    W = fused(t.Kinv, t.alpha, product=lambda B: truth._mm(B, np.ascontiguousarray(B.T)))
    _, terms = t.cov.train(t.X)
    grad = np.array(terms(W) + (t.sn2 * np.trace(W),), dtype=LD)
    return dict(mu=mu, var=var, logp=logp, ll=ll, grad=grad, y=yl)


def brute(X, y, cov):
    """Leave-one-out by actually leaving one out, in longdouble: point i predicted from the other n - 1 by a factorisation of
    their own -> (mu, var, logp, L_LOO).  O(n^4): for the small cases of the CPU suite."""
    Xl = np.asarray(X, dtype=np.float64).astype(LD)
    yl = np.asarray(y, dtype=np.float64).astype(LD)
    n = len(yl)
    Kf, _ = cov.train(Xl)
    K = Kf + cov.sn2 * np.eye(n, dtype=LD)
    mu, var = np.empty(n, dtype=LD), np.empty(n, dtype=LD)
    for i in range(n):
        o = np.arange(n) != i
        T = truth.tri_inverse(truth.cholesky(K[np.ix_(o, o)]))
        w = T @ K[o, i]
        mu[i] = w @ (T @ yl[o])
        var[i] = K[i, i] - w @ w
    logp = -np.log(var) / 2 - (yl - mu) ** 2 / (2 * var) - LD(truth.LL_CONST) / 2
    ll = LD(0)
    for v in logp:
        ll = ll + v
    return mu, var, logp, ll


# ---------------------------------------------------------------------------------------- fp64: yardstick and stand-in
def dK_list(c, X):
    """(Kf, [dK_j]) in fp64: the explicit derivative matrices of K = Kf + sn2 I in the family's hyper-parameter order."""
    n = X.shape[0]
    if isinstance(c, (truth.ARD, tam.ARDMatern)):
        S = truth.wsqdist(X, X, c.w)
        Kf, H = (c.sf2 * np.exp(-S / 2),) * 2 if isinstance(c, truth.ARD) else tam.parts(S, c.sf2, c.kind)
        lead = [None] * len(c.w)

        def per_dim(j, D2):
            lead[j] = H * D2
        truth.wsqdist(X, X, c.w, per_dim)
    elif isinstance(c, truth.Matern):
        Kf, dK = truth.matern_kernel(truth.sqdist(X, X, c.dtype) / c.l2, c.sf2, c.kind)
        lead = [dK]
    else:
        S = truth.sqdist(X, X, c.dtype) / c.l2
        Kf = c.sf2 * np.exp(-S / 2)
        lead = [Kf * S]
    return Kf, lead + [2 * Kf, 2 * c.sn2 * np.eye(n)]


def textbook(oracle, cov, X, y):
    """GPML 5.10-5.13 in fp64: K^-1 and alpha from the oracle's potri / potrs, then per hyper-parameter Z_j = K^-1 dK_j and
        dL/dtheta_j = sum_i [alpha_i (Z_j alpha)_i - 1/2 (1 + alpha_i^2 / kappa_i) (Z_j K^-1)_ii] / kappa_i
    -> (ll, grad of -L_LOO, mu, var, logp)."""
    c = cov.fp64()
    X, y = np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n = len(y)
    Kf, dKs = dK_list(c, X)
    K = Kf + c.sn2 * np.eye(n)
    Ki = np.asarray(oracle.K_inverse(K))
    a = np.asarray(oracle.Kinvy(K, y))
    kap = np.diag(Ki).copy()
    mu, var, logp = point_quantities(kap, a, y, truth.LL_CONST)
    ll = 0.0
    for v in logp:
        ll = ll + v
    g = []
    for dK in dKs:
        Z = Ki @ dK
        g.append(-np.sum((a * (Z @ a) - 0.5 * (1 + a * a / kap) * np.sum(Z * Ki.T, axis=1)) / kap))
    return ll, np.array(g), mu, var, logp


def standin(cov, X, y, mutate=None):
    """The fused formulation in fp64, LAPACK / BLAS order -> (ll, grad, mu, var, logp)."""
    import scipy.linalg as sl
    c = cov.fp64()
    X, y = np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n = len(y)
    Kf, terms = c.train(X)
    L = np.linalg.cholesky(Kf + c.sn2 * np.eye(n))
    T = sl.solve_triangular(L, np.eye(n), lower=True)
    Ki = T.T @ T
    a = Ki @ y
    mu, var, logp = point_quantities(np.diag(Ki).copy(), a, y, truth.LL_CONST)
    ll = 0.0
    for v in logp:
        ll = ll + v
    W = fused(Ki, a, mutate)
    return ll, np.array(terms(W) + (c.sn2 * np.trace(W),)), mu, var, logp


def errors(cov, tt, ll, grad, mu, var, logp):
    """Errors of one fp64 evaluation against truth_of's tt: truth.errors_ll_grad on L_LOO and the gradient, the largest
    absolute error of mu, var and logp."""
    e = truth.errors_ll_grad(cov, ll, grad, tt["ll"], tt["grad"])
    for q, v in zip(POINT_QUANTITIES, (mu, var, logp)):
        e[q] = float(np.max(np.abs(np.asarray(v).astype(LD) - tt[q])))
    return e


def quantities(cov):
    return cov.quantities[:4] + POINT_QUANTITIES


def floors(cov, tt):
    """4 ulp of each quantity's scale: 1 for L_LOO and the gradient (relative errors), max|mu|, sf2 + sn2, max|logp|.
    At n = 1 every mu is exactly 0 (nothing is left to predict from): its scale is then that of the cancelling
    y - alpha / kappa, max|y|."""
    fl = {q: U4 for q in cov.quantities[:4]}
    mu_scale = float(np.max(np.abs(tt["mu"])))
    if mu_scale == 0:
        mu_scale = float(np.max(np.abs(tt["y"])))
    fl.update(mu=U4 * mu_scale, var=U4 * float(cov.sf2 + cov.sn2),
              logp=U4 * float(np.max(np.abs(tt["logp"]))))
    return fl


def yardstick(oracle, cov, X, y, tt):
    """The textbook route over the data as given and truth.permutations -> (noise, first, rest) per quantity, as
    truth.noise_level's."""
    n = len(y)

    def one(idx):
        ll, g, mu, var, logp = textbook(oracle, cov, X[idx], y[idx])
        inv = np.empty(n, dtype=np.int64)
        inv[idx] = np.arange(n)
        return errors(cov, tt, ll, g, mu[inv], var[inv], logp[inv])
    E = list(truth._pool().map(one, truth.permutations(n)))
    Q = quantities(cov)
    return {q: max(e[q] for e in E) for q in Q}, {q: E[0][q] for q in Q}, {q: max(e[q] for e in E[1:]) for q in Q}


_CASES = {}


def case(oracle, family, name):
    """Truth, yardstick and floors of (family, case), computed once per process whichever test asks."""
    key = (family, name)
    if key not in _CASES:
        c = live(oracle, family, name)
        tt = truth_of(c["t"], c["y"])
        noise, first, rest = yardstick(oracle, c["cov"], c["X"], c["y"], tt)
        _CASES[key] = dict(X=c["X"], y=c["y"], cov=c["cov"], t=c["t"], tt=tt, noise=noise, first=first, rest=rest,
                           floor=floors(c["cov"], tt), family=family)
    return _CASES[key]


def ratios(c, out):
    """error / max(yardstick, floor) per quantity of one evaluation `out` = (ll, grad, mu, var, logp)."""
    e = errors(c["cov"], c["tt"], *out)
    return {q: e[q] / max(c["noise"][q], c["floor"][q]) for q in quantities(c["cov"])}


def hold(rep, c, ll, grad, mu, var, logp, tag=""):
    """Adds every checked quantity of one evaluation to the accuracy.Report `rep` under the bound F_LOO[family]."""
    F = F_LOO[c["family"]]
    e = errors(c["cov"], c["tt"], ll, grad, mu, var, logp)
    for q in quantities(c["cov"]):
        if q in e:
            rep.add(tag + q, e[q], c["noise"][q], c["floor"][q], F)


def assert_yardstick_is_sane(c, tag):
    """accuracy.assert_yardstick_is_sane's two conditions on this module's quantities: the data as given is no outlier among
    the permutations, and no yardstick exceeds truth.YARDSTICK_CAP of its scale."""
    for q in quantities(c["cov"]):
        assert c["first"][q] <= c["cov"].F * max(c["rest"][q], c["floor"][q]), (tag, q, c["first"][q], c["rest"][q])
        assert c["noise"][q] <= truth.YARDSTICK_CAP * c["floor"][q] / U4, (tag, q, c["noise"][q])
