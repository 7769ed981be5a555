"""Truth, yardstick, stand-in and bound of the gradients of the predictive mean and variance with respect to the test
inputs (include/cugp.h: cugp_predict_grad, cugp_poe_combine_grad) -- TEST INFRASTRUCTURE, CPU, numpy only; a plain module
beside tests/truth.py and tests/accuracy.py, which it imports and leaves as they are.

With k_i = k(x*, x_i), alpha = K^-1 y, v = K^-1 k* (row t of V = Ks K^-1):

    dmean[t][c] = -s_c sum_i G_ti alpha_i (x*_tc - x_ic)        dvar[t][c] = +2 s_c sum_i G_ti V_ti (x*_tc - x_ic)
    SE, ARD  G = k,  s_c = 1 / l^2 | w_c^2;   Matern 3/2  G = sf2 3 e^-a;   5/2  G = sf2 (5/3) (1 + a) e^-a,  s_c = 1 / l^2

  truth      from the cached accuracy.live(oracle, family, name) truth: alpha, K^-1 and X in longdouble (no second
             factorisation), V = Ks K^-1 and the sums above in longdouble, per feature, the difference formed first
  yardstick  the project's procedure (truth.permutations: the data as given and 7 row permutations).  For each: alpha from
             the family's evaluator(..., solve=True); K of the permuted rows from cov.fp64().train; L = oracle.cholesky(K)
             (the reference's order); V by two triangular substitutions; the sums in fp64 numpy.  The yardstick is the
             largest absolute error over all nt x d entries, for dmean and for dvar.  (V is NOT taken from the oracle's
             explicit K^-1: that is 20 to 1000 times looser at cond(K) ~ 1e6 and exceeds truth.YARDSTICK_CAP.)
  floor      4 ulp of max|true dmean| and of max|true dvar|
  stand-in   the library's formulation in fp64, LAPACK / BLAS order: V = (Ks T^T) T, (G alpha) and (G V) rounded, then
             times the difference; `coordinate=True` is the mutation x*_c sum(G a) - sum(G a x_c)
  bound      err <= F_family max(yardstick, floor) with truth.F, F_MATERN, F_ARD as they stand: the stand-in stays at or
             below half of them on every case (tests/test_truth_predict_grad_cpu.py; docs/ACCURACY.md has the table).
             F_GRAD (None: not needed) would replace them by truth.factor_rule of the largest ratio.

The product of experts: `combine_grad` is the chain rule of the combination rules (truth_poe_modes.combine) in the arrays'
own precision; truth = the experts' truths through it in longdouble, yardstick = the experts' fp64 yardstick evaluations
through it in fp64, the rows permuted inside each expert.
"""
import numpy as np

import accuracy
import truth
import truth_poe_modes as tpm

LD = truth.LD
QUANTITIES = ("dmean", "dvar")
F_GRAD = None                     # a factor of its own is not needed (docs/ACCURACY.md: the largest stand-in ratio is below F / 2)

# family -> its cases: the smallest shapes at which the tile pass can go wrong (one tile with identity padding and the
# boundary at 64; two training tiles; ragged n; two and three feature chunks; ill conditioning; |x| >> |x - x'|)
CASES = {
    "se": ("n1", "n2", "n63", "n64", "n65", "n257_d3", "n300_d17", "n515_d33", "n384_cond1e6"),
    "matern32": ("n1", "n2", "n63", "n64", "n65", "n257_d3"),
    "matern52": ("n1", "n63", "n300_d17", "n384_cond1e6"),
    "ard": ("n1_d2", "n2_d2", "n63_d2", "n64_d2", "n65_d2", "n257_d3", "n300_d17", "n257_d3_shift", "n384_cond1e6"),
}
CASE_LIST = [(f, n) for f, names in CASES.items() for n in names]
WIDE_CASES = (("se", "n257_d3"), ("ard", "n257_d3"), ("matern52", "n300_d17"))
WIDE_NTS = (129, 200)
BCM_CASES = ("se_3x300", "se_5x261p2", "matern52_3x300", "ard_3x300")
BCM_NT = 200
BCM_MODES = tpm.MODES + ("reference",)


def factor(cov):
    return cov.F if F_GRAD is None else F_GRAD


# ------------------------------------------------------------------ the formulas, in the arrays' own precision
def g_and_scale(cov, Xt, X):
    """-> (G [nt, n], s [d]) of the descriptor `cov` in its dtype."""
    T = cov.dtype
    Xt, X = np.asarray(Xt, dtype=T), np.asarray(X, dtype=T)
    d = X.shape[1]
    if isinstance(cov, truth.ARD):
        return cov.k(Xt, X), cov.w * cov.w
    s = np.full(d, T(1) / cov.l2, dtype=T)
    if isinstance(cov, truth.Matern):
        a = np.sqrt(truth.C2[cov.kind] * (truth.sqdist(Xt, X, T) / cov.l2))
        e = np.exp(-a)
        if cov.kind == truth.MATERN32:
            return cov.sf2 * 3 * e, s
        return cov.sf2 * (T(5) / T(3)) * (1 + a) * e, s
    return cov.k(Xt, X), s


def sums(GA, Xt, X, s, coordinate=False):
    """out[t][c] = s_c sum_i GA[t][i] (xt[t][c] - x[i][c]), the difference first; coordinate: the mutation
    s_c (xt[t][c] (GA 1) - GA x_c), two matrix-vector products as a GEMM-shaped kernel would form them."""
    out = np.empty((Xt.shape[0], X.shape[1]), dtype=GA.dtype)
    for c in range(X.shape[1]):
        if coordinate:
            out[:, c] = (Xt[:, c] * (GA @ np.ones(X.shape[0], dtype=GA.dtype)) - GA @ X[:, c]) * s[c]
        else:
            out[:, c] = (GA * (Xt[:, c][:, None] - X[:, c][None, :])).sum(1) * s[c]
    return out


def gradients(cov, Xt, X, alpha, V, coordinate=False):
    """-> (dmean, dvar) [nt, d] in cov's dtype from alpha [n] and V [nt, n]."""
    T = cov.dtype
    Xt, X = np.asarray(Xt, dtype=T), np.asarray(X, dtype=T)
    G, s = g_and_scale(cov, Xt, X)
    return -sums(G * alpha[None, :], Xt, X, s, coordinate), 2 * sums(G * V, Xt, X, s, coordinate)


# ------------------------------------------------------------------ truth
def truth_gradients(t, Xt):
    """From a truth.Truth kept with K^-1: V = Ks K^-1 and the sums in longdouble."""
    Xt = np.asarray(Xt, dtype=np.float64).astype(LD)
    V = truth._mm(t.cov.k(Xt, t.X), t.Kinv)
    return gradients(t.cov, Xt, t.X, t.alpha, V)


def truth_predict(t, Xt, latent=False):
    """(mean, var) of a truth.Truth at one set of points, the inputs taken AS GIVEN in longdouble (truth.Truth.predict
    rounds them to fp64 first: the central differences perturb them below that)."""
    Xt = np.asarray(Xt, dtype=LD)
    Ks = t.cov.k(Xt, t.X)
    Wt = Ks @ t.T.T
    return Ks @ t.alpha, t.sf2 + (0 if latent else t.sn2) - (Wt * Wt).sum(1)


def errors(dm, dv, tdm, tdv):
    return dict(dmean=float(np.max(np.abs(np.asarray(dm).astype(LD) - tdm))),
                dvar=float(np.max(np.abs(np.asarray(dv).astype(LD) - tdv))))


# ------------------------------------------------------------------ yardstick
def yardstick_gradients(oracle, cov, evaluate, Xe, X, y, Xt, idx):
    """One fp64 yardstick evaluation on the rows idx: (dmean, dvar)."""
    import scipy.linalg as sl
    c64 = cov.fp64()
    Xp = np.ascontiguousarray(X[idx])
    a = evaluate(np.ascontiguousarray(Xe[idx]), np.ascontiguousarray(y[idx]))[4]
    Kf, _ = c64.train(Xp)
    L = np.asarray(oracle.cholesky(Kf + c64.sn2 * np.eye(len(idx))))
    Ks = c64.k(Xt, Xp)
    V = sl.solve_triangular(L.T, sl.solve_triangular(L, Ks.T, lower=True), lower=False).T
    return gradients(c64, Xt, Xp, np.asarray(a), V)


def yardstick(oracle, cov, X, y, Xt, tdm, tdv):
    """-> (noise, first, rest) per quantity, as truth.noise_level."""
    Xe, evaluate = cov.evaluator(oracle, X, Xt, solve=True)
    X, Xt = np.asarray(X, dtype=np.float64), np.asarray(Xt, dtype=np.float64)

    def one(idx):
        return errors(*yardstick_gradients(oracle, cov, evaluate, Xe, X, y, Xt, idx), tdm, tdv)
    E = list(truth._pool().map(one, truth.permutations(len(y))))
    Q = QUANTITIES
    return {q: max(e[q] for e in E) for q in Q}, {q: E[0][q] for q in Q}, {q: max(e[q] for e in E[1:]) for q in Q}


def case_at(oracle, cov, X, y, Xt, t):
    tdm, tdv = truth_gradients(t, Xt)
    noise, first, rest = yardstick(oracle, cov, X, y, Xt, tdm, tdv)
    floor = dict(dmean=truth.U4 * float(np.max(np.abs(tdm))), dvar=truth.U4 * float(np.max(np.abs(tdv))))
    return dict(X=X, y=y, Xt=Xt, cov=cov, t=t, tdm=tdm, tdv=tdv, noise=noise, first=first, rest=rest, floor=floor)


_CASES = {}


def case(oracle, family, name):
    """Truth, yardsticks and floors of the gradients of a live case at its 64 test points, once per process."""
    if (family, name) not in _CASES:
        c = accuracy.live(oracle, family, name)
        _CASES[family, name] = case_at(oracle, c["cov"], c["X"], c["y"], c["Xt"], c["t"])
    return _CASES[family, name]


def wide_case(oracle, family, name, nt):
    """The same at nt test points (truth.wide_inputs), on the live case's truth."""
    if (family, name, nt) not in _CASES:
        X, y, Xt, cov = truth.wide_inputs(name, nt, family)
        _CASES[family, name, nt] = case_at(oracle, cov, X, y, Xt, accuracy.live(oracle, family, name)["t"])
    return _CASES[family, name, nt]


def ratios(c, dm, dv):
    e = errors(dm, dv, c["tdm"], c["tdv"])
    return {q: e[q] / max(c["noise"][q], c["floor"][q]) for q in QUANTITIES}


def hold(rep, c, dm, dv, tag=""):
    """Adds both quantities of a GPU (or stand-in) result to an accuracy.Report at the family's factor."""
    e = errors(dm, dv, c["tdm"], c["tdv"])
    for q in QUANTITIES:
        rep.add(tag + q, e[q], c["noise"][q], c["floor"][q], factor(c["cov"]))


def assert_yardstick_is_sane(c, tag):
    """accuracy.assert_yardstick_is_sane's two conditions on the two quantities (their scale: the largest true entry)."""
    for q in QUANTITIES:
        assert c["first"][q] <= c["cov"].F * max(c["rest"][q], c["floor"][q]), (tag, q, c["first"][q], c["rest"][q])
        scale = c["floor"][q] / truth.U4
        assert c["noise"][q] <= truth.YARDSTICK_CAP * scale, (tag, q, c["noise"][q], scale)


# ------------------------------------------------------------------ stand-in
def standin(cov, X, y, Xt, coordinate=False):
    """The library's formulation in fp64, LAPACK / BLAS order: alpha = T^T (T y), V = (Ks T^T) T."""
    import scipy.linalg as sl
    c64 = cov.fp64()
    X, Xt = np.asarray(X, dtype=np.float64), np.asarray(Xt, dtype=np.float64)
    n = len(y)
    Kf, _ = c64.train(X)
    L = np.linalg.cholesky(Kf + c64.sn2 * np.eye(n))
    T = sl.solve_triangular(L, np.eye(n), lower=True)
    a = T.T @ (T @ y)                                   # (z = L^-1 y, alpha = L^-T z: the library's two triangular products)
    Ks = c64.k(Xt, X)
    return gradients(c64, Xt, X, a, (Ks @ T.T) @ T, coordinate)


# ------------------------------------------------------------------ the product of experts
def combine_grad(m, v, dm, dv, mode, sf2):
    """The chain rule of truth_poe_modes.combine: experts' means and variances m, v [K][nt] and their gradients dm, dv
    [K][nt][d] -> (dmean, dvar) [nt][d] of the combination, in the arrays' own precision.  mode "reference": the plain
    product (poe's arithmetic; the caller passes the noisy variances)."""
    m, v, dm, dv = np.asarray(m), np.asarray(v), np.asarray(dm), np.asarray(dv)
    T = v.dtype.type
    one, sf2, K = T(1), T(sf2), len(v)
    p = one / v
    db = np.zeros_like(dv)
    if mode == "gpoe":
        beta = np.full_like(p, one / T(K))
    elif mode == "rbcm":
        beta = T(0.5) * np.log(sf2 * p)
        db = -T(0.5) * dv / v[..., None]
    else:
        beta = np.ones_like(p)
    prior = mode in ("bcm", "rbcm")
    sp, S, sb = (beta * p).sum(0), (beta * p * m).sum(0), beta.sum(0)
    prec = sp + (one - sb) / sf2 if prior else sp
    dp = -dv / (v * v)[..., None]
    dprec = (db * p[..., None] + beta[..., None] * dp).sum(0)
    if prior:
        dprec = dprec - db.sum(0) / sf2
    dS = (db * (p * m)[..., None] + beta[..., None] * dp * m[..., None] + (beta * p)[..., None] * dm).sum(0)
    dvar = -dprec / (prec * prec)[:, None]
    return dvar * S[:, None] + dS / prec[:, None], dvar


def combine_all(ex, mode, cov):
    """Per-expert (m, var_f, dm, dv) -> (dmean, dvar) of rule `mode`; "reference" adds sn2 to the variances first."""
    m, v = np.array([e[0] for e in ex]), np.array([e[1] for e in ex])
    dm, dv = np.array([e[2] for e in ex]), np.array([e[3] for e in ex])
    if mode == "reference":
        v = v + v.dtype.type(cov.sn2)
    return combine_grad(m, v, dm, dv, mode, cov.sf2)


def bcm_case(oracle, name, nt=BCM_NT):
    """A case of truth_poe_modes.CASES at nt points: truth, yardstick and floor of the combined gradients per mode of
    BCM_MODES.  -> dict(X, y, Xt, cov, K, modes={mode: dict(tdm, tdv, noise, floor)})."""
    if ("bcm", name, nt) not in _CASES:
        X, y, Xt, cov, K = tpm.inputs(name, nt)
        _CASES["bcm", name, nt] = bcm_case_at(oracle, X, y, Xt, cov, truth.bcm_rows(len(y), K), tpm.expert_truths(name))
    return _CASES["bcm", name, nt]


def bcm_case_at(oracle, X, y, Xt, cov, parts, truths):
    """bcm_case's body for experts on the rows `parts` [(offset, rows)] of (X, y) with their truth.Truth `truths`."""
    c64 = cov.fp64()
    ex = []
    for (o, r), t in zip(parts, truths):
        # (the experts' truths are kept without K^-1: V = (Ks T^T) T in longdouble)
        Xl = Xt.astype(LD)
        _, Ks, Wt = t._cross(Xt)
        ex.append((Ks @ t.alpha, t.sf2 - (Wt * Wt).sum(1)) + gradients(cov, Xl, t.X, t.alpha, truth._mm(Wt, t.T)))
    Xe, evaluate = cov.evaluator(oracle, X, Xt, solve=True)

    def one(idx):
        out = []
        for o, r in parts:
            i = idx[o: o + r]
            res = evaluate(np.ascontiguousarray(Xe[i]), np.ascontiguousarray(y[i]))
            out.append((res[2], res[3] - c64.sn2) + yardstick_gradients(oracle, cov, evaluate, Xe, X, y, Xt, i))
        return out
    E = list(truth._pool().map(one, truth.permutations(len(y), parts)))
    modes = {}
    for mode in BCM_MODES:
        tdm, tdv = combine_all(ex, mode, cov)
        errs = [errors(*combine_all(e, mode, c64), tdm, tdv) for e in E]
        modes[mode] = dict(tdm=tdm, tdv=tdv, noise={q: max(e[q] for e in errs) for q in QUANTITIES},
                           floor=dict(dmean=truth.U4 * float(np.max(np.abs(tdm))), dvar=truth.U4 * float(np.max(np.abs(tdv)))))
    return dict(X=X, y=y, Xt=Xt, cov=cov, K=len(parts), parts=parts, modes=modes)


def bcm_standin(c, mode):
    """The stand-in per expert (LAPACK / BLAS order, the latent variance direct) through the chain rule in fp64."""
    cov = c["cov"]
    ms, vs = tpm.standin_experts(c)
    ex = [(ms[k], vs[k]) + standin(cov, c["X"][o: o + r], c["y"][o: o + r], c["Xt"])
          for k, (o, r) in enumerate(tpm.rows_of(c))]
    return combine_all(ex, mode, cov.fp64())


def bcm_ratios(c, mode, dm, dv):
    m = c["modes"][mode]
    e = errors(dm, dv, m["tdm"], m["tdv"])
    return {q: e[q] / max(m["noise"][q], m["floor"][q]) for q in QUANTITIES}
