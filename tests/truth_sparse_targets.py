"""Multi-target regression over one set of inducing points (cugp_sparse_*_targets): the targets, the truth, the yardstick,
the stand-in and the factors of its tests -- TEST INFRASTRUCTURE, CPU, numpy only; a plain module beside tests/truth.py,
tests/truth_sparse.py, tests/truth_sparse_z.py and tests/truth_targets.py, which it imports and leaves as they are.

p targets y_1 .. y_p share the rows X, the hyper-parameters, the inducing inputs Z and the jitter; F = sum_t F_t with F_t
truth_sparse's bound for y_t; the library returns F, the F_t, the gradient of -F (in theta and in Z) and the means.

  targets    truth_targets.targets(y, p) on the case's y: Y[0] = y, and the first rows of a wider set are the narrower set
  truth      `Truth`: longdouble, from the definition -- ONE Cholesky factor of Qff + s2 I per case, F_t from a forward
             substitution per target; the gradient from truth_sparse.Truth's G formulas with Kuu^-1 and Sigma^-1 shared,
             beta_t per target and G_Phi, G_uu summed over the targets; gZ from truth_sparse_z.formula on the summed G_uf and
             2 G_uu; the means Ks beta_t; the variance truth_sparse.Truth's (no target enters)
  yardstick  truth_sparse.computed_form (and truth_sparse_z.computed_gz) PER TARGET, summed in target order, over the data as
             given and truth.permutations: fp64 numpy / LAPACK on the whole data at once
  stand-in   `standin`: the fused formulation of include/cugp.h in fp64 numpy, in cugp_sparse_plan's chunks: Q through
             128-row slabs, H = p (I - B^-1) - sum_t gamma_t gamma_t', the rank-p part added to W_c R' target after target
  errors     F and every F_t relative; every gradient component relative to max|g|; gZ relative to max|gZ|; the means the
             largest absolute error over all targets; the variance the largest absolute error
  bound      F_SPARSE_TARGETS[family] max(yardstick, 4 ulp of the quantity's scale) (gZ: F_SPARSE_TARGETS_Z), fixed below
             from the stand-in's ratios measured on the CPU (docs/ACCURACY.md has the table), never from the GPU's errors.
"""
import numpy as np

import truth
import truth_sparse as ts
import truth_sparse_z as tz
import truth_targets

LD = truth.LD
U4 = truth.U4
JITTER = ts.JITTER

# (case of truth_sparse.CASES, p): what each covers is in tests/test_gpu_sparse_targets.py.  The library's group of targets in
# the Q pass is 8 wide, its staging rounds in the H and weight passes 16: 9 and 17 reach a second group / round of one target.
CASES = (
    ("se_n128_m128", 1),
    ("se_n300_m65", 3),
    ("se_n1300_m200", 17),
    ("ard_n300_m130_d17", 5),
    ("matern32_ard_n1000_m130", 9),
    ("matern52_n800_m65_d3_c0", 2),
    ("se_n300_dup60", 3),
)
P_OF = dict(CASES)
MUTATIONS = ("h_without_p", "rank_one_only")

# The larger of F_SPARSE[family] (F_SPARSE_Z for gZ) and truth.factor_rule of the largest stand-in / yardstick ratio over
# CASES (tests/test_truth_sparse_targets_cpu.py measures and asserts; docs/ACCURACY.md: the table).
# Largest stand-in ratios measured (gZ in brackets): se 3.14, g0 of se_n1300_m200 with 17 targets (1.00; factor_rule 8 (4)),
# ard 0.51 (1.44), matern32_ard 0.94 (0.54), matern52 0.86 (0.46) (factor_rule 2 (1 to 4)): every family's F_SPARSE
# (8, 32, 32, 16) and F_SPARSE_Z stand.
F_SPARSE_TARGETS = dict(ts.F_SPARSE)
F_SPARSE_TARGETS_Z = dict(tz.F_SPARSE_Z)


def targets(name, p):
    """Y [p][n] target-major of a case: truth_targets.targets on its y."""
    return truth_targets.targets(ts.inputs(name)[1], p)


# ---------------------------------------------------------------------------------------- the truth
class Truth:
    """Every checked quantity in longdouble: F_each, F (summed in target order), grad (of -F), gz (of -F, [M][d]),
    predict(Xt) -> (means [p][nt], var with noise [nt])."""

    def __init__(self, X, Y, Z, cov, jitter=JITTER):
        truth.require_extended()
        Xl, Zl = np.asarray(X, dtype=np.float64).astype(LD), np.asarray(Z, dtype=np.float64).astype(LD)
        Yl = np.asarray(Y, dtype=np.float64).astype(LD)
        p, N = Yl.shape
        M = len(Zl)
        s2, sf2 = cov.sn2, cov.sf2
        Kuu, dKuu = ts.kernel_parts(cov, Zl, Zl)
        Kuu[np.arange(M), np.arange(M)] += LD(jitter)
        Kuf, dKuf = ts.kernel_parts(cov, Zl, Xl)
        Tu = truth.tri_inverse(truth.cholesky(Kuu))
        A0 = truth._mm(Tu, Kuf)
        Qff = truth._mm(np.ascontiguousarray(A0.T), A0)
        Cm = Qff.copy()
        Cm[np.arange(N), np.arange(N)] += s2
        LC = truth.cholesky(Cm)                                       # the ONE N x N factor
        base = -N * ts.LOG2PI / 2 - np.log(np.diag(LC)).sum() - (N * sf2 - np.trace(Qff)) / (2 * s2)
        self.F_each = np.array([base - z @ z / 2 for z in (ts.forward(LC, y) for y in Yl)], dtype=LD)
        self.F = LD(0)
        for v in self.F_each:
            self.F = self.F + v
        # the gradient: Kuu^-1 and Sigma^-1 shared, beta_t per target
        Kuui = truth.gram_lower(Tu)
        Phi = truth._mm(Kuf, np.ascontiguousarray(Kuf.T))
        Si = truth.gram_lower(truth.tri_inverse(truth.cholesky(Kuu + Phi / s2)))
        V = Kuf @ Yl.T                                                # [M, p]
        Beta = Si @ V / s2                                            # [M, p]
        BB = Beta @ Beta.T                                            # sum_t beta_t beta_t'
        G_phi = (p * (Kuui - Si) - BB) / (2 * s2)
        G_uu = p * Kuui / 2 - (p * Si + BB) / 2 - p * (Kuui @ Phi @ Kuui) / (2 * s2)
        G_uf = 2 * truth._mm(G_phi, Kuf) + (Beta / s2) @ Yl
        Kuu0 = Kuu.copy()
        Kuu0[np.arange(M), np.arange(M)] -= LD(jitter)
        dF = [(G_uu * a).sum() + (G_uf * b).sum() for a, b in zip(dKuu, dKuf)]
        dF.append(2 * ((G_uu * Kuu0).sum() + (G_uf * Kuf).sum()) - p * N * sf2 / s2)
        yy, vb, bpb = (Yl * Yl).sum(), (V * Beta).sum(), (Beta * (Phi @ Beta)).sum()
        dF.append(2 * s2 * (-p * N / (2 * s2) + p * np.trace(Si @ Phi) / (2 * s2 * s2) + yy / (2 * s2 * s2) - vb / (s2 * s2)
                            + bpb / (2 * s2 * s2) + p * (N * sf2 - np.trace(Kuui @ Phi)) / (2 * s2 * s2)))
        self.grad = -np.array(dF, dtype=LD)
        self.gz = tz.formula(cov, G_uf, 2 * G_uu, Xl, Zl)
        self.cov, self.Zl, self.D, self.Beta, self.p = cov, Zl, Kuui - Si, Beta, p

    def predict(self, Xt, with_noise=True):
        Ks = ts.kernel_parts(self.cov, np.asarray(Xt, dtype=np.float64).astype(LD), self.Zl)[0]      # [nt, M]
        var = self.cov.sf2 - ((Ks @ self.D) * Ks).sum(1)
        return (Ks @ self.Beta).T, var + self.cov.sn2 if with_noise else var


def bound_sum_definition(X, Y, Z, cov, jitter=JITTER):
    """sum_t F_t from truth_sparse.bound_definition per target (a whole factorisation each: for the smallest cases and
    the central differences only)."""
    F = LD(0)
    for y in Y:
        F = F + ts.bound_definition(X, y, Z, cov, jitter)
    return F


# ---------------------------------------------------------------------------------------- fp64: the yardstick
def computed_sum(cov, X, Y, Z, Xt, want_gz=True):
    """truth_sparse.computed_form per target, summed in target order -> (F, grad, F_each, means [p][nt], var, gZ)."""
    F, g, gz, each, means, var = 0.0, 0.0, 0.0, [], [], None
    for y in Y:
        Ft, gt, mt, var = ts.computed_form(cov, X, y, Z, Xt)
        F, g = F + Ft, g + gt
        each.append(Ft)
        means.append(mt)
        if want_gz:
            gz = gz + tz.computed_gz(cov, X, y, Z)
    return F, g, np.array(each), np.array(means), var, gz


# ---------------------------------------------------------------------------------------- fp64: the stand-in
def standin(cov, X, Y, Z, Xt, chunk_rows, jitter=JITTER, mutate=None):
    """The library's fused formulation in fp64 numpy -> (F, grad of -F, F_each, means [p][nt], var with noise, gZ).
    mutate: "h_without_p" takes I - B^-1 once in H; "rank_one_only" adds the rank-p part of the weights for target 0 only."""
    import scipy.linalg as sl
    c = cov.fp64()
    X, Y, Z = (np.asarray(a, dtype=np.float64) for a in (X, Y, Z))
    p, N = Y.shape
    M = len(Z)
    s2, sf2 = float(c.sn2), float(c.sf2)
    Kuu0, dKuu = ts.kernel_parts(c, Z, Z)
    Tu = sl.solve_triangular(np.linalg.cholesky(Kuu0 + jitter * np.eye(M)), np.eye(M), lower=True)
    P, Q = np.zeros((M, M)), np.zeros((p, M))
    chunks = ts.plan(N, M, chunk_rows)
    Ws = []
    for r0, rows, cpad, split, kstep in chunks:
        W = ts.kernel_parts(c, X[r0: r0 + rows], Z)[0] @ Tu.T
        Ws.append(W)
        for sidx in range(split):                                    # the Gram partials in plan order
            Wk = W[sidx * kstep: min((sidx + 1) * kstep, cpad)]
            P = P + Wk.T @ Wk
        for k0 in range(0, rows, 128):                               # Q through the 128-row slabs, every target
            Q = Q + Y[:, r0 + k0: r0 + k0 + 128] @ W[k0: k0 + 128]
    LB = np.linalg.cholesky(np.eye(M) + P / s2)
    TB = sl.solve_triangular(LB, np.eye(M), lower=True)
    Binv = TB.T @ TB
    Cp = Q @ TB.T                                                    # row t = LB^-1 q_t
    Gm = Cp @ TB                                                     # row t = LB^-T c'_t
    Bt = Gm @ Tu                                                     # row t = Lu^-T gamma'_t
    trp, nsf, lds = np.trace(P), N * sf2, np.log(np.diag(LB)).sum()
    each, F, yy, cc, gg = [], 0.0, 0.0, 0.0, 0.0
    for t in range(p):
        yyt, cct = Y[t] @ Y[t], Cp[t] @ Cp[t]
        Ft = ((((-0.5 * N * np.log(2 * np.pi) - lds) - 0.5 * N * np.log(s2)) - yyt / (2 * s2)) + cct / (2 * s2 * s2)) \
            - (nsf - trp) / (2 * s2)
        each.append(Ft)
        F, yy, cc, gg = F + Ft, yy + yyt, cc + cct, gg + Gm[t] @ Gm[t]
    H = (1 if mutate == "h_without_p" else p) * (np.eye(M) - Binv)
    for t in range(p):
        H = H - np.outer(Gm[t] / s2, Gm[t] / s2)
    H2 = H - p * (P / s2)
    R = (H @ Tu).T / s2
    Guu2 = ((H2 @ Tu).T) @ Tu
    Bs = Bt / s2 / s2
    nl = len(dKuu)
    S_uf, Sz = np.zeros(nl + 1), np.zeros(Z.shape)
    for (r0, rows, cpad, split, kstep), W in zip(chunks, Ws):
        Xc = X[r0: r0 + rows]
        Kc, dKc = ts.kernel_parts(c, Xc, Z)
        G = W @ R.T
        for t in range(1 if mutate == "rank_one_only" else p):
            G = G + np.outer(Y[t, r0: r0 + rows], Bs[t])
        S_uf = S_uf + np.array([(G * a).sum() for a in dKc] + [(G * Kc).sum()])
        Sz = Sz + tz.weighted_differences((G * tz.h_factor(c, Xc, Z)[0]).T, Xc, Z)
    S_uu = np.array([(Guu2 * a).sum() for a in dKuu] + [(Guu2 * Kuu0).sum()])
    Sz = Sz + tz.weighted_differences((Guu2 * tz.h_factor(c, Z, Z)[0]).T, Z, Z)
    gz = -(Sz * tz.h_factor(c, Z[:1], Z[:1])[1][None, :])
    S = S_uf + S_uu / 2
    g = list(-S[:nl])
    g.append(-(2 * S[nl] - p * nsf / s2))
    g.append(-(((p * np.sum(1 - np.diag(Binv)) - p * N) + (((yy - cc / s2) + p * (nsf - trp)) / s2)) - gg / (s2 * s2)))
    Wt = ts.kernel_parts(c, np.asarray(Xt, dtype=np.float64), Z)[0] @ Tu.T
    Vt = Wt @ TB.T
    return F, np.array(g), np.array(each), (Cp / s2) @ Vt.T, ((sf2 - (Wt * Wt).sum(1)) + (Vt * Vt).sum(1)) + s2, gz


# ---------------------------------------------------------------------------------------- errors, yardstick, bound
QUANTITIES_EXTRA = ("F_each", "gZ")


def errors(cov, t, tm, tv, F, grad, each, means, var, gz=None):
    """Errors of one fp64 evaluation against the Truth t: truth.errors_ll_grad on the sums, the largest relative error over
    the F_t, the largest absolute error over the mean matrix and the variances, gZ relative to max|gZ|."""
    e = dict(truth.errors_ll_grad(cov, F, grad, t.F, t.grad), **truth.errors_pred(means, var, tm, tv))
    e["F_each"] = float(np.max(np.abs(np.asarray(each).astype(LD) - t.F_each) / np.abs(t.F_each)))
    if gz is not None:
        e["gZ"] = tz.error(gz, t.gz)
    return e


def quantities(cov):
    return tuple(cov.quantities) + QUANTITIES_EXTRA


_CASES = {}


def case(name, p=None):
    """Inputs, targets, truth, yardstick (noise, first, rest) and floors of a case, once per process."""
    p = P_OF[name] if p is None else p
    if (name, p) not in _CASES:
        X, _, Z, Xt, cov, chunk = ts.inputs(name)
        Y = targets(name, p)
        t = Truth(X, Y, Z, cov)
        tm, tv = t.predict(Xt)
        # (the permutations on truth's thread pool: numpy and LAPACK release the GIL, and each evaluation is its own)
        E = list(truth._pool().map(lambda idx: errors(cov, t, tm, tv, *computed_sum(cov, X[idx], Y[:, idx], Z, Xt)),
                                   truth.permutations(Y.shape[1])))
        Qs = quantities(cov)
        fl = truth.floors(cov, truth.scales(cov, t.F, t.grad, tm))
        fl.update(F_each=U4, gZ=U4)
        _CASES[name, p] = dict(X=X, Y=Y, Z=Z, Xt=Xt, cov=cov, chunk=chunk, t=t, tm=tm, tv=tv, family=ts.CASES[name][0], p=p,
                               noise={q: max(e[q] for e in E) for q in Qs}, first={q: E[0][q] for q in Qs},
                               rest={q: max(e[q] for e in E[1:]) for q in Qs}, floor={q: fl[q] for q in Qs})
    return _CASES[name, p]


def factor(c, q):
    return (F_SPARSE_TARGETS_Z if q == "gZ" else F_SPARSE_TARGETS)[c["family"]]


def ratios(c, out):
    """error / max(yardstick, floor) per quantity of one evaluation `out` = (F, grad, F_each, means, var[, gZ])."""
    e = errors(c["cov"], c["t"], c["tm"], c["tv"], *out)
    return {q: e[q] / max(c["noise"][q], c["floor"][q]) for q in e}


def hold(rep, c, F, grad, each, means, var, gz=None, tag=""):
    """Adds every checked quantity of one evaluation to the accuracy.Report `rep` under the bound."""
    e = errors(c["cov"], c["t"], c["tm"], c["tv"], F, grad, each, means, var, gz)
    for q in e:
        rep.add(tag + q, e[q], c["noise"][q], c["floor"][q], factor(c, q))


# ---------------------------------------------------------------------------------------- beyond one test tile
_WIDE = {}


def wide_case(name, p, nt, z_row=ts.WIDE_Z_ROW, data_row=None):
    """The case at truth_sparse.wide_points' nt test points: the truth's means [p][nt] and variance there and the yardstick
    (computed_form per target over the data as given and truth.permutations), once per process."""
    key = (name, p, nt, z_row, data_row)
    if key not in _WIDE:
        c = case(name, p)
        Xt = ts.wide_points(name, nt, z_row, data_row)
        tm, tv = c["t"].predict(Xt)

        def one(idx):
            out = computed_sum(c["cov"], c["X"][idx], c["Y"][:, idx], c["Z"], Xt, want_gz=False)
            return truth.errors_pred(out[3], out[4], tm, tv)
        E = list(truth._pool().map(one, truth.permutations(c["Y"].shape[1])))
        fl = truth.floors(c["cov"], truth.scales(c["cov"], c["t"].F, c["t"].grad, tm))
        _WIDE[key] = dict(Xt=Xt, tm=tm, tv=tv, noise={q: max(e[q] for e in E) for q in ("mean", "var")},
                          floor={q: fl[q] for q in ("mean", "var")})
    return _WIDE[key]


def hold_wide(rep, c, w, means, var, tag=""):
    e = truth.errors_pred(means, var, w["tm"], w["tv"])
    for q in ("mean", "var"):
        rep.add(tag + q, e[q], w["noise"][q], w["floor"][q], factor(c, q))
