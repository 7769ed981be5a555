"""Sparse variational GP regression on inducing points (cugp_sparse_*; Titsias 2009): the truth, the yardstick, the stand-in
and the factors of its tests -- TEST INFRASTRUCTURE, CPU, numpy only; a plain module beside tests/truth.py and
tests/truth_loo.py, which it imports and leaves as they are.

With Kuu = k(Z, Z) + eps I, Kuf = k(Z, X), Qff = Kfu Kuu^-1 Kuf, s2 = exp(2 theta_n), sf2 = exp(2 theta_f):

    F = -N/2 log 2 pi - 1/2 log|Qff + s2 I| - 1/2 y'(Qff + s2 I)^-1 y - (N sf2 - tr Qff) / (2 s2)

  truth      `Truth`: F from that DEFINITION in longdouble -- the explicit N x N matrix Qff + s2 I through truth.cholesky --;
             the gradient of -F from the G formulas of include/cugp.h (G_Phi, G_uu, G_uf with explicit Kuu^-1 and Sigma^-1)
             in longdouble; the prediction from Kuu^-1 - Sigma^-1 in longdouble.  tests/test_truth_sparse_cpu.py checks the
             gradient against central differences of the definition.
  yardstick  `computed_form`: the numerically standard form (Lu = chol Kuu, A = Lu^-1 Kuf / s, B = I + A A', LB = chol B,
             c = LB^-1 A y / s) in fp64 numpy / LAPACK on the whole data at once, triangular solves, explicit M x N weight
             and derivative matrices -- what GPflow's SGPR does --, over the data as given and truth.permutations.
  stand-in   `standin`: the library's formulation in fp64 on other arithmetic: explicit triangular inverses, the data in
             cugp_sparse_plan's chunks, the Gram partials of a chunk added in plan order, q through 128-row slabs, the
             gradient through H, R = Lu^-T H / s2 and 2 G_uu = Lu^-T H2 Lu^-1 -- k_sparse_finalize_targets' final formulas at p = 1.
  errors     F relative; every gradient component relative to max|g| (truth.errors_ll_grad's quantities); the mean the
             largest absolute error; the variance the largest absolute error, floored at 4 ulp of sf2 + s2
  bound      F_SPARSE[family] max(yardstick, 4 ulp of the quantity's scale); F_SPARSE is fixed below from the stand-in's
             ratios measured on the CPU (docs/ACCURACY.md has the table), never from the GPU's errors.
"""
import ctypes as C

import numpy as np

import truth
import truth_ard_matern as tam  # (adds "matern52_ard" to truth.FAMILIES)
from conftest import HP_DEFAULT, synth

LD = truth.LD
U4 = truth.U4
JITTER = 1e-6
NT = 20
LOG2PI = np.log(LD(8) * np.arctan(LD(1)))      # log 2 pi in longdouble

_ARD17 = truth.ARD_CASES["n300_d17"]
_ARD3 = truth.ARD_CASES["n257_d3"]
_ARD33 = truth.ARD_CASES["n515_d33"]
_LIVE33 = truth.LIVE_CASES["n515_d33"]
CHUNK_DEFAULT = 16384                          # what chunk_rows = 0 stands for (include/cugp.h: cugp_sparse_create)
# name -> (family, N, M, d, chunk_rows, hyper-parameters (of the existing case tables), box half-width of synth, duplicates)
CASES = {
    "se_n128_m128": ("se", 128, 128, 2, 128, HP_DEFAULT, 4.0, False),         # no padding anywhere, one chunk
    "se_n300_m65": ("se", 300, 65, 2, 128, HP_DEFAULT, 4.0, False),           # three chunks, the last of 44 rows; identity padding of mpad
    "se_n1300_m200": ("se", 1300, 200, 6, 512, truth.HP_A, 2.5, False),       # two M tiles, three output tiles, split-k of 2
    "matern32_n300_m65": ("matern32", 300, 65, 2, 128, HP_DEFAULT, 4.0, False),
    "ard_n300_m130_d17": ("ard", 300, 130, 17, 256, list(_ARD17[2]) + [_ARD17[3], _ARD17[4]], _ARD17[5], False),
    "matern52_ard_n257_m64": ("matern52_ard", 257, 64, 3, 128, list(_ARD3[2]) + [_ARD3[3], _ARD3[4]], _ARD3[5], False),
    "se_n300_dup60": ("se", 300, 120, 2, 128, HP_DEFAULT, 4.0, True),         # Z = 60 rows and the same rows + 1e-4
    # chunk_rows 0 (the library's 16384): one 896-row pass, the Gram launch split in 3 with kstep 304 -- 19, 19 and 18
    # stages of 16, an odd count and a shorter last split --, row ranges of 5, 5 and 4 tiles in the Z pass
    "se_n800_m65_d3_c0": ("se", 800, 65, 3, 0, HP_DEFAULT, 4.0, False),
    "matern52_n800_m65_d3_c0": ("matern52", 800, 65, 3, 0, HP_DEFAULT, 4.0, False),
    # two passes (896 rows split in 3, then 104 accumulated behind them), two M tiles
    "matern32_ard_n1000_m130": ("matern32_ard", 1000, 130, 3, 896, list(_ARD3[2]) + [_ARD3[3], _ARD3[4]], _ARD3[5], False),
    "matern32_ard_n257_m64": ("matern32_ard", 257, 64, 3, 128, list(_ARD3[2]) + [_ARD3[3], _ARD3[4]], _ARD3[5], False),
    # mpad 384 (six lower output tiles): one 1408-row pass split in 5 with kstep 288, Z ranges of 5, 5, 5, 5 and 2 tiles
    "se_n1300_m260_c0": ("se", 1300, 260, 6, 0, truth.HP_A, 2.5, False),
    # d an exact multiple of the feature chunk DC = 16; three feature chunks, the last of one feature
    "matern52_n300_m65_d32": ("matern52", 300, 65, 32, 128, _LIVE33[2], _LIVE33[3], False),
    "ard_n300_m65_d33": ("ard", 300, 65, 33, 128, list(_ARD33[2]) + [_ARD33[3], _ARD33[4]], _ARD33[5], False),
    "se_n300_m16_d3": ("se", 300, 16, 3, 0, HP_DEFAULT, 4.0, False),          # the model of the two-pass prediction
}
DUP_SHIFT = 1e-4

EXISTING = {"se": truth.F, "matern32": truth.F_MATERN, "matern52": truth.F_MATERN, "ard": truth.F_ARD,
            "matern52_ard": truth.F_ARD, "matern32_ard": truth.F_ARD}
# The larger of the family's existing factor and truth.factor_rule of the largest stand-in / yardstick ratio over CASES
# (tests/test_truth_sparse_cpu.py measures and asserts; docs/ACCURACY.md: the table).
# Largest stand-in ratios measured: se 3.07 (g0 of se_n1300_m200; factor_rule 8), matern32 1.13, matern52 0.78, ard 2.35,
# matern52_ard 1.60, matern32_ard 2.27 (gf of matern32_ard_n1000_m130) (factor_rule 2 to 8); at the wide test points 1.63
# at most (the variance of se_n1300_m260_c0 at nt = 257; factor_rule 4): every family's existing factor stands.
F_SPARSE = dict(EXISTING)


def chunk_of(chunk_rows):
    """chunk_rows as the library resolves it: 0 is its default (cugp_sparse_dims reports the same)."""
    return chunk_rows if chunk_rows > 0 else CHUNK_DEFAULT


def inputs(name):
    """-> (X, y, Z, Xt, cov, chunk_rows): synth data of the case, its inducing inputs (a fixed-seed subset of the rows,
    ascending; the duplicate case: 60 rows and the same rows shifted by DUP_SHIFT), NT test points in the box (one of them
    a data row) and the family's descriptor."""
    family, N, M, d, chunk, hp, scale, dup = CASES[name]
    X, y = synth(N, d=d, seed=3 * N + d, scale=scale)
    rows = np.sort(np.random.default_rng(1000 + M).choice(N, M // 2 if dup else M, replace=False))
    Z = np.concatenate([X[rows], X[rows] + DUP_SHIFT]) if dup else X[rows]
    Xt = truth.points(X, d, scale, NT)
    return X, y, np.ascontiguousarray(Z), np.ascontiguousarray(Xt), truth.FAMILIES[family][1](list(hp)), chunk


# ---------------------------------------------------------------------------------------- the covariance, rectangular
def kernel_parts(cov, A, B):
    """(K, [dK / dtheta_l]) between the rows of A and of B in cov's dtype, without noise: one derivative matrix per
    length-scale hyper-parameter (one, ARD d)."""
    T = cov.dtype
    A, B = np.asarray(A, dtype=T), np.asarray(B, dtype=T)
    if hasattr(cov, "w"):
        S = truth.wsqdist(A, B, cov.w)
        if isinstance(cov, tam.ARDMatern):
            K, H = tam.parts(S, cov.sf2, cov.kind)
        else:
            K = cov.sf2 * np.exp(-S / 2)
            H = K
        lead = [None] * len(cov.w)

        def per_dim(c, D2):
            lead[c] = H * D2
        truth.wsqdist(A, B, cov.w, per_dim)
        return K, lead
    S = truth.sqdist(A, B, T) / cov.l2
    if isinstance(cov, truth.Matern):
        K, dK = truth.matern_kernel(S, cov.sf2, cov.kind)
        return K, [dK]
    K = cov.sf2 * np.exp(-S / 2)
    return K, [K * S]


def forward(L, b):
    """L^-1 b by substitution, in the dtype of L."""
    z = np.array(b, dtype=L.dtype)
    for i in range(len(z)):
        z[i] = (z[i] - L[i, :i] @ z[:i]) / L[i, i]
    return z


# ---------------------------------------------------------------------------------------- the truth
def bound_definition(X, y, Z, cov, jitter=JITTER, keep=None):
    """F from the definition in longdouble: the explicit N x N matrix Qff + s2 I and its Cholesky factor."""
    truth.require_extended()
    Xl, Zl = np.asarray(X, dtype=np.float64).astype(LD), np.asarray(Z, dtype=np.float64).astype(LD)
    yl = np.asarray(y, dtype=np.float64).astype(LD)
    N, M = len(yl), len(Zl)
    Kuu, dKuu = kernel_parts(cov, Zl, Zl)
    Kuu[np.arange(M), np.arange(M)] += LD(jitter)
    Kuf, dKuf = kernel_parts(cov, Zl, Xl)
    Tu = truth.tri_inverse(truth.cholesky(Kuu))
    A0 = truth._mm(Tu, Kuf)
    Qff = truth._mm(np.ascontiguousarray(A0.T), A0)
    Cm = Qff.copy()
    Cm[np.arange(N), np.arange(N)] += cov.sn2
    LC = truth.cholesky(Cm)
    z = forward(LC, yl)
    F = -N * LOG2PI / 2 - np.log(np.diag(LC)).sum() - z @ z / 2 - (N * cov.sf2 - np.trace(Qff)) / (2 * cov.sn2)
    if keep is not None:
        keep.update(Xl=Xl, Zl=Zl, yl=yl, Kuu=Kuu, dKuu=dKuu, Kuf=Kuf, dKuf=dKuf, Tu=Tu)
    return F


class Truth:
    """Every checked quantity in longdouble: F (the definition), grad (of -F, the G formulas with explicit Kuu^-1 and
    Sigma^-1), predict(Xt) (from Kuu^-1 - Sigma^-1)."""

    def __init__(self, X, y, Z, cov, jitter=JITTER):
        k = {}
        self.F = bound_definition(X, y, Z, cov, jitter, k)
        self.cov, self.Zl = cov, k["Zl"]
        yl, Kuu, Kuf, Tu = k["yl"], k["Kuu"], k["Kuf"], k["Tu"]
        N, M = len(yl), len(Kuu)
        s2, sf2 = cov.sn2, cov.sf2
        Kuui = truth.gram_lower(Tu)
        Phi = truth._mm(Kuf, np.ascontiguousarray(Kuf.T))
        v = Kuf @ yl
        Ts = truth.tri_inverse(truth.cholesky(Kuu + Phi / s2))
        Si = truth.gram_lower(Ts)
        beta = Si @ v / s2
        bb = np.outer(beta, beta)
        G_phi = (Kuui - Si - bb) / (2 * s2)
        G_uu = Kuui / 2 - (Si + bb) / 2 - Kuui @ Phi @ Kuui / (2 * s2)
        G_uf = 2 * truth._mm(G_phi, Kuf) + np.outer(beta / s2, yl)
        Kuu0 = Kuu.copy()
        Kuu0[np.arange(M), np.arange(M)] -= LD(jitter)                # (eps is no hyper-parameter: it has no derivative)
        dF = [(G_uu * a).sum() + (G_uf * b).sum() for a, b in zip(k["dKuu"], k["dKuf"])]
        dF.append(2 * ((G_uu * Kuu0).sum() + (G_uf * Kuf).sum()) - N * sf2 / s2)
        dF.append(2 * s2 * (-N / (2 * s2) + np.trace(Si @ Phi) / (2 * s2 * s2) + yl @ yl / (2 * s2 * s2)
                            - v @ beta / (s2 * s2) + beta @ Phi @ beta / (2 * s2 * s2)
                            + (N * sf2 - np.trace(Kuui @ Phi)) / (2 * s2 * s2)))
        self.grad = -np.array(dF, dtype=LD)
        self.D, self.beta = Kuui - Si, beta

    def predict(self, Xt, with_noise=True):
        Ks = kernel_parts(self.cov, np.asarray(Xt, dtype=np.float64).astype(LD), self.Zl)[0]          # [nt, M]
        var = self.cov.sf2 - ((Ks @ self.D) * Ks).sum(1)
        return Ks @ self.beta, var + self.cov.sn2 if with_noise else var


# ---------------------------------------------------------------------------------------- fp64: the yardstick
def computed_form(cov, X, y, Z, Xt, jitter=JITTER):
    """The computed form in fp64, the whole data at once, LAPACK / BLAS: -> (F, grad of -F, mean, var with noise)."""
    import scipy.linalg as sl
    c = cov.fp64()
    X, y, Z = (np.asarray(a, dtype=np.float64) for a in (X, y, Z))
    N, M = len(y), len(Z)
    s2, sf2 = float(c.sn2), float(c.sf2)
    s = np.sqrt(s2)
    Kuu0, dKuu = kernel_parts(c, Z, Z)
    Kuf, dKuf = kernel_parts(c, Z, X)
    Lu = np.linalg.cholesky(Kuu0 + jitter * np.eye(M))
    A = sl.solve_triangular(Lu, Kuf, lower=True) / s
    AAt = A @ A.T
    LB = np.linalg.cholesky(np.eye(M) + AAt)
    Ay = A @ y
    cv = sl.solve_triangular(LB, Ay, lower=True) / s
    F = (-N / 2 * np.log(2 * np.pi) - np.log(np.diag(LB)).sum() - N / 2 * np.log(s2) - y @ y / (2 * s2) + cv @ cv / 2
         - N * sf2 / (2 * s2) + np.trace(AAt) / 2)
    # the gradient through Lu and LB: Sigma^-1 = Lu^-T B^-1 Lu^-1, gamma = Lu^T beta
    gam = sl.solve_triangular(LB, cv, lower=True, trans="T")
    Binv = sl.cho_solve((LB, True), np.eye(M))
    Hm = np.eye(M) - Binv - np.outer(gam, gam)
    beta = sl.solve_triangular(Lu, gam, lower=True, trans="T")
    G_uf = sl.solve_triangular(Lu, Hm @ (A * s), lower=True, trans="T") / s2 + np.outer(beta / s2, y)
    Y = sl.solve_triangular(Lu, Hm - AAt, lower=True, trans="T")                  # Lu^-T (H - P / s2)
    G_uu = sl.solve_triangular(Lu, Y.T, lower=True, trans="T").T / 2
    dF = [(G_uu * a).sum() + (G_uf * b).sum() for a, b in zip(dKuu, dKuf)]
    dF.append(2 * ((G_uu * Kuu0).sum() + (G_uf * Kuf).sum()) - N * sf2 / s2)
    Pm = AAt * s2
    qg = (A @ y) * s @ gam                                                         # v'beta
    dF.append(-N + (M - np.trace(Binv)) + (y @ y - qg + N * sf2 - np.trace(Pm)) / s2 - gam @ gam)
    Ks = kernel_parts(c, np.asarray(Xt, dtype=np.float64), Z)[0]
    Wt = sl.solve_triangular(Lu, Ks.T, lower=True)
    Vt = sl.solve_triangular(LB, Wt, lower=True)
    return F, -np.array(dF), Vt.T @ cv, sf2 - (Wt * Wt).sum(0) + (Vt * Vt).sum(0) + s2


# ---------------------------------------------------------------------------------------- fp64: the stand-in
def plan(n, m, chunk_rows):
    """cugp_sparse_plan replayed: [(row0, rows, rows_padded, split, kstep)] (pure arithmetic in the library: no device)."""
    from cugp_amd import capi
    out = (C.c_int * 5)()
    passes, i = [], 0
    while True:
        count = capi.lib().cugp_sparse_plan(int(n), int(m), int(chunk_rows), i, out)
        assert count > 0, capi.lib().cugp_last_error()
        passes.append(tuple(out))
        i += 1
        if i >= count:
            return passes


def standin(cov, X, y, Z, Xt, chunk_rows, jitter=JITTER, mutate=None):
    """The library's formulation in fp64 numpy -> (F, grad of -F, mean, var with noise).  mutate: "drop_tr" leaves the
    trace term out of F; "guf_without_2" takes G_Phi Kuf once in G_uf."""
    import scipy.linalg as sl
    c = cov.fp64()
    X, y, Z = (np.asarray(a, dtype=np.float64) for a in (X, y, Z))
    N, M = len(y), len(Z)
    s2, sf2 = float(c.sn2), float(c.sf2)
    Kuu0, dKuu = kernel_parts(c, Z, Z)
    Tu = sl.solve_triangular(np.linalg.cholesky(Kuu0 + jitter * np.eye(M)), np.eye(M), lower=True)
    P, q = np.zeros((M, M)), np.zeros(M)
    chunks = plan(N, M, chunk_rows)
    Ws = []
    for r0, rows, cpad, split, kstep in chunks:
        W = kernel_parts(c, X[r0: r0 + rows], Z)[0] @ Tu.T
        Ws.append(W)
        for sidx in range(split):                                    # the Gram partials in plan order
            Wk = W[sidx * kstep: min((sidx + 1) * kstep, cpad)]
            P = P + Wk.T @ Wk
        for k0 in range(0, rows, 128):                               # q through the 128-row slabs
            q = q + W[k0: k0 + 128].T @ y[r0 + k0: r0 + k0 + 128]
    LB = np.linalg.cholesky(np.eye(M) + P / s2)
    TB = sl.solve_triangular(LB, np.eye(M), lower=True)
    Binv = TB.T @ TB
    cp = TB @ q
    gp = TB.T @ cp
    bp = Tu.T @ gp
    yy, cc, gg, trp = y @ y, cp @ cp, gp @ gp, np.trace(P)
    nsf = N * sf2
    F = ((((-0.5 * N * np.log(2 * np.pi) - np.log(np.diag(LB)).sum()) - 0.5 * N * np.log(s2)) - yy / (2 * s2))
         + cc / (2 * s2 * s2)) - ((nsf - trp) if mutate != "drop_tr" else nsf) / (2 * s2)
    H = np.eye(M) - Binv - np.outer(gp / s2, gp / s2)
    H2 = H - P / s2
    R = (H @ Tu).T / s2
    Guu2 = ((H2 @ Tu).T) @ Tu
    nl = len(dKuu)
    S_uf, S_uu = np.zeros(nl + 1), np.zeros(nl + 1)
    for (r0, rows, cpad, split, kstep), W in zip(chunks, Ws):
        Kc, dKc = kernel_parts(c, X[r0: r0 + rows], Z)
        G = W @ R.T
        if mutate == "guf_without_2":
            G = G / 2
        G = G + np.outer(y[r0: r0 + rows], bp / (s2 * s2))
        S_uf = S_uf + np.array([(G * a).sum() for a in dKc] + [(G * Kc).sum()])
    S_uu = np.array([(Guu2 * a).sum() for a in dKuu] + [(Guu2 * Kuu0).sum()])
    S = S_uf + S_uu / 2
    g = list(-S[:nl])
    g.append(-(2 * S[nl] - nsf / s2))
    g.append(-(((np.sum(1 - np.diag(Binv)) - N) + (((yy - cc / s2) + (nsf - trp)) / s2)) - gg / (s2 * s2)))
    Wt = kernel_parts(c, np.asarray(Xt, dtype=np.float64), Z)[0] @ Tu.T
    Vt = Wt @ TB.T
    return F, np.array(g), Vt @ cp / s2, ((sf2 - (Wt * Wt).sum(1)) + (Vt * Vt).sum(1)) + s2


# ---------------------------------------------------------------------------------------- errors, yardstick, bound
def errors(cov, t, tm, tv, F, grad, mean, var):
    """Errors of one fp64 evaluation against the truth: truth.errors_ll_grad on F and the gradient (the bound under the
    name of the family's first quantity), the largest absolute error of the means and of the variances."""
    return dict(truth.errors_ll_grad(cov, F, grad, t.F, t.grad), **truth.errors_pred(mean, var, tm, tv))


_CASES = {}


def case(name):
    """Inputs, truth, yardstick (noise, first, rest as truth.noise_level's) and floors of a case, once per process."""
    if name not in _CASES:
        X, y, Z, Xt, cov, chunk = inputs(name)
        t = Truth(X, y, Z, cov)
        tm, tv = t.predict(Xt)

        def one(idx):
            return errors(cov, t, tm, tv, *computed_form(cov, X[idx], y[idx], Z, Xt))
        E = [one(idx) for idx in truth.permutations(len(y))]
        Q = cov.quantities
        fl = truth.floors(cov, truth.scales(cov, t.F, t.grad, tm))
        _CASES[name] = dict(X=X, y=y, Z=Z, Xt=Xt, cov=cov, chunk=chunk, t=t, tm=tm, tv=tv, family=CASES[name][0],
                            noise={q: max(e[q] for e in E) for q in Q}, first={q: E[0][q] for q in Q},
                            rest={q: max(e[q] for e in E[1:]) for q in Q}, floor={q: fl[q] for q in Q})
    return _CASES[name]


# ---------------------------------------------------------------------------------------- beyond one test tile
# tests/test_gpu_sparse_wide.py: NT = 20 runs one 128-row test tile, and rows below 128 of k_sparse_predict_finish only.
WIDE_NTS = truth.WIDE_NTS                      # two tiles, one row into the second; two tiles, ragged; three tiles
WIDE_NAMES = ("se_n800_m65_d3_c0", "se_n1300_m260_c0", "matern32_ard_n1000_m130", "ard_n300_m65_d33")
WIDE_Z_ROW = 128                               # the test row that is Z[0]: the first row of the second tile at every size
TWO_PASS_NAME = "se_n300_m16_d3"               # the model of the prediction that takes two passes
_WIDE = {}


def wide_points(name, nt, z_row=WIDE_Z_ROW, data_row=None):
    """truth.wide_points of the case's data (the last but one a training row) with row z_row replaced by Z[0] -- a test point
    that is an inducing input --, and, where given, row data_row by a data row."""
    X, _, Z, _, _, _ = inputs(name)
    Xt = truth.wide_points(X, nt, CASES[name][6])
    Xt[z_row] = Z[0]
    if data_row is not None:
        Xt[data_row] = X[len(X) // 3]
    return np.ascontiguousarray(Xt)


def wide_case(name, nt, z_row=WIDE_Z_ROW, data_row=None):
    """The case at nt test points: Xt, the truth's mean and variance (with noise) there and the yardstick -- computed_form at
    the same points over the data as given and truth.permutations --, once per process.  The floors are case()'s."""
    key = (name, nt, z_row, data_row)
    if key not in _WIDE:
        c = case(name)
        Xt = wide_points(name, nt, z_row, data_row)
        tm, tv = c["t"].predict(Xt)
        E = [truth.errors_pred(*computed_form(c["cov"], c["X"][idx], c["y"][idx], c["Z"], Xt)[2:], tm, tv)
             for idx in truth.permutations(len(c["y"]))]
        _WIDE[key] = dict(Xt=Xt, tm=tm, tv=tv, noise={q: max(e[q] for e in E) for q in ("mean", "var")},
                          first={q: E[0][q] for q in ("mean", "var")}, rest={q: max(e[q] for e in E[1:]) for q in ("mean", "var")})
    return _WIDE[key]


def wide_ratios(c, w, mean, var):
    """error / max(yardstick, floor) of the means and variances at a wide_case's points."""
    e = truth.errors_pred(mean, var, w["tm"], w["tv"])
    return {q: e[q] / max(w["noise"][q], c["floor"][q]) for q in ("mean", "var")}


def hold_wide(rep, c, w, mean, var, latent_var=None, tag=""):
    """Adds the means and variances (with noise) at a wide_case's points to the accuracy.Report `rep` under the bound
    F_SPARSE[family]; with latent_var also the variances without noise against the truth's."""
    e = truth.errors_pred(mean, var, w["tm"], w["tv"])
    F = F_SPARSE[c["family"]]
    for q in ("mean", "var"):
        rep.add(tag + q, e[q], w["noise"][q], c["floor"][q], F)
    if latent_var is not None:
        el = float(np.max(np.abs(np.asarray(latent_var).astype(LD) - (w["tv"] - c["cov"].sn2))))
        rep.add(tag + "latent_var", el, w["noise"]["var"], c["floor"]["var"], F)


def ratios(c, out):
    """error / max(yardstick, floor) per quantity of one evaluation `out` = (F, grad, mean, var)."""
    e = errors(c["cov"], c["t"], c["tm"], c["tv"], *out)
    return {q: e[q] / max(c["noise"][q], c["floor"][q]) for q in c["cov"].quantities}


def hold(rep, c, F, grad, mean, var, tag=""):
    """Adds every checked quantity of one evaluation to the accuracy.Report `rep` under the bound F_SPARSE[family]."""
    e = errors(c["cov"], c["t"], c["tm"], c["tv"], F, grad, mean, var)
    for q in c["cov"].quantities:
        rep.add(tag + q, e[q], c["noise"][q], c["floor"][q], F_SPARSE[c["family"]])


def assert_yardstick_is_sane(c, tag):
    """The data as given is no outlier among the permutations, and no yardstick exceeds truth.YARDSTICK_CAP of its scale."""
    for q in c["cov"].quantities:
        assert c["first"][q] <= c["cov"].F * max(c["rest"][q], c["floor"][q]), (tag, q, c["first"][q], c["rest"][q])
        assert c["noise"][q] <= truth.YARDSTICK_CAP * c["floor"][q] / U4, (tag, q, c["noise"][q])
