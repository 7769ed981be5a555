"""The gradient of the sparse model's bound with respect to the inducing inputs Z (cugp_sparse_bound_grad_z): the truth, the
yardstick, the stand-in and the factors of its tests -- TEST INFRASTRUCTURE, CPU, numpy only; a plain module beside
tests/truth_sparse.py, which it imports and leaves as it is.

With H the factor of the input derivatives (SE and SE-ARD: k itself; Matern 3/2: 3 sf2 e^-a; Matern 5/2: (5/3) sf2 (1 + a)
e^-a) and s_c = 1 / l^2 (ARD: w_c^2):  dk(z_j, x) / dz_jc = -H(z_j, x) (z_jc - x_c) s_c  and

    dF / dz_jc = -s_c sum_i G_uf[j,i] H(z_j,x_i) (z_jc - x_ic)  -  s_c sum_b (2 G_uu)[j,b] H(z_j,z_b) (z_jc - z_bc)

(row j and column j of Kuu both move with z_j: weight 1 on the symmetric 2 G_uu; the diagonal and the jitter have no
derivative).  Everything below is the gradient of -F, as the library returns it.

  truth      `truth_gz`: the formula in longdouble with the explicit G_uf, G_uu of truth_sparse.Truth (Kuu^-1 and Sigma^-1
             through truth.cholesky).  tests/test_truth_sparse_z_cpu.py checks it against central differences of
             truth_sparse.bound_definition in Z.
  yardstick  `computed_gz`: truth_sparse.computed_form's G_uf, G_uu (fp64 numpy / LAPACK, triangular solves, the whole data
             at once) in the same formula, over the data as given and truth.permutations.
  stand-in   `standin_gz`: the library's formulation in fp64 on other arithmetic: per chunk G_c = W_c R^T + y (beta' / s2^2)^T,
             then 2 G_uu = Lu^-T H2 Lu^-1, chunks in cugp_sparse_plan's order, the square last, differences before products,
             s_c and the sign once at the end.
  error      the largest |gZ - truth| over all entries relative to max|truth gZ|, floored at truth.U4
  bound      F_SPARSE_Z[family] max(yardstick, 4 ulp); F_SPARSE_Z is fixed below from the stand-in's ratios measured on the
             CPU (docs/ACCURACY.md has the table), never from the GPU's errors.

Cases.  Z is a fixed-seed subset of the rows as in truth_sparse.inputs, the jitter 1e-6: the smallest shapes that reach each
way the pass can go wrong.  truth_sparse's d = 2 cases are left out because the REFERENCE itself leaves
truth.YARDSTICK_CAP (1e-9) on them: the fp64 computed form over the 8 permutations reads 6.7e-10 on se_n300_m65 (and 1.7e-8
on a 256 x 128 variant at d = 2), 6.0e-9 on se_n300_dup60; their d = 3 siblings below read 1e-13.  se_n128_m128 is left out
because there Z is all the data, the bound is tight and |gZ| ~ 2e-7 is pure cancellation.
"""
import numpy as np

import truth
import truth_ard_matern as tam
import truth_sparse as ts
from conftest import HP_DEFAULT, synth

LD = truth.LD
U4 = truth.U4
JITTER = ts.JITTER

# name -> (family, N, M, d, chunk_rows, what it reaches); a name of truth_sparse.CASES takes that case's inputs as they are,
# the others its recipe (synth(N, d, seed = 3 N + d, scale = 4), HP_DEFAULT)
CASES = {
    "se_n256_m128_d3": ("se", 256, 128, 3, 128, "no padding anywhere, two chunks"),
    "se_n300_m65_d3": ("se", 300, 65, 3, 128, "ragged last chunk of 44 rows, mp padding beyond column 65"),
    "se_n1300_m200": ("se", 1300, 200, 6, 512, "several row tiles per workgroup range, four column tiles"),
    "matern32_n300_m65": ("matern32", 300, 65, 2, 128, "Matern 3/2"),
    "matern52_n300_m65_d3": ("matern52", 300, 65, 3, 128, "Matern 5/2"),
    "ard_n300_m130_d17": ("ard", 300, 130, 17, 256, "two feature chunks (d = 17 > DC)"),
    "matern52_ard_n257_m64": ("matern52_ard", 257, 64, 3, 128, "Matern-ARD"),
    "se_n800_m65_d3_c0": ("se", 800, 65, 3, 0, "the default chunk: one 896-row pass, row ranges of 5, 5 and 4 tiles"),
    "matern52_n800_m65_d3_c0": ("matern52", 800, 65, 3, 0, "the same shape, Matern 5/2"),
    "matern32_ard_n1000_m130": ("matern32_ard", 1000, 130, 3, 896, "Matern-3/2-ARD: two passes, two M tile rows"),
    "matern32_ard_n257_m64": ("matern32_ard", 257, 64, 3, 128, "Matern-3/2-ARD"),
    "se_n1300_m260_c0": ("se", 1300, 260, 6, 0, "mpad 384: row ranges of 5, 5, 5, 5 and 2 tiles, six column tiles"),
    "matern52_n300_m65_d32": ("matern52", 300, 65, 32, 128, "d an exact multiple of DC: the last chunk stays staged, full"),
    "ard_n300_m65_d33": ("ard", 300, 65, 33, 128, "three feature chunks, the last of one feature"),
    "se_n300_m16_d3": ("se", 300, 16, 3, 0, "the model of the two-pass prediction"),
}

# The larger of F_SPARSE[family] and truth.factor_rule of the largest stand-in / yardstick ratio over CASES
# (tests/test_truth_sparse_z_cpu.py measures and asserts; docs/ACCURACY.md: the table).
# Largest stand-in ratios measured: se 1.21 (se_n256_m128_d3; factor_rule 4), matern32 0.94, matern52 1.19
# (matern52_n300_m65_d32), ard 1.21, matern52_ard 0.99, matern32_ard 0.71 (factor_rule 2 to 4): every family's F_SPARSE
# (8, 16, 16, 32, 32, 32) stands.
F_SPARSE_Z = dict(ts.F_SPARSE)


def inputs(name):
    """-> (X, y, Z, cov, chunk_rows) of a case."""
    family, N, M, d, chunk, _ = CASES[name]
    if name in ts.CASES:
        assert ts.CASES[name][:5] == (family, N, M, d, chunk)
        X, y, Z, _, cov, chunk = ts.inputs(name)
        return X, y, Z, cov, chunk
    X, y = synth(N, d=d, seed=3 * N + d, scale=4.0)
    rows = np.sort(np.random.default_rng(1000 + M).choice(N, M, replace=False))
    return X, y, np.ascontiguousarray(X[rows]), truth.FAMILIES[family][1](list(HP_DEFAULT)), chunk


Z_SLOTS = 512                     # SPARSE_Z_SLOTS of cugp_amd/csrc/kernels.h (tests/test_truth_sparse_z_cpu.py reads it there)


def z_ranges(rows_pad, mpad, d, slots=Z_SLOTS):
    """sparse_z_shape (cugp_amd/csrc/sparse_gfx950.h) replayed: the 64-row tiles of each row range of one k_trace_cross_z launch
    over rows_pad rows -- the last range is what the clamp to the tile count leaves."""
    tiles = rows_pad // 64
    ranges = max(1, min(slots // (mpad // 64), rows_pad // 256))
    while ranges > 1 and ranges * mpad * d * 8 > 1 << 30:
        ranges -= 1
    per = -(-tiles // ranges)
    return [min(per, tiles - t0) for t0 in range(0, tiles, per)]


# ---------------------------------------------------------------------------------------- the formula
def h_factor(cov, A, B):
    """(H between the rows of A and of B, s_c [d]) in cov's dtype."""
    T = cov.dtype
    A, B = np.asarray(A, dtype=T), np.asarray(B, dtype=T)
    if hasattr(cov, "w"):
        S = truth.wsqdist(A, B, cov.w)
        H = tam.parts(S, cov.sf2, cov.kind)[1] if isinstance(cov, tam.ARDMatern) else cov.sf2 * np.exp(-S / 2)
        return H, cov.w * cov.w
    S = truth.sqdist(A, B, T) / cov.l2
    sc = np.full(A.shape[1], 1 / cov.l2, dtype=T)
    if isinstance(cov, truth.Matern):
        return tam.parts(S, cov.sf2, cov.kind)[1], sc
    return cov.sf2 * np.exp(-S / 2), sc


def weighted_differences(WH, P, Z):
    """S[j][c] = sum_i WH[j][i] (p_ic - z_jc): the difference first, then the product."""
    out = np.zeros(Z.shape, dtype=WH.dtype)
    for c in range(Z.shape[1]):
        out[:, c] = (WH * (P[:, c][None, :] - Z[:, c][:, None])).sum(1)
    return out


def formula(cov, G_uf, G_uu2, X, Z):
    """The gradient of -F with respect to Z [M, d] from G_uf [M, N] and 2 G_uu [M, M], in cov's dtype."""
    T = cov.dtype
    X, Z = np.asarray(X, dtype=T), np.asarray(Z, dtype=T)
    Hf, sc = h_factor(cov, Z, X)
    Hu = h_factor(cov, Z, Z)[0]
    S = weighted_differences(G_uf * Hf, X, Z) + weighted_differences(G_uu2 * Hu, Z, Z)
    return -(S * sc[None, :])


# ---------------------------------------------------------------------------------------- the truth
def truth_gz(X, y, Z, cov, jitter=JITTER):
    """Longdouble: truth_sparse.Truth's G_uf and G_uu (explicit Kuu^-1 and Sigma^-1) in the formula."""
    k = {}
    ts.bound_definition(X, y, Z, cov, jitter, k)
    yl, Kuu, Kuf, Tu = k["yl"], k["Kuu"], k["Kuf"], k["Tu"]
    s2 = cov.sn2
    Kuui = truth.gram_lower(Tu)
    Phi = truth._mm(Kuf, np.ascontiguousarray(Kuf.T))
    v = Kuf @ yl
    Si = truth.gram_lower(truth.tri_inverse(truth.cholesky(Kuu + Phi / s2)))
    beta = Si @ v / s2
    bb = np.outer(beta, beta)
    G_phi = (Kuui - Si - bb) / (2 * s2)
    G_uu = Kuui / 2 - (Si + bb) / 2 - Kuui @ Phi @ Kuui / (2 * s2)
    G_uf = 2 * truth._mm(G_phi, Kuf) + np.outer(beta / s2, yl)
    return formula(cov, G_uf, 2 * G_uu, k["Xl"], k["Zl"])


# ---------------------------------------------------------------------------------------- fp64: the yardstick
def computed_gz(cov, X, y, Z, jitter=JITTER):
    """truth_sparse.computed_form's G_uf and G_uu (fp64, LAPACK, the whole data at once) in the formula."""
    import scipy.linalg as sl
    c = cov.fp64()
    X, y, Z = (np.asarray(a, dtype=np.float64) for a in (X, y, Z))
    M = len(Z)
    s2 = float(c.sn2)
    s = np.sqrt(s2)
    Kuu0 = ts.kernel_parts(c, Z, Z)[0]
    Kuf = ts.kernel_parts(c, Z, X)[0]
    Lu = np.linalg.cholesky(Kuu0 + jitter * np.eye(M))
    A = sl.solve_triangular(Lu, Kuf, lower=True) / s
    AAt = A @ A.T
    LB = np.linalg.cholesky(np.eye(M) + AAt)
    cv = sl.solve_triangular(LB, A @ y, lower=True) / s
    gam = sl.solve_triangular(LB, cv, lower=True, trans="T")
    Binv = sl.cho_solve((LB, True), np.eye(M))
    Hm = np.eye(M) - Binv - np.outer(gam, gam)
    beta = sl.solve_triangular(Lu, gam, lower=True, trans="T")
    G_uf = sl.solve_triangular(Lu, Hm @ (A * s), lower=True, trans="T") / s2 + np.outer(beta / s2, y)
    Y = sl.solve_triangular(Lu, Hm - AAt, lower=True, trans="T")
    G_uu2 = sl.solve_triangular(Lu, Y.T, lower=True, trans="T").T
    return formula(c, G_uf, G_uu2, X, Z)


# ---------------------------------------------------------------------------------------- fp64: the stand-in
MUTATIONS = ("square_half", "no_rank_one", "s0_for_all")


def standin_gz(cov, X, y, Z, chunk_rows, jitter=JITTER, mutate=None):
    """The library's formulation in fp64 numpy.  mutate: "square_half" weighs the square term 1/2 as the hyper-parameter
    trace does; "no_rank_one" drops y (beta' / s2^2)^T from G_c; "s0_for_all" applies dimension 0's s_c to every dimension."""
    import scipy.linalg as sl
    c = cov.fp64()
    X, y, Z = (np.asarray(a, dtype=np.float64) for a in (X, y, Z))
    N, M = len(y), len(Z)
    s2 = float(c.sn2)
    Kuu0 = ts.kernel_parts(c, Z, Z)[0]
    Tu = sl.solve_triangular(np.linalg.cholesky(Kuu0 + jitter * np.eye(M)), np.eye(M), lower=True)
    P, q = np.zeros((M, M)), np.zeros(M)
    chunks = ts.plan(N, M, chunk_rows)
    Ws = []
    for r0, rows, cpad, split, kstep in chunks:
        W = ts.kernel_parts(c, X[r0: r0 + rows], Z)[0] @ Tu.T
        Ws.append(W)
        for sidx in range(split):
            Wk = W[sidx * kstep: min((sidx + 1) * kstep, cpad)]
            P = P + Wk.T @ Wk
        for k0 in range(0, rows, 128):
            q = q + W[k0: k0 + 128].T @ y[r0 + k0: r0 + k0 + 128]
    TB = sl.solve_triangular(np.linalg.cholesky(np.eye(M) + P / s2), np.eye(M), lower=True)
    Binv = TB.T @ TB
    gp = TB.T @ (TB @ q)
    bp = Tu.T @ gp
    H = np.eye(M) - Binv - np.outer(gp / s2, gp / s2)
    H2 = H - P / s2
    R = (H @ Tu).T / s2
    Guu2 = ((H2 @ Tu).T) @ Tu
    S = np.zeros(Z.shape)
    for (r0, rows, cpad, split, kstep), W in zip(chunks, Ws):        # chunks ascending: G_c is [rows][M], as the library holds it
        Xc = X[r0: r0 + rows]
        G = W @ R.T
        if mutate != "no_rank_one":
            G = G + np.outer(y[r0: r0 + rows], bp / (s2 * s2))
        S = S + weighted_differences((G * h_factor(c, Xc, Z)[0]).T, Xc, Z)
    sq = weighted_differences((Guu2 * h_factor(c, Z, Z)[0]).T, Z, Z)  # the square last: rows b, columns j
    S = S + (sq / 2 if mutate == "square_half" else sq)
    sc = h_factor(c, Z[:1], Z[:1])[1]
    if mutate == "s0_for_all":
        sc = np.full_like(sc, sc[0])
    return -(S * sc[None, :])


# ---------------------------------------------------------------------------------------- errors, yardstick, bound
def error(gz, tz):
    """The largest |gZ - truth| over all entries relative to max|truth gZ|."""
    tz = np.asarray(tz, dtype=LD)
    return float(np.max(np.abs(np.asarray(gz, dtype=np.float64).astype(LD) - tz)) / np.max(np.abs(tz)))


_CASES = {}


def case(name):
    """Inputs, truth and yardstick (noise: the largest over the data as given and truth.permutations; first, rest) of a
    case, once per process."""
    if name not in _CASES:
        X, y, Z, cov, chunk = inputs(name)
        tz = truth_gz(X, y, Z, cov)
        E = [error(computed_gz(cov, X[idx], y[idx], Z), tz) for idx in truth.permutations(len(y))]
        _CASES[name] = dict(X=X, y=y, Z=Z, cov=cov, chunk=chunk, tz=tz, family=CASES[name][0], noise=max(E), first=E[0],
                            rest=max(E[1:]), floor=U4)
    return _CASES[name]


def ratio(c, gz):
    return error(gz, c["tz"]) / max(c["noise"], c["floor"])


def hold(rep, c, gz, tag=""):
    """Adds gZ of one evaluation to the accuracy.Report `rep` under the bound F_SPARSE_Z[family]."""
    rep.add(tag + "gZ", error(gz, c["tz"]), c["noise"], c["floor"], F_SPARSE_Z[c["family"]])


def assert_yardstick_is_sane(c, tag):
    """truth_sparse.assert_yardstick_is_sane's two conditions on the gZ metric: the data as given is no outlier among the
    permutations, and the yardstick stays within truth.YARDSTICK_CAP (relative)."""
    assert c["first"] <= c["cov"].F * max(c["rest"], c["floor"]), (tag, c["first"], c["rest"])
    assert c["noise"] <= truth.YARDSTICK_CAP, (tag, c["noise"])
