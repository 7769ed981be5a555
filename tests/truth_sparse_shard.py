"""The sparse variational model with its rows sharded over ranks (cugp_sparse_sharded_*): the cases,
the stand-in and the factors of its tests -- TEST INFRASTRUCTURE, CPU, numpy only; a plain module beside
tests/truth_sparse.py and tests/truth_sparse_z.py, which it imports and leaves as they are.

The model is truth_sparse's: the bound, its gradients and the prediction of ALL rows do not depend on how the rows are cut,
so the truth and the yardstick of a sharded case are those of the truth_sparse case it is built over.

  cases      SHARD_CASES: (case of truth_sparse.CASES, row counts of the shards) -- contiguous row blocks in order
  stand-in   `standin_sharded`: truth_sparse.standin restated with the sums the library takes in global shard order: every
             shard runs cugp_sparse_plan's chunks over its own rows into P_k, q_k, y_k'y_k, n_k and S_uf,k; P, q, y'y, N and
             S_uf are the first shard's with every further one added as a = a + b.  With one shard it is truth_sparse.standin
             bit for bit (tests/test_truth_sparse_shard_cpu.py).
  bound      F_SPARSE_SHARD[family] max(yardstick, 4 ulp of the quantity's scale), fixed below from the stand-in's ratios
             measured on the CPU (docs/ACCURACY.md has the table), never from the GPU's errors.
"""
import numpy as np

import truth
import truth_sparse as ts
import truth_sparse_z as tz

JITTER = ts.JITTER
NT = ts.NT

# (case of truth_sparse.CASES, rows of each shard)
SHARD_CASES = (
    ("se_n300_m65", (171, 128, 1)),                 # more than a tile, exactly a tile, one row
    ("se_n300_m65", (300,)),                        # one shard: SparseGP's bits
    ("se_n128_m128", (26, 26, 26, 26, 24)),         # five shards below a tile each
    ("se_n1300_m200", (700, 600)),                  # two M tiles and split-k inside a shard
    ("ard_n300_m130_d17", (129, 127, 44)),
    ("matern32_ard_n1000_m130", (900, 100)),        # two passes in shard 0
    ("matern52_n800_m65_d3_c0", (400, 400)),
    ("se_n300_dup60", (150, 150)),
)

# The largest stand-in / yardstick ratios of standin_sharded over SHARD_CASES, measured on the CPU
# (tests/test_truth_sparse_shard_cpu.py prints and asserts; docs/ACCURACY.md: the table), stay below every family's
# F_SPARSE: the factors stand.
F_SPARSE_SHARD = dict(ts.F_SPARSE)
F_SPARSE_SHARD_Z = dict(tz.F_SPARSE_Z)

MUTATIONS = ("yy_without_a_shard", "suf_last_shard_twice")


def case_id(sc):
    return "%s-%s" % (sc[0], "_".join(str(n) for n in sc[1]))


def blocks(counts):
    """[(row0, rows)] of contiguous blocks with the given row counts."""
    out, r0 = [], 0
    for n in counts:
        out.append((r0, int(n)))
        r0 += int(n)
    return out


def shards_of(name, counts):
    """-> ([(X_k, y_k)], Z, Xt, cov, chunk_rows) of a sharded case: the truth_sparse case's rows cut into blocks."""
    X, y, Z, Xt, cov, chunk = ts.inputs(name)
    assert sum(counts) == len(y) and min(counts) >= 1
    return [(np.ascontiguousarray(X[r0:r0 + n]), np.ascontiguousarray(y[r0:r0 + n])) for r0, n in blocks(counts)], Z, Xt, cov, chunk


def standin_sharded(cov, shards, Z, Xt, chunk_rows, jitter=JITTER, mutate=None):
    """truth_sparse.standin with the sums over the shards in global shard order -> (F, grad of -F, mean, var with noise).
    mutate: "yy_without_a_shard" leaves the last shard out of y'y; "suf_last_shard_twice" adds the last shard's S_uf twice."""
    import scipy.linalg as sl
    c = cov.fp64()
    Z = np.asarray(Z, dtype=np.float64)
    shards = [(np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64)) for X, y in shards]
    M = len(Z)
    s2, sf2 = float(c.sn2), float(c.sf2)
    Kuu0, dKuu = ts.kernel_parts(c, Z, Z)
    Tu = sl.solve_triangular(np.linalg.cholesky(Kuu0 + jitter * np.eye(M)), np.eye(M), lower=True)
    stats = []
    for X, y in shards:                                               # phase 1, per shard: truth_sparse.standin's chunk loop
        Pk, qk = np.zeros((M, M)), np.zeros(M)
        chunks = ts.plan(len(y), M, chunk_rows)
        Ws = []
        for r0, rows, cpad, split, kstep in chunks:
            W = ts.kernel_parts(c, X[r0: r0 + rows], Z)[0] @ Tu.T
            Ws.append(W)
            for sidx in range(split):
                Wk = W[sidx * kstep: min((sidx + 1) * kstep, cpad)]
                Pk = Pk + Wk.T @ Wk
            for k0 in range(0, rows, 128):
                qk = qk + W[k0: k0 + 128].T @ y[r0 + k0: r0 + k0 + 128]
        stats.append((Pk, qk, y @ y, len(y), chunks, Ws))
    P, q, yy, N = stats[0][0], stats[0][1], stats[0][2], stats[0][3]   # the first term copied ...
    for k, (Pk, qk, yyk, nk, _, _) in enumerate(stats[1:], 1):        # ... every further one added, in shard order
        P, q, N = P + Pk, q + qk, N + nk
        if not (mutate == "yy_without_a_shard" and k == len(stats) - 1):
            yy = yy + yyk
    LB = np.linalg.cholesky(np.eye(M) + P / s2)
    TB = sl.solve_triangular(LB, np.eye(M), lower=True)
    Binv = TB.T @ TB
    cp = TB @ q
    gp = TB.T @ cp
    bp = Tu.T @ gp
    cc, gg, trp = cp @ cp, gp @ gp, np.trace(P)
    nsf = N * sf2
    F = ((((-0.5 * N * np.log(2 * np.pi) - np.log(np.diag(LB)).sum()) - 0.5 * N * np.log(s2)) - yy / (2 * s2))
         + cc / (2 * s2 * s2)) - (nsf - trp) / (2 * s2)
    H = np.eye(M) - Binv - np.outer(gp / s2, gp / s2)
    H2 = H - P / s2
    R = (H @ Tu).T / s2
    Guu2 = ((H2 @ Tu).T) @ Tu
    nl = len(dKuu)
    rows_uf = []
    for (X, y), (_, _, _, _, chunks, Ws) in zip(shards, stats):       # phase 2, per shard
        Sk = np.zeros(nl + 1)
        for (r0, rows, cpad, split, kstep), W in zip(chunks, Ws):
            Kc, dKc = ts.kernel_parts(c, X[r0: r0 + rows], Z)
            G = W @ R.T
            G = G + np.outer(y[r0: r0 + rows], bp / (s2 * s2))
            Sk = Sk + np.array([(G * a).sum() for a in dKc] + [(G * Kc).sum()])
        rows_uf.append(Sk)
    S_uf = rows_uf[0]
    for Sk in rows_uf[1:]:
        S_uf = S_uf + Sk
    if mutate == "suf_last_shard_twice":
        S_uf = S_uf + rows_uf[-1]
    S_uu = np.array([(Guu2 * a).sum() for a in dKuu] + [(Guu2 * Kuu0).sum()])
    S = S_uf + S_uu / 2
    g = list(-S[:nl])
    g.append(-(2 * S[nl] - nsf / s2))
    g.append(-(((np.sum(1 - np.diag(Binv)) - N) + (((yy - cc / s2) + (nsf - trp)) / s2)) - gg / (s2 * s2)))
    Wt = ts.kernel_parts(c, np.asarray(Xt, dtype=np.float64), Z)[0] @ Tu.T
    Vt = Wt @ TB.T
    return F, np.array(g), Vt @ cp / s2, ((sf2 - (Wt * Wt).sum(1)) + (Vt * Vt).sum(1)) + s2


_GZ = {}


def gz_case(name):
    """truth_sparse_z.case for a case of truth_sparse.CASES, whether or not truth_sparse_z lists it: the truth of gZ and its
    yardstick over the data as given and truth.permutations, once per process."""
    if name in tz.CASES:
        return tz.case(name)
    if name not in _GZ:
        X, y, Z, _, cov, chunk = ts.inputs(name)
        t = tz.truth_gz(X, y, Z, cov)
        E = [tz.error(tz.computed_gz(cov, X[idx], y[idx], Z), t) for idx in truth.permutations(len(y))]
        _GZ[name] = dict(X=X, y=y, Z=Z, cov=cov, chunk=chunk, tz=t, family=ts.CASES[name][0], noise=max(E), first=E[0],
                         rest=max(E[1:]), floor=truth.U4)
    return _GZ[name]


def hold(rep, c, F, grad, mean, var, tag=""):
    """truth_sparse.hold under F_SPARSE_SHARD[family]."""
    e = ts.errors(c["cov"], c["t"], c["tm"], c["tv"], F, grad, mean, var)
    for q in c["cov"].quantities:
        rep.add(tag + q, e[q], c["noise"][q], c["floor"][q], F_SPARSE_SHARD[c["family"]])


def hold_gz(rep, c, gz, tag=""):
    """truth_sparse_z.hold under F_SPARSE_SHARD_Z[family]."""
    rep.add(tag + "gZ", tz.error(gz, c["tz"]), c["noise"], c["floor"], F_SPARSE_SHARD_Z[c["family"]])
