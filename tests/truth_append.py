"""Appending observations to a factored model (include/cugp.h: cugp_append, cugp_append_plan) -- TEST INFRASTRUCTURE, a plain
module beside tests/truth.py and tests/accuracy.py.

Every case appends the LAST rows of an existing live case of truth.FAMILIES: the truth, the yardsticks and the floors are
the ones accuracy.live(oracle, family, name) caches for the whole case, and the bound is the bound a fresh handle on all
rows is held to,

    err <= F_APPEND[family] max(noise, floor)        (alpha and 64 rows of K^-1: F_SOLVE)

`standin_append` is the update in fp64 numpy / LAPACK in the order of the header's algebra: a fresh factor of the first n0
rows, then one bordering step per pass of `plan` (the passes of cugp_append_plan, restated).  F_APPEND is set from its
ratios (tests/test_truth_append_cpu.py, docs/ACCURACY.md), never from the GPU's errors.
"""
import numpy as np

import accuracy
import truth

LD = truth.LD
TILE = 128

# (family, live case, n0, chunks): the handle is created with n0 rows and the case's n as capacity, evaluated, and the
# chunks are appended in order.  What each exercises: docs/ACCURACY.md, "Appending observations".
CASES = (
    ("se", "n2", 1, (1,)),                          # smallest possible
    ("se", "n65", 63, (1, 1)),                      # across the 64-row build tile
    ("se", "n257_d3", 127, (2, 128)),               # a chunk that straddles 128 (2 passes), then a full unaligned tile (2 passes)
    ("se", "n300_d17", 128, (128, 44)),             # new rows open a fresh tile row; two feature chunks
    ("se", "n515_d33", 387, (128,)),                # three feature chunks, 4 -> 5 tile rows
    ("se", "n384_cond1e6", 300, (84,)),             # cond(K) ~ 1e6, one pass
    ("se", "n384_cond1e6", 300, (1,) * 84),         # the same, row by row
    ("se", "n1025_dense", 1000, (25,)),             # dense K, across the 1024 boundary
    ("se", "n1300_d6", 1290, (10,)),                # inverse built by the pipelined hand-over path
    ("ard", "n257_d3", 127, (2, 128)),
    ("ard", "n384_cond1e6", 300, (1,) * 84),
    ("matern52", "n300_d17", 128, (128, 44)),
    ("matern32", "n384_cond1e6", 300, (84,)),
    ("matern32", "n2", 1, (1,)),                    # below one build tile, the other families
    ("ard", "n2_d2", 1, (1,)),
    ("ard", "n65_d2", 63, (1, 1)),
    ("matern52", "n65", 63, (1, 1)),
    ("se", "n64", 1, (62, 1)),                      # from one row up to a full build tile
)

# family -> factor.  The larger of the family's own factor and truth.factor_rule of the largest stand-in ratio over the
# family's cases above (measured on the CPU: tests/test_truth_append_cpu.py prints the table, docs/ACCURACY.md keeps it).
F_APPEND = {"se": 16, "ard": truth.F_ARD, "matern32": truth.F_MATERN, "matern52": truth.F_MATERN}
F_SOLVE = truth.F_SOLVE


def case_id(case):
    family, name, n0, chunks = case
    return "%s-%s-%d+%s" % (family, name, n0, "+".join(str(k) for k in chunks) if len(chunks) <= 4
                            else "%dx%d" % (len(chunks), chunks[0]))


def plan(n, k):
    """The passes of an append of k rows to n: [a, b) pieces of [n, n + k), cut at the multiples of 128."""
    out, a = [], n
    while a < n + k:
        b = min((a // TILE + 1) * TILE, n + k)
        out.append((a, b))
        a = b
    return out


def standin_append(cov, X, y, Xt, n0, chunks, mutate=None, factors=False):
    """-> (ll, grad, mean, var, alpha, K^-1) of all n0 + sum(chunks) rows, by bordering in fp64; factors=True: -> (T, K^-1,
    log|K|) as the bordering leaves them (tests/truth_targets.py: targets set on a grown handle).
    mutate "drop_qtq": K^-1's leading block is not updated; "plus_q": Q = +C^-1 V -- the CPU suite shows that either
    leaves the bound by orders of magnitude."""
    import scipy.linalg as sl
    c = cov.fp64()
    X, y, Xt = np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64), np.asarray(Xt, dtype=np.float64)
    Kf, _ = c.train(X[:n0])
    L = np.linalg.cholesky(Kf + c.sn2 * np.eye(n0))
    T = sl.solve_triangular(L, np.eye(n0), lower=True)
    Ki = T.T @ T
    z = T @ y[:n0]
    a = T.T @ z
    logdet = 2 * np.log(np.diag(L)).sum()
    n = n0
    for k in chunks:
        for r0, r1 in plan(n, k):
            kk = r1 - r0
            Xb, yb = X[r0:r1], y[r0:r1]
            B = c.k(Xb, X[:r0])
            P = B @ T.T
            V = P @ T
            S = c.k(Xb, Xb) + c.sn2 * np.eye(kk) - P @ P.T
            Cf = np.linalg.cholesky(S)
            Ci = sl.solve_triangular(Cf, np.eye(kk), lower=True)
            Q = Ci @ V if mutate == "plus_q" else -(Ci @ V)
            zb = Ci @ (yb - P @ z)
            T = np.block([[T, np.zeros((r0, kk))], [Q, Ci]])
            lead = Ki if mutate == "drop_qtq" else Ki + Q.T @ Q
            Ki = np.block([[lead, Q.T @ Ci], [Ci.T @ Q, Ci.T @ Ci]])
            a = np.concatenate([a + Q.T @ zb, Ci.T @ zb])
            z = np.concatenate([z, zb])
            logdet = logdet + 2 * np.log(np.diag(Cf)).sum()
        n += k
    assert n == len(y)
    if factors:
        return T, Ki, logdet
    ll = -0.5 * (z @ z + logdet + n * truth.LL_CONST)
    Kf, terms = c.train(X)
    W = Ki - np.outer(a, a)
    g = np.array(terms(W) + (c.sn2 * np.trace(W),))
    Ks = c.k(Xt, X)
    Wt = Ks @ T.T
    return ll, g, Ks @ a, c.sf2 + c.sn2 - (Wt * Wt).sum(1), a, Ki


def ratios(c, ll, g, mean, var, alpha, Ki):
    """err / max(noise, floor) per quantity of the family and for alpha and K^-1, against the live case c."""
    e = truth.errors(c["cov"], ll, g, mean, var, c["t"].ll, c["t"].grad, c["tm"], c["tv"])
    es = truth.solve_errors(alpha, Ki, c["t"], c["rows"])
    return ({q: e[q] / max(c["noise"][q], c["floor"][q]) for q in c["cov"].quantities},
            {q: es[q] / max(c["solve"][q], truth.U4) for q in truth.SOLVE_QUANTITIES})


_STANDIN = {}


def standin_ratios(oracle, case):
    """The stand-in's ratios of a case of CASES, once per process."""
    if case not in _STANDIN:
        family, name, n0, chunks = case
        c = accuracy.live(oracle, family, name)
        _STANDIN[case] = ratios(c, *standin_append(c["cov"], c["X"], c["y"], c["Xt"], n0, chunks))
    return _STANDIN[case]


def hold(rep, c, family, ll, g, mean, var, alpha, Ki, tag=""):
    """Every quantity of a result at all rows into an accuracy.Report: F_APPEND of the family, F_SOLVE for alpha, K^-1."""
    e = truth.errors(c["cov"], ll, g, mean, var, c["t"].ll, c["t"].grad, c["tm"], c["tv"])
    rep.add_all(tag, e, c["noise"], c["floor"], F_APPEND[family])
    es = truth.solve_errors(alpha, Ki, c["t"], c["rows"])
    for q in truth.SOLVE_QUANTITIES:
        rep.add(tag + q, es[q], c["solve"][q], truth.U4, F_SOLVE)
