"""Replays of the preconditioner's arithmetic on the CPU, shared by test_gpu_iter_precond.py and the table of
docs/ACCURACY.md: the pivoted-Cholesky recurrence along a given pivot order in any number format, and M^-1 V =
(V - Q Q'V) / sn2 with Q = L Lc^-T, Lc Lc' = sn2 I + L'L."""
import numpy as np

import truth

LD, U = truth.LD, truth.U
F_PCHOL, F_PCAPPLY = 4, 4            # docs/ACCURACY.md, "Pivoted-Cholesky preconditioner": truth.factor_rule of the stand-ins


def replay(Kf, piv, reverse=False):
    """-> (L [n, r], the residual diagonal in front of every step with -inf at the rows already taken) in Kf's format;
    the sum over the earlier columns by numpy's product, or (reverse: the stand-in) term by term from the last column down."""
    n, r = len(Kf), len(piv)
    L, dres, taken, hist = np.zeros((n, r), Kf.dtype), np.diag(Kf).copy(), np.zeros(n, bool), []
    for k, p in enumerate(piv):
        hist.append(np.where(taken, -np.inf, dres))
        if reverse:
            s = np.zeros(n, Kf.dtype)
            for m in range(k - 1, -1, -1):
                s = s + L[:, m] * L[p, m]
        else:
            s = L[:, :k] @ L[p, :k]
        root = np.sqrt(dres[p])
        col = (Kf[:, p] - s) / root
        col[taken] = 0
        col[p] = root
        L[:, k], dres, taken[p] = col, dres - col * col, True
    return L, hist


def greedy_pivots(Kf, r):
    """The pivot order of the recurrence in Kf's format: the largest residual, the lowest row on ties."""
    piv = []
    for _ in range(r):
        piv.append(int(np.argmax(replay(Kf, piv + [0])[1][-1])))
    return piv


def apply(L, sn2, V, order=None):
    """M^-1 V' for V [t, n] in L's format by the formula the device uses; order: the rows of L permuted (the stand-in)."""
    idx = np.arange(len(L)) if order is None else order
    Lo, Vo = L[idx], V[:, idx].T
    C = Lo.T @ Lo + sn2 * np.eye(L.shape[1], dtype=L.dtype)
    Lc = truth.cholesky(C) if L.dtype == LD else np.linalg.cholesky(C)
    Q = Lo @ (truth.tri_inverse(Lc).T if L.dtype == LD else np.linalg.inv(Lc).T)
    out = np.empty_like(Vo)
    out[idx] = (Vo - Q @ (Q.T @ Vo)) / sn2
    return out.T


def apply_truth(L, sn2, V):
    """(L L' + sn2 I)^-1 V' in longdouble, by a Cholesky factorisation of the n x n matrix itself."""
    Ll = L.astype(LD)
    M = Ll @ Ll.T + LD(sn2) * np.eye(len(L), dtype=LD)
    return V.astype(LD) @ truth.gram_lower(truth.tri_inverse(truth.cholesky(M))).T
