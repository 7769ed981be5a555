"""The fp64 numpy stand-in behind F_VC, F_VCK and VC_FLOOR of the variance cache (tests/test_gpu_iter_varcache.py, kernels.h;
docs/ACCURACY.md, "Variance cache"): the algorithm of cugp_iter_varcache_build in another order of summation -- block Arnoldi
from the same start block, classical Gram-Schmidt twice against all earlier columns, CholQR twice inside the block with the
device's floor rule, H from the coefficients (diagonal blocks averaged, the rest mirrored from above) = L L', R = Q L^-T, var = prior - |R'k*|^2 -- on the test's very
cases, against the test's truths and yardstick.  No GPU.

    python tools/varcache_standin.py     # prints every ratio, the largest per factor, and the floor's two sides
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import scipy.linalg as sl  # noqa: E402
import test_gpu_iter_varcache as tv  # noqa: E402

U, VC_FLOOR = 2.0 ** -53, 5.0
RATIOS = {"kept": np.inf, "ended": 0.0}          # pivot / (norm before projection): smallest kept, largest ended


def cholqr(W, c0, nrm0):
    """One round: -> (W T^-1 over the live columns, T, live); nrm0 None: the second round (ends at a non-positive pivot only)"""
    cw = W.shape[1]
    G, T, live = W.T @ W, np.zeros((cw, cw)), cw
    for c in range(cw):
        p = G[c, c] - T[:c, c] @ T[:c, c]
        if nrm0 is not None and nrm0[c] > 0:
            key = "kept" if p > VC_FLOOR * (c0 + c + 1) * U * nrm0[c] else "ended"
            RATIOS[key] = (min if key == "kept" else max)(RATIOS[key], p / nrm0[c])
        if not p > (VC_FLOOR * (c0 + c + 1) * U * nrm0[c] if nrm0 is not None else 0.0):
            live = c
            break
        T[c, c] = np.sqrt(p)
        T[c, c + 1:] = (G[c, c + 1:] - T[:c, c] @ T[:c, c + 1:]) / T[c, c]
    T = T[:live, :live]
    return (sl.solve_triangular(T, W[:, :live].T, trans="T", lower=False).T if live else W[:, :0]), T, live


def build(K, B, rank):
    """-> (Q [n, got], R [n, got], H [got, got] as factored)"""
    n, bw = K.shape[0], B.shape[0]
    Q, H, ended = np.zeros((n, 0)), np.zeros((rank, rank)), False

    def orthonormalise(W, nrm0):
        c0, cw = Q.shape[1], min(bw, rank - Q.shape[1])
        W1, T1, l1 = cholqr(W[:, :cw], c0, nrm0)
        W2, T2, l2 = cholqr(W1, c0, None)
        return W2, l1 < cw or l2 < l1

    P, ended = orthonormalise(B.T.copy(), (B * B).sum(1))
    Q = np.hstack([Q, P])
    while P.shape[1]:
        W = K @ P
        nrm0, c0p = (W * W).sum(0), Q.shape[1] - P.shape[1]
        C1 = Q.T @ W
        H[:Q.shape[1], c0p:Q.shape[1]] = C1
        if ended or Q.shape[1] >= rank:
            break
        W = W - Q @ C1
        C2 = Q.T @ W
        W = W - Q @ C2
        H[:Q.shape[1], c0p:Q.shape[1]] += C2
        Pn, ended = orthonormalise(W, nrm0)
        Q, P = np.hstack([Q, Pn]), Pn
    got = Q.shape[1]
    blk = np.arange(got) // bw                     # the device's k_vc_hsym: diagonal blocks averaged, the rest mirrored from above
    up = blk[:, None] < blk[None, :]
    H = H[:got, :got]
    H = np.where(up, H, np.where(up.T, H.T, (H + H.T) * 0.5))
    L = np.linalg.cholesky(H)
    return Q, sl.solve_triangular(L, Q.T, lower=True).T, H


def cached_var(family, n, rank, nt, B=None):
    X, _, _, cov, t, _, B0 = tv.case(family, n)
    _, R, _ = build(t.K.astype(np.float64), B0 if B is None else B, rank)
    Ks = cov.k(tv.points(family, n, nt).astype(tv.LD), X.astype(tv.LD)).astype(np.float64)
    return float(t.sf2) + float(t.sn2) - ((Ks @ R) ** 2).sum(1), R.shape[1]


def main():
    worst = {"full": 0.0, "partial": 0.0}
    for family in tv.SEVEN:
        for n in (48, 40):
            for nt in (5, 70):
                tvar, bv = tv.var_bound(family, n, nt)
                var, got = cached_var(family, n, n, nt)
                ratio = float(np.max(np.abs(var.astype(tv.LD) - tvar) / bv))
                worst["full"] = max(worst["full"], ratio)
                print("%-13s n %-3d rank %-3d got %-3d nt %-2d stand-in error / yardstick %.3g" % (family, n, n, got, nt, ratio))
    for family in ("se", "rq_ard"):
        for n in (200, 257):
            cond = np.linalg.cond(tv.case(family, n)[4].K.astype(np.float64))
            for rank in (32, 64):
                _, bv = tv.var_bound(family, n, 70)
                var, got = cached_var(family, n, rank, 70)
                ratio = float(np.max(np.abs(var.astype(tv.LD) - tv.galerkin_var(family, n, rank, 70)) / bv))
                worst["partial"] = max(worst["partial"], ratio)
                print("%-13s n %-3d rank %-3d got %-3d cond %.3g stand-in error / yardstick %.3g" % (family, n, rank, got, cond, ratio))
    B = tv.case("se", 200)[6].copy()
    B[1] = B[0]
    print("a repeated start column: rank", cached_var("se", 200, 64, 5, B)[1])
    print("largest ratios: full %.3g, partial %.3g  ->  F_VC = 4 x %.3g, F_VCK = 4 x %.3g" % (worst["full"], worst["partial"], worst["full"], worst["partial"]))
    print("floor: smallest pivot / norm of a kept column %.3g, largest of an ended one %.3g (floor at k = 512: %.3g)"
          % (RATIOS["kept"], RATIOS["ended"], VC_FLOOR * 512 * U))


if __name__ == "__main__":
    main()
