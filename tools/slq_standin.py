"""The fp64 numpy stand-in behind F_SLQ and F_QUAD of tests/test_gpu_iter_loglik.py (docs/ACCURACY.md, "Lanczos quadrature"):
the same recurrences and quadrature as cugp_iter_loglik in another order of summation -- a pivoted Cholesky factor of Kf,
probes z = L g1 + sn g2, (preconditioned) conjugate gradients per probe that stop at |r| <= tol |z|, the Jacobi matrix of the
coefficients, LAPACK's tridiagonal eigensolver -- on the test's very cases, against the test's truth and yardsticks.  No GPU.

    python tools/slq_standin.py          # prints every ratio and the two largest: the factors are 4 x those
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import scipy.linalg as sl  # noqa: E402
import test_gpu_iter as ti  # noqa: E402
import test_gpu_iter_loglik as tl  # noqa: E402
import truth  # noqa: E402
from cugp_amd import gp  # noqa: E402


def pivoted_cholesky(Kf, r):
    n = len(Kf)
    L, d = np.zeros((n, r)), np.diag(Kf).copy()
    for k in range(r):
        p = int(np.argmax(d))
        L[:, k] = (Kf[:, p] - L[:, :k] @ L[p, :k]) / np.sqrt(d[p])
        d = d - L[:, k] ** 2
        d[p] = -np.inf
    return L


def quadrature(K, z, Minv, tol, max_iter):
    """-> (w sum tau^2 log lambda, x) of one probe: CG on K (Minv: the preconditioner's inverse, or None)"""
    if not z.any():
        return 0.0, z
    x, r = np.zeros_like(z), z.copy()
    zz = r if Minv is None else Minv @ r
    p, rz, w, bb = zz.copy(), r @ zz, r @ zz, z @ z
    a, b = [], []
    for _ in range(max_iter):
        q = K @ p
        a.append(rz / (p @ q))
        x, r = x + a[-1] * p, r - a[-1] * q
        if r @ r <= tol * tol * bb:
            break
        zz = r if Minv is None else Minv @ r
        rz, old = r @ zz, rz
        b.append(rz / old)
        p = zz + b[-1] * p
    a, b = np.array(a), np.array(b[:len(a) - 1])
    dg = 1 / a
    dg[1:] += b / a[:-1]
    lam, V = sl.eigh_tridiagonal(dg, np.sqrt(b) / a[:-1], lapack_driver="stev") if len(a) > 1 else (dg, np.ones((1, 1)))
    return w * (V[0] ** 2 @ np.log(lam)), x


def main():
    worst = {"ll": 0.0, "quad": 0.0}
    for family in tl.KERNELS:
        for n, r in tl.CASES + [(200, "quad0"), (200, "quad8")]:
            X, y, _, cov, K, _ = ti.case(family, n, tl.D)
            K64, sn2 = K.astype(np.float64), float(cov.sn2)
            per_probe = isinstance(r, str)
            r = int(r[4:]) if per_probe else r
            L = pivoted_cholesky(K64 - sn2 * np.eye(n), r)
            Minv = np.linalg.inv(L @ L.T + sn2 * np.eye(n)) if r else None
            if per_probe:
                rng = np.random.default_rng(5)
                G2, G1 = gp.rademacher(rng, 9, n), (gp.rademacher(rng, 9, r) if r else None)
            else:
                G2, G1 = tl.complete_probes(n, r)
            Z = G2 if not r else G1 @ L.T + np.sqrt(sn2) * G2
            quad = np.array([quadrature(K64, z, Minv, tl.TOL, 4 * n + 8)[0] for z in Z])
            if per_probe:
                want, yard = tl.quad_truth(family, n, L, Z)
                ratio, key = float(np.max(np.abs(quad - want) / yard)), "quad"
            else:
                alpha = quadrature(K64, y, Minv, tl.TOL, 4 * n + 8)[1]
                ldm = np.linalg.slogdet(L @ L.T + sn2 * np.eye(n))[1] if r else 0.0
                ll = -0.5 * (y @ alpha + ldm + quad.mean() + n * truth.LL_CONST)
                want, yard = tl.ll_yardstick(family, n)
                ratio, key = float(abs(truth.LD(ll) - want) / yard), "ll"
            worst[key] = max(worst[key], ratio)
            print("%-9s n %-3d r %d %-4s stand-in error / yardstick %.3g" % (family, n, r, key, ratio))
    print("largest ratios: ll %.3g, quad %.3g  ->  F_SLQ = 4 x %.3g, F_QUAD = 4 x %.3g" % (worst["ll"], worst["quad"], worst["ll"], worst["quad"]))


if __name__ == "__main__":
    main()
