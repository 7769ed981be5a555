"""The leave-one-out kernels of cugp_amd/csrc/loo_device.h on the CPU, without a GPU: k_loo_point, k_loo_sum,
k_loo_mirror_scale, k_loo_bsum, k_trace_loo<ARD, KIND> and k_loo_finalize -- the text kernels.hip includes -- in a lock-step
host emulation (tools/loo_host_check.cpp) built with -fsanitize=address,undefined, in the order cugp_loo launches them; the
tile product k_loo_product is a plain loop there.  K^-1, alpha and y are padded as the library pads them, but with NaN
instead of the identity and zeros, and the strict upper triangle of K^-1 is NaN too: a missing mask or a read above the
diagonal shows as NaN, an access beyond a buffer as a sanitizer report.  Compared with an fp64 restatement in numpy
(tests/truth_loo.py: point_quantities, fused) on the same K^-1 and alpha:
  per point   mu, var, logp, a, s: 4 ulp of the largest entry; b = K^-1 a: 1e-13 of the largest entry;
              L_LOO against the sum of the kernel's own logp in longdouble: 4 ulp of |L_LOO|
  gradient    1e-13 of max|g|
  padding     rows >= n of all five per-point rows and of b, and rows and columns >= n of B: exact zeros

    python tools/loo_host_check.py          # builds into a temporary directory; about a minute
"""
import os
import struct
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import host_check  # noqa: E402  (also puts the repository root and tests/ on the path)

# (family, case, rows taken from the case or None for all): npad 128, 256 and 384; n = 65, 128, 129, 257 and 300; and below
# and at one 64-row build tile: n = 1, 2, 63, 64
CASES = (("se", "n65", None), ("se", "n128", None), ("se", "n257_d3", 129), ("matern52", "n300_d17", None),
         ("ard", "n257_d3", None), ("matern32_ard", "n65_d2", None), ("matern32_ard", "n257_d3", None),
         ("se", "n65", 1), ("se", "n65", 2), ("se", "n65", 63), ("se", "n65", 64),
         ("ard", "n257_d3", 2), ("ard", "n257_d3", 63), ("matern52", "n300_d17", 2), ("matern52", "n300_d17", 63))
ULP4 = 4 * 2.0 ** -52


def run(exe, tmp, family, name, rows):
    import scipy.linalg as sl
    import truth
    import truth_loo as tl
    X, y, _, cov = tl.inputs(family, name)
    if rows is not None:
        X, y = np.ascontiguousarray(X[:rows]), np.ascontiguousarray(y[:rows])
    c64 = cov.fp64()
    n, d = X.shape
    npad = (n + 127) // 128 * 128
    ard = hasattr(c64, "w")
    kind = getattr(c64, "kind", 0)
    Kf, terms = c64.train(X)
    T = sl.solve_triangular(np.linalg.cholesky(Kf + c64.sn2 * np.eye(n)), np.eye(n), lower=True)
    Ki = T.T @ T
    Ki = np.tril(Ki) + np.tril(Ki, -1).T                      # what the library holds: the lower triangle, mirrored on reading
    a = T.T @ (T @ y)
    Kp = np.full((npad, npad), np.nan)
    Kp[:n, :n] = np.where(np.tri(n, dtype=bool), Ki, np.nan)
    ap, yp = np.full(npad, np.nan), np.full(npad, np.nan)
    ap[:n], yp[:n] = a, y
    w = np.asarray(c64.w, dtype=np.float64) if ard else np.full(d, np.nan)
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("5i", n, d, npad, kind, 1 if ard else 0))
        f.write(struct.pack("3d", 1.0 if ard else float(c64.l2), float(c64.sf2), float(c64.sn2)))
        for arr in (w, X, Kp, ap, yp):
            f.write(np.ascontiguousarray(arr, dtype=np.float64).tobytes())
    if not host_check.execute(exe, fin, fout, family, name, rows):
        return False
    out = np.fromfile(fout)
    nh = (d if ard else 1) + 2
    pt = out[: 5 * npad].reshape(5, npad)
    b = out[5 * npad: 6 * npad]
    row = out[6 * npad: 6 * npad + 1 + nh]
    B = out[6 * npad + 1 + nh:].reshape(npad, npad)
    # the restatement
    kap = np.diag(Ki).copy()
    mu, var, logp = tl.point_quantities(kap, a, y, truth.LL_CONST)
    av = a / kap
    sv = np.sqrt((1 + a * av) / kap)
    # (n = 1: mu = y - alpha / kappa is 0 up to the rounding of the quotient: its scale is then |y|, that of the difference)
    point = max(float(np.max(np.abs(got[:n] - want)) / (np.max(np.abs(want)) or np.max(np.abs(y))))
                for got, want in zip(pt, (mu, var, logp, av, sv))) / ULP4
    eb = float(np.max(np.abs(b[:n] - Ki @ av)) / np.max(np.abs(Ki @ av)))
    lsum = np.sum(pt[2, :n].astype(np.longdouble))
    el = float(abs(np.longdouble(row[0]) - lsum) / abs(lsum)) / ULP4
    W = tl.fused(Ki, a)
    g = np.array(terms(W) + (c64.sn2 * np.trace(W),))
    eg = float(np.max(np.abs(row[1:] - g)) / np.max(np.abs(g)))
    zeros = not pt[:, n:].any() and not b[n:].any() and not B[n:].any() and not B[:, n:].any()
    eB = float(np.max(np.abs(B[:n, :n] - Ki * sv[None, :])) / np.max(np.abs(Ki * sv[None, :]))) / ULP4
    ok = (point <= 1.0 and el <= 1.0 and eb < 1e-13 and eg < 1e-13 and eB <= 1.0 and zeros and bool(np.all(np.isfinite(out))))
    print("loo %-12s %-9s n %-3d npad %-3d  against numpy, same formulation: per point %.2f  L_LOO %.2f  B %.2f (of 4 ulp)  "
          "b %.2e  gradient %.2e  padding zero %s  %s" % (family, name, n, npad, point, el, eB, eb, eg, zeros, "ok" if ok else "BAD"))
    return ok


if __name__ == "__main__":
    sys.exit(host_check.main("loo_host_check", CASES, run))
