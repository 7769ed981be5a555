"""The k_predict_grad family on the CPU, without a GPU: the kernels' own text (cugp_amd/csrc/cov_device.h, the header kernels.hip includes) in a
lock-step host emulation (tools/predict_grad_host_check.cpp) built with -fsanitize=address,undefined, on cases of
tests/truth_predict_grad.py.  Ks, V and alpha are padded as the library pads them, but with NaN instead of zeros: a
missing mask shows as NaN, an access beyond a buffer as a sanitizer report.  The results are compared with the same
formulation in fp64 numpy (tests/truth_predict_grad.py: gradients) -- equal up to the order of summation.

    python tools/predict_grad_host_check.py          # builds into a temporary directory; about a minute
"""
import os
import struct
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import host_check  # noqa: E402  (also puts the repository root and tests/ on the path)

CASES = (("se", "n2", None, 1), ("se", "n64", None, 1), ("se", "n65", None, 1), ("se", "n65", None, 0),
         ("matern32", "n65", None, 1), ("ard", "n257_d3_shift", None, 1), ("se", "n300_d17", None, 1),
         ("matern52", "n300_d17", None, 1), ("se", "n515_d33", None, 1), ("ard", "n257_d3", 200, 1),
         ("matern52", "n300_d17", 129, 1),
         ("matern32", "n2", None, 1), ("ard", "n2_d2", None, 1), ("se", "n63", 1, 1))      # below one build tile; one test point


def run(exe, tmp, family, name, nt, want_var):
    import scipy.linalg as sl
    import truth
    import truth_predict_grad as tpg
    X, y, Xt, cov = truth.family_inputs(family, name) if nt in (None, 1) else truth.wide_inputs(name, nt, family)
    if nt == 1:
        Xt = np.ascontiguousarray(Xt[:1])                     # (one test point: the first of the case's 64)
    c64 = cov.fp64()
    n, d = X.shape
    nt = len(Xt)
    npad, cpad = (n + 127) // 128 * 128, (nt + 127) // 128 * 128
    Kf, _ = c64.train(X)
    T = sl.solve_triangular(np.linalg.cholesky(Kf + c64.sn2 * np.eye(n)), np.eye(n), lower=True)
    a = T.T @ (T @ y)
    Ks = c64.k(Xt, X)
    V = (Ks @ T.T) @ T
    Kp, Vp, ap = np.full((cpad, npad), np.nan), np.full((cpad, npad), np.nan), np.full(npad, np.nan)
    Kp[:nt, :n], Vp[:nt, :n], ap[:n] = Ks, V, a
    ard = family == "ard"
    kind = {"se": 0, "ard": 0, "matern32": 1, "matern52": 2}[family]
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("8i", n, d, npad, nt, cpad, kind, want_var, int(ard)))
        f.write(struct.pack("2d", 1.0 if ard else float(c64.l2), float(c64.sf2)))
        for arr in (X, Xt, Kp, Vp, ap, c64.w if ard else np.ones(d)):
            f.write(np.ascontiguousarray(arr, dtype=np.float64).tobytes())
    if not host_check.execute(exe, fin, fout, family, name, nt):
        return False
    out = np.fromfile(fout)
    dm = out[: nt * d].reshape(nt, d)
    rm, rv = tpg.gradients(c64, Xt, X, a, V)
    em = float(np.max(np.abs(dm - rm)) / np.max(np.abs(rm)))
    ev = float(np.max(np.abs(out[nt * d:].reshape(nt, d) - rv)) / np.max(np.abs(rv))) if want_var else 0.0
    ok = em < 1e-13 and ev < 1e-13 and bool(np.all(np.isfinite(out)))
    print("%-9s %-14s nt %-4d dvar %d   against numpy, same formulation: dmean %.2e  dvar %.2e  %s"
          % (family, name, nt, want_var, em, ev, "ok" if ok else "BAD"))
    return ok


if __name__ == "__main__":
    sys.exit(host_check.main("predict_grad_host_check", CASES, run))
