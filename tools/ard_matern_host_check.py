"""The ARD Matern instantiations of trace_ard_body (k_trace<true, KIND>) and k_predict_grad<true, KIND> on the CPU, without a GPU: the kernels' own text (cugp_amd/csrc/cov_device.h,
the header kernels.hip includes) in a lock-step host emulation (tools/ard_matern_host_check.cpp) built with
-fsanitize=address,undefined, on cases of truth.ARD_CASES.  K^-1, alpha and V are padded as the library pads them, but with
NaN instead of zeros: a missing mask shows as NaN, an access beyond a buffer as a sanitizer report.  The results are
compared with the same formulation in fp64 numpy (tests/truth_ard_matern.py) -- equal up to the order of summation:
  trace         the blocks' partials added per column: S_c / 2 against g_c = 1/2 sum W o H o u_c^2, column d against
                sum W o K, column d + 1 against tr W; tolerance 1e-12 of the sum of the terms' absolute values
  predict-grad  dmean, dvar after k_predict_grad_finish against truth_ard_matern.gradients; 1e-13 of the largest entry

    python tools/ard_matern_host_check.py          # builds into a temporary directory; a few minutes
"""
import os
import struct
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import host_check  # noqa: E402  (also puts the repository root and tests/ on the path)

# (kernel, case, kind, nt or None for the case's 64 points, with the variance's sums)
CASES = (("trace", "n65_d2", 1, None, 1), ("trace", "n65_d2", 2, None, 1), ("trace", "n257_d3_shift", 2, None, 1),
         ("trace", "n300_d17", 1, None, 1), ("trace", "n515_d33", 2, None, 1),
         ("grad", "n65_d2", 1, None, 1), ("grad", "n65_d2", 2, None, 0), ("grad", "n257_d3_shift", 2, None, 1),
         ("grad", "n300_d17", 1, None, 1), ("grad", "n515_d33", 2, None, 1), ("grad", "n257_d3", 2, 129, 1),
         ("trace", "n2_d2", 1, None, 1), ("trace", "n63_d2", 2, None, 1),                  # below one 64-row build tile
         ("grad", "n2_d2", 2, None, 1), ("grad", "n63_d2", 1, None, 1))


def run(exe, tmp, kernel, name, kind, nt, want_var):
    import scipy.linalg as sl
    import truth
    import truth_ard_matern as tam
    X, y, Xt, cov = tam.inputs(name, kind) if nt is None else truth.wide_inputs(name, nt, tam.FAMILY[kind])
    c64 = cov.fp64()
    n, d = X.shape
    nt = len(Xt)
    npad, cpad = (n + 127) // 128 * 128, (nt + 127) // 128 * 128
    Kf, terms = c64.train(X)
    T = sl.solve_triangular(np.linalg.cholesky(Kf + c64.sn2 * np.eye(n)), np.eye(n), lower=True)
    Ki = T.T @ T
    Ki = (Ki + Ki.T) / 2
    a = T.T @ (T @ y)
    ap = np.full(npad, np.nan)
    ap[:n] = a
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("8i", 0 if kernel == "trace" else 1, n, d, npad, nt, cpad, kind, want_var))
        f.write(struct.pack("2d", float(c64.sf2), float(c64.sn2)))
        arrays = [c64.w, X]
        if kernel == "trace":
            Kp = np.full((npad, npad), np.nan)
            Kp[:n, :n] = Ki
            arrays += [Kp, ap]
        else:
            V = (c64.k(Xt, X) @ T.T) @ T
            Vp = np.full((cpad, npad), np.nan)
            Vp[:nt, :n] = V
            arrays += [Xt, Vp, ap]
        for arr in arrays:
            f.write(np.ascontiguousarray(arr, dtype=np.float64).tobytes())
    if not host_check.execute(exe, fin, fout, kernel, name, kind, nt):
        return False
    out = np.fromfile(fout)
    if kernel == "trace":
        nb = (npad // 64) * (npad // 64 + 1) // 2
        col = out.reshape(d + 2, nb).sum(1)
        W = Ki - np.outer(a, a)
        ref = np.array(terms(W))                                       # g_0 .. g_{d-1}, sum W o Kf
        got = np.concatenate([col[:d] / 2, [col[d] - c64.sn2 * col[d + 1], col[d + 1]]])
        want = np.concatenate([ref, [np.trace(W)]])
        scale = np.array(c64.train(X)[1](np.abs(W)) + (np.abs(np.diag(W)).sum(),))      # the terms' absolute values
        scale[d] += c64.sn2 * scale[d + 1]
        err = float(np.max(np.abs(got - want) / scale))
        ok = err < 1e-12 and bool(np.all(np.isfinite(out)))
        print("trace  %-14s kind %d   against numpy, same formulation: largest error / sum |terms| %.2e  %s"
              % (name, kind, err, "ok" if ok else "BAD"))
        return ok
    dm = out[: nt * d].reshape(nt, d)
    rm, rv = tam.gradients(c64, Xt, X, a, V)
    em = float(np.max(np.abs(dm - rm)) / np.max(np.abs(rm)))
    ev = float(np.max(np.abs(out[nt * d:].reshape(nt, d) - rv)) / np.max(np.abs(rv))) if want_var else 0.0
    ok = em < 1e-13 and ev < 1e-13 and bool(np.all(np.isfinite(out)))
    print("grad   %-14s kind %d nt %-4d dvar %d   against numpy, same formulation: dmean %.2e  dvar %.2e  %s"
          % (name, kind, nt, want_var, em, ev, "ok" if ok else "BAD"))
    return ok


if __name__ == "__main__":
    sys.exit(host_check.main("ard_matern_host_check", CASES, run))
