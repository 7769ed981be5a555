"""The rational quadratic instantiations of the ARD gradient pass (k_trace<true, RQ>, plain and over m targets) and of
k_predict_grad<true, RQ> on the CPU, without a GPU: the kernels' own text (cugp_amd/csrc/cov_device.h, the header kernels.hip
includes) in a lock-step host emulation (tools/rq_host_check.cpp) built as a stand-alone program with
-fsanitize=address,undefined.  K^-1, alpha, the targets' alphas and V are padded as the library pads them, but with NaN
instead of zeros: a missing mask shows as NaN, an access beyond a buffer as a sanitizer report.  The program itself
compares every output BIT FOR BIT with a plain loop in the same order of summation (exit code 4 on a mismatch; the loop calls
the header's rq_entry, so that comparison covers summation order, masking and indexing); this script checks the arithmetic: the columns' sums against fp64 numpy (tests/truth_rq.py) at
1e-12 of the sum of the terms' absolute values, the input gradients at 1e-13 of their largest entry.

    python tools/rq_host_check.py          # builds into a temporary directory; about a minute
"""
import os
import struct
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import host_check  # noqa: E402  (also puts the repository root and tests/ on the path)

# (kernel, n, d, theta_alpha, m targets or nt test points, with the variance's sums): npad <= 384, ragged n
CASES = (("trace", 65, 3, 0.4, 1, 1), ("trace", 257, 3, -0.7, 1, 1), ("trace", 65, 17, 2.0, 1, 1), ("trace", 257, 17, 12.0, 1, 1),
         ("targets", 65, 3, 0.4, 3, 1), ("targets", 257, 17, 2.0, 17, 1), ("targets", 65, 17, -0.7, 3, 1),
         ("grad", 65, 3, 0.4, 70, 1), ("grad", 257, 3, -0.7, 64, 0), ("grad", 65, 17, 2.0, 129, 1), ("grad", 257, 17, 12.0, 70, 1))


def run(exe, tmp, kernel, n, d, theta_alpha, mt, want_var):
    import truth_ard_matern as tam
    import truth_rq as trq
    rng = np.random.default_rng(1000 * n + d)
    X = rng.uniform(-2.0, 2.0, (n, d))
    hp = list(np.linspace(0.4, 1.1, d) + 0.5 * np.log(d)) + [theta_alpha, 0.3, -0.8]
    c64 = trq.RQ(hp).fp64()
    alpha, h2a = trq.host_shape(theta_alpha)
    w = np.exp(-np.asarray(hp[:d]))
    npad = (n + 127) // 128 * 128
    B = rng.standard_normal((n, n)) / np.sqrt(n)
    Ki = B @ B.T + np.eye(n)
    Ki = (Ki + Ki.T) / 2
    a = rng.standard_normal(n)
    ap = np.full(npad, np.nan)
    ap[:n] = a
    Kp = np.full((npad, npad), np.nan)
    Kp[:n, :n] = Ki
    nt = mt if kernel == "grad" else 0
    m = mt if kernel == "targets" else 1
    cpad = (nt + 127) // 128 * 128
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("8i", {"trace": 0, "targets": 1, "grad": 2}[kernel], n, d, npad, nt, cpad, m, want_var))
        f.write(struct.pack("2d", float(c64.sf2), float(c64.sn2)))
        arrays = [w, [alpha, h2a], X]
        if kernel == "trace":
            arrays += [Kp, ap]
        elif kernel == "targets":
            A = rng.standard_normal((m, n))
            Ap = np.full((m, npad), np.nan)
            Ap[:, :n] = A
            arrays += [Kp, Ap]
        else:
            Xt = rng.uniform(-2.0, 2.0, (nt, d))
            Xt[0] += 50.0                                              # a far point
            Xt[nt // 2] = X[n // 2]                                    # a training row
            V = rng.standard_normal((nt, n))
            Vp = np.full((cpad, npad), np.nan)
            Vp[:nt, :n] = V
            arrays += [Xt, Vp, ap]
        for arr in arrays:
            f.write(np.ascontiguousarray(arr, dtype=np.float64).tobytes())
    if not host_check.execute(exe, fin, fout, kernel, n, d, theta_alpha, mt):
        return False
    out = np.fromfile(fout)
    if kernel in ("trace", "targets"):
        nb = (npad // 64) * (npad // 64 + 1) // 2
        col = out.reshape(d + 3, nb).sum(1)
        W = Ki - np.outer(a, a) if kernel == "trace" else m * Ki - A.T @ A
        terms = c64.train(X)[1]
        ref = np.array(terms(W))                                       # g_0 .. g_{d-1}, g_alpha, sum W o Kf
        got = np.concatenate([col[:d + 1] / 2, [col[d + 1] - c64.sn2 * col[d + 2], col[d + 2]]])
        want = np.concatenate([ref, [np.trace(W)]])
        Wa = np.abs(W)
        Kf, H, Aa = c64._parts(tam.wsqdist64(X, X, w))
        scale = np.array([float((Wa * H * ((X[:, c][:, None] - X[:, c][None, :]) * w[c]) ** 2).sum()) / 2 for c in range(d)]
                         + [float((Wa * np.abs(Aa)).sum()) / 2, float((Wa * Kf).sum()) + c64.sn2 * float(np.abs(np.diag(W)).sum()),
                            float(np.abs(np.diag(W)).sum())])
        err = float(np.max(np.abs(got - want) / scale))
        ok = err < 1e-12 and bool(np.all(np.isfinite(out)))
        print("%-7s n %-3d d %-2d theta_alpha %-4g m %-2d  bits equal the plain loop; against numpy: largest error / sum |terms| %.2e  %s"
              % (kernel, n, d, theta_alpha, m, err, "ok" if ok else "BAD"))
        return ok
    dm = out[: nt * d].reshape(nt, d)
    rm, rv = tam.gradients(c64, Xt, X, a, V)
    em = float(np.max(np.abs(dm - rm)) / np.max(np.abs(rm)))
    ev = float(np.max(np.abs(out[nt * d:].reshape(nt, d) - rv)) / np.max(np.abs(rv))) if want_var else 0.0
    ok = em < 1e-13 and ev < 1e-13 and bool(np.all(np.isfinite(out)))
    print("grad    n %-3d d %-2d theta_alpha %-4g nt %-3d dvar %d  bits equal the plain loop; against numpy: dmean %.2e  dvar %.2e  %s"
          % (n, d, theta_alpha, nt, want_var, em, ev, "ok" if ok else "BAD"))
    return ok


if __name__ == "__main__":
    sys.exit(host_check.main("rq_host_check", CASES, run))
