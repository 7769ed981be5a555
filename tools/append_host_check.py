"""k_append_border and k_append_kinv on the CPU, without a GPU: the kernels' own text (cugp_amd/csrc/append_device.h,
the header kernels.hip includes) in a lock-step host emulation (tools/append_host_check.cpp) built with
-fsanitize=address,undefined.  One bordering pass per case: the state of a handle that holds its inverse quantities for r0
rows is laid out as the library lays it out (identity padding; NaN where the kernels must not read: the rows of P and V
beyond k, the strict upper tiles of T and the strict lower tiles of U), P, V, C and C^-1 come from numpy, and what the
kernels leave is compared with the header's algebra in fp64 numpy -- equal up to the order of summation.  A missing mask
shows as NaN, an access beyond a buffer as a sanitizer report.

    python tools/append_host_check.py          # builds into a temporary directory; about a minute
"""
import os
import struct
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import host_check  # noqa: E402  (also puts the repository root and tests/ on the path)

# (r0, k): one row to one row; a pass that ends inside the first 64 rows; old rows in the pass's own tile; a fresh tile row;
# a full tile; r0 no multiple of 32; the last row of the capacity
CASES = ((1, 1), (5, 40), (127, 1), (128, 128), (130, 126), (200, 56), (300, 84), (255, 1))


def run(exe, tmp, r0, k):
    import scipy.linalg as sl
    import truth
    from conftest import synth
    n = r0 + k
    npad = (n + 127) // 128 * 128
    X, y = synth(n, d=3, seed=n, scale=3.0)
    c = truth.SE([0.9, 0.2, -1.0], np.float64)
    K = c.train(X)[0] + c.sn2 * np.eye(n)
    L = np.linalg.cholesky(K[:r0, :r0])
    T = sl.solve_triangular(L, np.eye(r0), lower=True)
    Ki, z = T.T @ T, T @ y[:r0]
    a = T.T @ z
    P = K[r0:, :r0] @ T.T
    V = P @ T
    Cf = np.linalg.cholesky(K[r0:, r0:] - P @ P.T)
    Ci = sl.solve_triangular(Cf, np.eye(k), lower=True)

    def padded(M, fill_upper=None, fill_lower=None):
        out = np.eye(npad)
        out[:M.shape[0], :M.shape[1]] = M
        t = np.arange(npad) // 128
        if fill_upper is not None:
            out[t[:, None] < t[None, :]] = fill_upper
        if fill_lower is not None:
            out[t[:, None] > t[None, :]] = fill_lower
        return out
    strip = lambda M: np.concatenate([np.pad(M, ((0, 0), (0, npad - r0))), np.full((128 - k, npad), np.nan)])
    tile = lambda M: padded(M)[:128, :128] if npad == 128 else np.block([[M, np.zeros((k, 128 - k))], [np.zeros((128 - k, k)), np.eye(128 - k)]])
    vec = lambda v: np.pad(v, (0, npad - len(v)))
    logdet = np.zeros(npad // 128)
    for t in range(npad // 128):
        logdet[t] = np.log(np.diag(L)[t * 128: min(r0, (t + 1) * 128)]).sum()
    yv = vec(y)                                                  # (the new targets are already in dy)
    bufs = [strip(P), strip(V), tile(Cf), tile(Ci), np.array([np.log(np.diag(Cf)).sum()]),
            padded(L), padded(T, fill_upper=np.nan), padded(T.T, fill_lower=np.nan), padded(Ki), yv, vec(z), vec(a), logdet]
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("3i", r0, k, npad))
        for arr in bufs:
            f.write(np.ascontiguousarray(arr, dtype=np.float64).tobytes())
    if not host_check.execute(exe, fin, fout, r0, k):
        return False
    out = np.fromfile(fout)
    nn = npad * npad
    A, Tn, Un, Kn = (out[i * nn: (i + 1) * nn].reshape(npad, npad) for i in range(4))
    y2, z2, a2 = (out[4 * nn + i * npad: 4 * nn + (i + 1) * npad] for i in range(3))
    ld2 = out[4 * nn + 3 * npad: 4 * nn + 3 * npad + npad // 128]
    Qt = out[4 * nn + 3 * npad + npad // 128:].reshape(npad, 128)
    # the header's algebra
    Q = -(Ci @ V)
    zb = Ci @ (y[r0:] - P @ z)
    Tw = np.block([[T, np.zeros((r0, k))], [Q, Ci]])
    Kw = np.block([[Ki + Q.T @ Q, Q.T @ Ci], [Ci.T @ Q, Ci.T @ Ci]])
    Lw = np.block([[L, np.zeros((r0, k))], [P, Cf]])
    aw, zw = np.concatenate([a + Q.T @ zb, Ci.T @ zb]), np.concatenate([z, zb])
    rel = lambda got, want: float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
    t = np.arange(npad) // 128
    low = (t[:, None] >= t[None, :])                             # the tiles T is read in; U: the transpose
    low64 = (np.arange(npad)[:, None] // 64 >= np.arange(npad)[None, :] // 64) | (t[:, None] == t[None, :])   # + diagonal 128-tiles complete
    e = dict(L=rel(np.tril(A), padded(Lw)), T=rel(np.where(low, Tn, 0.0), padded(Tw)), U=rel(np.where(low.T, Un, 0.0), padded(Tw.T)),
             Kinv=rel(np.where(low64, Kn, 0.0), np.where(low64, padded(Kw), 0.0)), z=rel(z2, vec(zw)), alpha=rel(a2, vec(aw)),
             logdet=abs(ld2.sum() - np.log(np.diag(Lw)).sum()) / abs(np.log(np.diag(Lw)).sum() or 1.0),
             Qt=rel(Qt[:(r0 + 63) // 64 * 64, :], np.pad(Q.T, ((0, (r0 + 63) // 64 * 64 - r0), (0, 128 - k)))))
    ok = all(v < 1e-12 for v in e.values()) and np.array_equal(y2, yv)
    ok = ok and bool(np.all(np.isfinite(np.where(low, Tn, 0.0)))) and bool(np.all(np.isfinite(np.where(low64, Kn, 0.0))))
    print("r0 %-4d k %-4d npad %-4d  against numpy, same algebra: " % (r0, k, npad)
          + "  ".join("%s %.1e" % kv for kv in e.items()) + ("  ok" if ok else "  BAD"))
    return ok


if __name__ == "__main__":
    sys.exit(host_check.main("append_host_check", CASES, run))
