"""The kernel of cugp_amd/csrc/sparse_predict_device.h on the CPU, without a GPU: k_sparse_predict_diff -- the text kernels.hip
includes -- in a host emulation (tools/sparse_joint_host_check.cpp) built with -fsanitize=address,undefined.  The pass
forms D = Wt - T over the whole 128-row tiles of a ragged number of test rows and a = beta' / s2 over m of mpad entries;
Wt, T and D carry 64 spare rows -- NaN in the inputs, a marker in the output -- and beta' is a heap block of exactly m
doubles: a read or write beyond the rows shows as NaN or a lost marker, a read beyond m as a sanitizer report.  Compared:
  bits     D and a against the program's plain double loop: identical; a alone (D null) and D alone (a null) identical to
           the joint launch; the spare rows of D untouched; a exactly 0.0 in [m, mpad)
  numpy    D and a against Wt - T and beta' / s2 in numpy: identical (one rounding each, nothing is summed)

    python tools/sparse_joint_host_check.py          # builds into a temporary directory; under a minute
"""
import os
import struct
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import host_check  # noqa: E402  (also puts the repository root and tests/ on the path)

# (test rows of the pass, inducing inputs): a ragged nt in two tiles against mpad 128 and 384; one row; no padding at all
CASES = ((200, 65), (129, 260), (1, 16), (128, 128))
MARKER = -12345.0


def run(exe, tmp, nt, m):
    rows, ld = (nt + 127) // 128 * 128, (m + 127) // 128 * 128
    rng = np.random.default_rng(1000 * nt + m)
    s2 = float(np.exp(2 * -1.3))

    def spare(a):
        out = np.full((rows + 64, ld), np.nan)
        out[:rows] = a
        return out
    # as the library holds them: exact zeros beyond row nt and column m, which the pass reads like any other entry
    Wt, T = np.zeros((rows, ld)), np.zeros((rows, ld))
    Wt[:nt, :m], T[:nt, :m] = rng.standard_normal((nt, m)), rng.standard_normal((nt, m))
    bp = rng.standard_normal(m)
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("3i", rows, ld, m))
        f.write(struct.pack("1d", s2))
        for arr in (spare(Wt), spare(T), bp):
            f.write(np.ascontiguousarray(arr, dtype=np.float64).tobytes())
    if not host_check.execute(exe, fin, fout, nt, m):
        return False
    out = np.fromfile(fout)
    n_all = (rows + 64) * ld
    assert len(out) == 3 * n_all + 3 * ld, "output size"
    D, a, a1 = out[:n_all].reshape(rows + 64, ld), out[n_all: n_all + ld], out[n_all + ld: n_all + 2 * ld]
    D1 = out[n_all + 2 * ld: 2 * n_all + 2 * ld].reshape(rows + 64, ld)
    Dref, aref = out[2 * n_all + 2 * ld: 3 * n_all + 2 * ld].reshape(rows + 64, ld), out[3 * n_all + 2 * ld:]

    def bits(x, y):
        return np.array_equal(np.ascontiguousarray(x).view(np.uint64), np.ascontiguousarray(y).view(np.uint64))
    same = bits(D, Dref) and bits(a, aref)
    alone = bits(a1, a) and bits(D1, D)
    spare_ok = bool(np.all(D[rows:] == MARKER))
    finite = bool(np.all(np.isfinite(D[:rows])) and np.all(np.isfinite(a)))
    zeros = not np.any(a[m:]) and not np.any(D[nt:rows]) and not np.any(D[:rows, m:])
    want_a = np.zeros(ld)
    want_a[:m] = bp / s2
    numpy_same = bits(D[:rows], Wt - T) and bits(a, want_a)
    ok = same and alone and spare_ok and finite and zeros and numpy_same
    print("sparse-joint nt %-4d rows %-4d m %-3d mpad %-3d  plain loop: %s  a alone / D alone: %s  spare rows %s  padding %s  "
          "numpy: %s  finite %s  %s" % (nt, rows, m, ld, "same bits" if same else "DIFFERENT", "same bits" if alone else "DIFFERENT",
                                        "untouched" if spare_ok else "WRITTEN", "zero" if zeros else "NONZERO",
                                        "same bits" if numpy_same else "DIFFERENT", finite, "ok" if ok else "BAD"))
    return ok


if __name__ == "__main__":
    sys.exit(host_check.main("sparse_joint_host_check", CASES, run))
