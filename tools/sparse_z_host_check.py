"""The kernels of cugp_amd/csrc/sparse_z_device.h on the CPU, without a GPU: k_trace_cross_z<ARD, KIND> over one chunk with
the rank-one part (the first pass) and over the square (Z, Z, 2 G_uu) (the last pass), k_trace_cross_z_finish behind each --
the text kernels.hip includes -- in a lock-step host emulation (tools/sparse_z_host_check.cpp) built with
-fsanitize=address,undefined.  The chunk is the LAST chunk of a case of tests/truth_sparse_z.py (ragged: 44, 128, 1 or 200 rows
of a padded block; 800 rows in ranges of 5, 5 and 4 tiles and 1300 rows in ranges of 5, 5, 5, 5 and 2, as chunk_rows 0 -- the
library's 16384 -- gives them), its weight matrices random; rows beyond the chunk and columns beyond M are NaN in every G
entry, label and rank-one weight the kernel must mask, and the points are heap blocks of exactly nr x d and m x d doubles: a
missing mask shows as NaN, an access beyond a buffer as a sanitizer report.  Compared:
  bits     the partial blocks of both passes, the running sums after each and the result against the program's plain double
           loop in the same summation order: identical; the pinned copy identical to the device result
  numpy    the result against the formula in numpy on the same inputs: 1e-13 of max_j,c s_c sum |w H (x - z)|

    python tools/sparse_z_host_check.py          # builds into a temporary directory; about a minute
"""
import os
import struct
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import host_check  # noqa: E402  (also puts the repository root and tests/ on the path)

# (case of truth_sparse_z.CASES, rows of the chunk or None for the case's last chunk, ranges of the chunk's pass, of the square's)
CASES = (("se_n300_m65_d3", None, 1, 1), ("se_n256_m128_d3", None, 2, 2), ("matern32_n300_m65", 1, 1, 2),
         ("matern52_n300_m65_d3", None, 2, 1), ("ard_n300_m130_d17", None, 1, 2), ("matern52_ard_n257_m64", None, 2, 1),
         ("se_n1300_m200", 200, 2, 4))
# the same at the default chunk (chunk_rows 0): 14 row tiles in ranges of 5, 5 and 4; 22 in 5, 5, 5, 5 and 2, six column tiles
CASES_DEFAULT_CHUNK = (("se_n800_m65_d3_c0", None, 3, 1), ("se_n1300_m260_c0", None, 5, 3))
CHUNK_DEFAULT = 16384                   # what chunk_rows = 0 stands for in the library (include/cugp.h: cugp_sparse_create)


def run(exe, tmp, name, rows, ranges_uf, ranges_uu):
    import truth_sparse_z as tz
    X, y, Z, cov, chunk = tz.inputs(name)
    c64 = cov.fp64()
    chunk = chunk if chunk > 0 else CHUNK_DEFAULT
    r0 = (len(y) - 1) // chunk * chunk
    Xr, yr = X[r0:], y[r0:]
    if rows is not None:
        Xr, yr = Xr[:rows], yr[:rows]
    nr, (m, d) = len(yr), Z.shape
    ld, rows_pad = (m + 127) // 128 * 128, (nr + 127) // 128 * 128
    ard, kind = hasattr(c64, "w"), getattr(c64, "kind", 0)
    rng = np.random.default_rng(nr + m + d)

    def padded(a, shape):
        out = np.full(shape, np.nan)
        out[tuple(slice(0, k) for k in a.shape)] = a
        return out
    G, bv, Guu = rng.standard_normal((nr, m)), rng.standard_normal(m), rng.standard_normal((m, m))
    w = np.asarray(c64.w, dtype=np.float64) if ard else np.full(d, np.nan)
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("9i", nr, m, d, ld, rows_pad, kind, 1 if ard else 0, ranges_uf, ranges_uu))
        f.write(struct.pack("3d", 1.0 if ard else float(c64.l2), float(c64.sf2), float(c64.sn2)))
        for arr in (w, Xr, Z, padded(G, (rows_pad, ld)), padded(yr, (rows_pad,)), padded(bv, (ld,)), padded(Guu, (ld, ld))):
            f.write(np.ascontiguousarray(arr, dtype=np.float64).tobytes())
    if not host_check.execute(exe, fin, fout, name, rows):
        return False
    out = np.fromfile(fout)
    md = m * d

    def shape(rows_, ranges):
        tiles = rows_ // 64
        per = -(-tiles // ranges)
        return -(-tiles // per)
    n_uf, n_uu = shape(rows_pad, ranges_uf), shape(ld, ranges_uu)
    half = (n_uf + n_uu + 3) * md
    assert len(out) == 2 * half + md, "output size"
    got, ref, hout = out[:half], out[half: 2 * half], out[2 * half:]
    same = np.array_equal(got.view(np.uint64), ref.view(np.uint64))
    pinned = np.array_equal(got[-md:].view(np.uint64), hout.view(np.uint64))
    finite = bool(np.all(np.isfinite(got)))
    # the formula in numpy: differences before products
    Hf, sc = tz.h_factor(c64, Z, Xr)
    Hu = tz.h_factor(c64, Z, Z)[0]
    Wf, Wu = (G + np.outer(yr, bv)).T * Hf, Guu.T * Hu
    want = -(tz.weighted_differences(Wf, Xr, Z) + tz.weighted_differences(Wu, Z, Z)) * sc[None, :]
    mag = np.zeros(Z.shape)
    for c in range(d):
        mag[:, c] = (np.abs(Wf) * np.abs(Xr[:, c][None, :] - Z[:, c][:, None])).sum(1) \
            + (np.abs(Wu) * np.abs(Z[:, c][None, :] - Z[:, c][:, None])).sum(1)
    en = float(np.max(np.abs(got[-md:].reshape(m, d) - want)) / np.max(mag * sc[None, :]))
    ok = same and pinned and finite and en < 1e-13 and (n_uf, n_uu) == (ranges_uf, ranges_uu)
    print("sparse-z %-22s rows %-4d m %-3d d %-2d ranges %d / %d  plain loop: %s  pinned copy: %s  against numpy %.2e  finite %s  %s"
          % (name, nr, m, d, n_uf, n_uu, "same bits" if same else "DIFFERENT", "same bits" if pinned else "DIFFERENT", en,
             finite, "ok" if ok else "BAD"))
    return ok


if __name__ == "__main__":
    sys.exit(host_check.main("sparse_z_host_check", CASES + CASES_DEFAULT_CHUNK, run))
