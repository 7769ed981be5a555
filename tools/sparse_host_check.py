"""The sparse-GP kernels of cugp_amd/csrc/sparse_device.h on the CPU, without a GPU, and those of sparse_targets_device.h
as the handle's own y runs them (p = 1): the rectangular gradient pass k_trace_cross<ARD, KIND> (one chunk with the
rank-one part; the square (Z, Z)), k_sparse_finalize_targets, and the small passes around the products
(k_sparse_gram_finish, k_sparse_form_b, k_sparse_wty_targets and its finish, k_sparse_yy_targets, k_sparse_h_targets,
k_sparse_transpose, k_sparse_predict_finish) -- the text kernels.hip includes -- in a lock-step host emulation
(tools/sparse_host_check.cpp) built with -fsanitize=address,undefined.  The MFMA product k_sparse_gram is not emulated.
The chunk is the LAST chunk of a case of tests/truth_sparse.py (ragged: 44, 1 or 128 rows of a 128-row pad; 257 rows of a
384-row pad at mpad 384, where k_sparse_gram_finish adds five partial tiles, k_sparse_h_targets and k_sparse_transpose run 6 x 6
blocks and k_sparse_predict_finish three test tiles; chunk_rows 0 is the library's 16384), its weight matrix random; rows
beyond the chunk and columns beyond M are NaN in every input a kernel must mask, and so are the strict upper 128-tiles of P
and B^-1: a missing mask shows as NaN, an access beyond a buffer as a sanitizer report.  Compared with numpy on the same
inputs:
  trace sums  per column, the blocks' partial sums added in longdouble against sum w o dK: 1e-13 of sum |w o dK|
  results     F and the nh gradient components against k_sparse_finalize_targets' formulas at p = 1 in numpy: 1e-13 of their scale
  small       P, B, q, y'y, H, H2, beta / s2^2, the transpose, mean and var: 4 ulp of the largest entry (sums: 1e-13)

    python tools/sparse_host_check.py          # builds into a temporary directory; about a minute
"""
import os
import struct
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import host_check  # noqa: E402  (also puts the repository root and tests/ on the path)

# (case of truth_sparse.CASES, rows of the chunk or None for the case's last chunk); three partial tiles in k_sparse_gram_finish
CASES = (("se_n300_m65", None), ("se_n128_m128", None), ("matern32_n300_m65", 1), ("ard_n300_m130_d17", None),
         ("matern52_ard_n257_m64", None), ("se_n1300_m200", 200))
# the same with the number of partial tiles k_sparse_gram_finish adds: mpad 384, five partials, 257 rows (three test tiles)
CASES_MPAD384 = (("se_n1300_m260_c0", 257, 5),)
ULP4 = 4 * 2.0 ** -52
CHUNK_DEFAULT = 16384                   # what chunk_rows = 0 stands for in the library (include/cugp.h: cugp_sparse_create)


def run(exe, tmp, name, rows, nscr=3):
    import truth_sparse as ts
    X, y, Z, _, cov, chunk = ts.inputs(name)
    c64 = cov.fp64()
    chunk = chunk if chunk > 0 else CHUNK_DEFAULT
    r0 = (len(y) - 1) // chunk * chunk
    Xr, yr = X[r0:], y[r0:]
    if rows is not None:
        Xr, yr = Xr[:rows], yr[:rows]
    nr, (m, d) = len(yr), Z.shape
    ld, rows_pad = (m + 127) // 128 * 128, (nr + 127) // 128 * 128
    ard, kind = hasattr(c64, "w"), getattr(c64, "kind", 0)
    nl = d if ard else 1
    rng = np.random.default_rng(nr + m)
    sf2, s2 = float(c64.sf2), float(c64.sn2)

    def padded(a, shape):
        out = np.full(shape, np.nan)
        out[tuple(slice(0, k) for k in a.shape)] = a
        return out
    G, bv, yv = rng.standard_normal((nr, m)), rng.standard_normal(m), padded(yr, (rows_pad,))
    Guu = rng.standard_normal((m, m))
    sym = [np.tril(a) + np.tril(a, -1).T for a in rng.standard_normal((2 + nscr, m, m))]
    lower128 = np.kron(np.tri(ld // 128), np.ones((128, 128))) > 0

    def lower(a, fill):                                            # full inside m, identity / zero padding, NaN above the lower 128-tiles
        out = np.eye(ld) * fill
        out[:m, :m] = a
        return np.where(lower128, out, np.nan)
    P, Binv = lower(sym[0], 0.0), lower(sym[1], 1.0)
    scr = [lower(a, 0.0) for a in sym[2:]]
    cp, gp, bp = (padded(rng.standard_normal(m), (ld,)) for _ in range(3))
    cp[m:] = 0.0                                                   # (c' is zero beyond m: LB's padding is the identity, q zero)
    logdet = rng.standard_normal(ld // 128)
    yy = float(yr @ yr)
    w = np.asarray(c64.w, dtype=np.float64) if ard else np.full(d, np.nan)
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("8i", nr, m, d, ld, rows_pad, kind, 1 if ard else 0, nscr))
        f.write(struct.pack("3d", 1.0 if ard else float(c64.l2), sf2, s2))
        for arr in (w, [float(len(y)), s2, float(np.log(s2)), yy], Xr, Z, padded(G, (rows_pad, ld)), yv, padded(bv, (ld,)),
                    padded(Guu, (ld, ld)), P, Binv, cp, gp, bp, logdet, np.stack(scr)):
            f.write(np.ascontiguousarray(arr, dtype=np.float64).tobytes())
    if not host_check.execute(exe, fin, fout, name, rows):
        return False
    out = np.fromfile(fout)
    nb_uf, nb_uu, nh, ll = (rows_pad // 64) * (ld // 64), (ld // 64) ** 2, nl + 2, ld * ld
    sizes = [(nl + 1) * (nb_uf + 3), (nl + 1) * nb_uu, 1 + nh, 1, ll, ll, ld, 1, ll, ll, ld, ll, nr, nr]
    parts = np.split(out, np.cumsum(sizes))
    assert len(parts[-1]) == 0, "output size"
    puf, puu, row, rowF, Pacc, Bm, q, yyk, H, H2, bsc, Gt, mean, var = parts[:-1]
    puf, puu = puf.reshape(nl + 1, nb_uf + 3), puu.reshape(nl + 1, nb_uu)
    Pacc, Bm = Pacc.reshape(ld, ld), Bm.reshape(ld, ld)
    offset_kept = bool(np.all(np.isnan(puf[:, :3])))
    # the restatement: sum w o dK per column, the rank-one part included
    LDT = np.longdouble
    Kc, dKc = ts.kernel_parts(c64, Xr, Z)
    Ku, dKu = ts.kernel_parts(c64, Z, Z)
    Wc = G + np.outer(yr, bv)
    want_uf = [(Wc * a).sum() for a in dKc] + [(Wc * Kc).sum()]
    want_uu = [(Guu * a).sum() for a in dKu] + [(Guu * Ku).sum()]
    mag_uf = [np.abs(Wc * a).sum() for a in dKc] + [np.abs(Wc * Kc).sum()]
    mag_uu = [np.abs(Guu * a).sum() for a in dKu] + [np.abs(Guu * Ku).sum()]
    s_uf, s_uu = puf[:, 3:].astype(LDT).sum(1), puu.astype(LDT).sum(1)
    et = max(max(float(abs(s - wv)) / mg for s, wv, mg in zip(s_uf, want_uf, mag_uf)),
             max(float(abs(s - wv)) / mg for s, wv, mg in zip(s_uu, want_uu, mag_uu)))
    # k_sparse_finalize_targets' formulas at p = 1 on the kernel's own sums
    N = float(len(y))
    S = np.asarray(s_uf + s_uu / 2, dtype=np.float64)
    Pd, Bd = np.diag(P)[:m], np.diag(Binv)[:m]
    trp, tb, cc, gg, lds = Pd.sum(), (1 - Bd).sum(), cp[:m] @ cp[:m], gp[:m] @ gp[:m], logdet.sum()
    F = -0.5 * N * np.log(2 * np.pi) - lds - 0.5 * N * np.log(s2) - yy / (2 * s2) + cc / (2 * s2 * s2) - (N * sf2 - trp) / (2 * s2)
    g = list(-S[:nl]) + [-(2 * S[nl] - N * sf2 / s2), -((tb - N) + ((yy - cc / s2) + (N * sf2 - trp)) / s2 - gg / (s2 * s2))]
    scale = np.abs([F] + g) + np.array([abs(lds) + yy / s2 + cc / s2 ** 2 + N] + [m_ for m_ in mag_uf[:nl]] + [2 * mag_uf[nl] + N, N + yy / s2 + gg / s2 ** 2])
    er = float(np.max(np.abs(row - np.array([F] + g)) / scale))
    same_f = row[0] == rowF[0]
    # the small passes
    def rel(got, want):
        return float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
    inner = np.zeros((ld, ld), dtype=bool)
    inner[:m, :m] = True
    Pfull, Bfull = sym[0], sym[1]
    acc = P
    for a in scr:
        acc = acc + a
    small = dict(
        gram=rel(Pacc[lower128], acc[lower128]) / ULP4,
        form_b=rel(Bm[lower128], (np.eye(ld) + P / s2)[lower128]) / ULP4,
        yy=abs(yyk[0] - yy) / yy / 1e-13,
        q=rel(q[:m], G.T @ yr) / 1e-13,
        H=rel(H.reshape(ld, ld)[:m, :m], np.eye(m) - Bfull - np.outer(gp[:m] / s2, gp[:m] / s2)) / ULP4,
        H2=rel(H2.reshape(ld, ld)[:m, :m], np.eye(m) - Bfull - np.outer(gp[:m] / s2, gp[:m] / s2) - Pfull / s2) / ULP4,
        bsc=rel(bsc[:m], bp[:m] / s2 / s2) / ULP4,
        transpose=rel(Gt.reshape(ld, ld)[:m, :m], Guu.T * 0.5) / ULP4,
        mean=rel(mean, G @ cp[:m] / s2) / 1e-13,
        var=rel(var, sf2 - (G * G).sum(1) + (G * G).sum(1) + s2) / 1e-13)
    zeros = not (H.reshape(ld, ld)[~inner].any() or H2.reshape(ld, ld)[~inner].any() or bsc[m:].any() or q[m:].any())
    finite = bool(np.all(np.isfinite(row)) and np.all(np.isfinite(puf[:, 3:])) and np.all(np.isfinite(puu))
                  and np.all(np.isfinite(mean)) and np.all(np.isfinite(var)) and np.all(np.isfinite(q[:m])))
    ok = et < 1e-13 and er < 1e-13 and same_f and offset_kept and zeros and finite and max(small.values()) <= 1.0
    print("sparse %-22s rows %-3d m %-3d ld %-3d nscr %d  against numpy: trace sums %.2e  results %.2e  small passes %.2f (of their "
          "tolerances; worst: %s)  padding zero %s  offset kept %s  %s"
          % (name, nr, m, ld, nscr, et, er, max(small.values()), max(small, key=small.get), zeros, offset_kept, "ok" if ok else "BAD"))
    return ok


if __name__ == "__main__":
    sys.exit(host_check.main("sparse_host_check", CASES + CASES_MPAD384, run))
