"""The multi-target sparse-GP kernels of cugp_amd/csrc/sparse_targets_device.h on the CPU, without a GPU: k_sparse_wty_targets
and its finish, k_sparse_yy_targets, k_sparse_h_targets, k_sparse_weights_targets, k_sparse_scale_targets and
k_sparse_finalize_targets -- the text kernels.hip includes -- in a lock-step host emulation
(tools/sparse_targets_host_check.cpp) built with -fsanitize=address,undefined as a stand-alone program.  Random inputs of a
shape (p targets, m inducing points padded to ld, nr rows of a rows_pad chunk); NaN wherever a kernel must mask -- rows
beyond the chunk's count, columns beyond m, the strict upper 128-tiles of P and B^-1 --, and the targets' buffers hold
exactly p rows, so a read of a target beyond p in the last group is a sanitizer report.  Every result is compared BIT FOR BIT
with plain numpy loops in the kernels' stated order (numpy's elementwise products and sums round once each, as the kernels
do under fp contract(off)): per target the slab shares (wpart), y_t'y_t (wyy) and H (h) are the sums the handle's own y
has, which runs these kernels with p = 1 (tools/sparse_host_check.py holds that case against its own numpy forms).

    python tools/sparse_targets_host_check.py          # builds into a temporary directory; about a minute
"""
import os
import struct
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import host_check  # noqa: E402  (also puts the repository root and tests/ on the path)

# (p, m, nr, rows_pad, nl): one target; three on identity padding with a ragged chunk; a second group of one target over two
# slabs and two M tiles; a third group and a second staging round of one target at mpad 256; ARD-like nl = 3
CASES = ((1, 65, 44, 128, 1), (3, 65, 44, 128, 1), (9, 130, 200, 256, 1), (17, 200, 129, 256, 3), (3, 128, 128, 128, 1))
LOG2PI = 1.8378770664093453


def tree(a):
    """wave_sum: lane l takes l + o for o = 32, 16, .. 1; -> lane 0."""
    a = a.copy()
    o = 32
    while o:
        a[..., :o] = a[..., :o] + a[..., o: 2 * o]
        o //= 2
    return a[..., 0]


def strided(x, width):
    """thread v of `width` adds the entries v, v + width, ... ascending from 0.0 -> [width]."""
    pad = np.zeros(-(-len(x) // width) * width)
    pad[: len(x)] = x
    s = np.zeros(width)
    for row in pad.reshape(-1, width):
        s = s + row
    return s


def block_sum(x):
    """one workgroup: 256 strided sums, the lanes by wave_sum, the four waves as (w0 + w1) + (w2 + w3)."""
    w = tree(strided(x, 256).reshape(4, 64))
    return (w[0] + w[1]) + (w[2] + w[3])


def same(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def run(exe, tmp, p, m, nr, rows_pad, nl):
    ld = (m + 127) // 128 * 128
    rng = np.random.default_rng(1000 * p + m + nr)
    N, sf2, s2 = 1234.0, 1.7, 0.31
    log_s2 = float(np.log(s2))
    slabs, nb_uf, nb_uu, nh, p64 = rows_pad // 128, (rows_pad // 64) * (ld // 64), (ld // 64) ** 2, nl + 2, (p + 63) // 64 * 64

    def padded(a, shape, fill):
        out = np.full(shape, fill)
        out[tuple(slice(0, k) for k in a.shape)] = a
        return out
    W = padded(rng.standard_normal((nr, m)), (rows_pad, ld), 0.0)
    Y = rng.standard_normal((p, nr))
    Yz, Yn = padded(Y, (p, rows_pad), 0.0), padded(Y, (p, rows_pad), np.nan)
    lower128 = np.kron(np.tri(ld // 128), np.ones((128, 128))) > 0
    sym = [np.tril(a) + np.tril(a, -1).T for a in rng.standard_normal((2, m, m))]

    def lower(a, fill):
        out = np.eye(ld) * fill
        out[:m, :m] = a
        return np.where(lower128, out, np.nan)
    P, Binv = lower(sym[0], 0.0), lower(sym[1], 1.0)
    Cp, Gm, Bt = (padded(rng.standard_normal((p, m)), (p, ld), np.nan) for _ in range(3))
    G0 = padded(rng.standard_normal((nr, m)), (rows_pad, ld), np.nan)
    logdet = rng.standard_normal(ld // 128)
    puf, puu = rng.standard_normal((nl + 1, nb_uf)), rng.standard_normal((nl + 1, nb_uu))
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("7i", p, m, ld, nr, rows_pad, nl, nb_uf))
        for arr in ([N, sf2, s2, log_s2], W, Yz, Yn, P, Binv, Cp, Gm, Bt, G0, logdet, puf, puu):
            f.write(np.ascontiguousarray(arr, dtype=np.float64).tobytes())
    if not host_check.execute(exe, fin, fout, p, m, nr):
        return False
    out = np.fromfile(fout)
    sizes = [p * slabs * ld, p * ld, p * ld, p, ld * ld, ld * ld, p * ld, rows_pad * ld, p64 * ld, 1 + nh + p, 1 + nh + p]
    parts = np.split(out, np.cumsum(sizes))
    assert len(parts[-1]) == 0, "output size"
    part, Q1, Q2, yy, H, H2, Bs, G, Cs, row, rowF = parts[:-1]
    bad = []

    def hold(what, got, want):
        if not same(got, want):
            bad.append(what)
    # ---- the restatement, in the kernels' order
    wpart = np.zeros((p, slabs, ld))
    for t in range(p):
        for sl in range(slabs):
            acc = np.zeros((4, ld))
            for j in range(32):
                for g in range(4):
                    r = sl * 128 + g + 4 * j
                    acc[g] = acc[g] + W[r] * Yz[t, r]
            wpart[t, sl] = (acc[0] + acc[1]) + (acc[2] + acc[3])
    hold("part", part.reshape(p, slabs, ld), wpart)
    q1 = np.zeros((p, ld))
    for sl in range(slabs):
        q1 = q1 + wpart[:, sl]
    q2 = q1.copy()
    for sl in range(slabs):
        q2 = q2 + wpart[:, sl]
    hold("Q first", Q1.reshape(p, ld), q1)
    hold("Q accumulated", Q2.reshape(p, ld), q2)
    wyy = np.array([block_sum(Y[t] * Y[t]) for t in range(p)])
    hold("yy", yy, wyy)
    Bf, Pf = sym[1], sym[0]
    gam = Gm[:, :m] / s2
    h = float(p) * (np.eye(m) - Bf)
    for t in range(p):
        h = h - np.outer(gam[t], gam[t])
    wH, wH2 = np.zeros((ld, ld)), np.zeros((ld, ld))
    wH[:m, :m], wH2[:m, :m] = h, h - float(p) * (Pf / s2)
    hold("H", H.reshape(ld, ld), wH)
    hold("H2", H2.reshape(ld, ld), wH2)
    wBs = np.zeros((p, ld))
    wBs[:, :m] = (Bt[:, :m] / s2) / s2
    hold("Bs", Bs.reshape(p, ld), wBs)
    wG = G0.copy()
    g = G0[:nr, :m].copy()
    for t in range(p):
        g = g + np.outer(Y[t], wBs[t, :m])
    wG[:nr, :m] = g
    hold("G", G.reshape(rows_pad, ld), wG)                        # (NaN beyond nr and m: left as they were, bit for bit)
    wCs = np.zeros((p64, ld))
    wCs[:p, :m] = Cp[:, :m] / s2
    hold("Cs", Cs.reshape(p64, ld), wCs)
    inner = np.zeros((ld, ld), dtype=bool)
    inner[:m, :m] = True
    ok_pad = not (H.reshape(ld, ld)[~inner].any() or H2.reshape(ld, ld)[~inner].any() or Bs.reshape(p, ld)[:, m:].any())
    # the final sums
    col = []
    for c in range(nl + 1):
        a, b = tree(strided(puf[c], 64)), tree(strided(puu[c], 64))
        col.append(a + b / 2.0)
    trp, tb, lds = block_sum(np.diag(P)[:m]), block_sum(1.0 - np.diag(Binv)[:m]), block_sum(logdet)
    nsf = N * sf2
    each, F, syy, scc, sgg = [], 0.0, 0.0, 0.0, 0.0
    for t in range(p):
        cct, ggt = block_sum(Cp[t, :m] * Cp[t, :m]), block_sum(Gm[t, :m] * Gm[t, :m])
        Ft = ((((-0.5 * N * LOG2PI - lds) - 0.5 * N * log_s2) - wyy[t] / (2.0 * s2)) + cct / (2.0 * s2 * s2)) - (nsf - trp) / (2.0 * s2)
        each.append(Ft)
        F, syy, scc, sgg = (Ft, wyy[t], cct, ggt) if t == 0 else (F + Ft, syy + wyy[t], scc + cct, sgg + ggt)
    pd = float(p)
    gr = [-s for s in col[:nl]]
    gr.append(-(2.0 * col[nl] - pd * nsf / s2))
    gr.append(-(((pd * tb - pd * N) + (((syy - scc / s2) + pd * (nsf - trp)) / s2)) - sgg / (s2 * s2)))
    hold("row", row, np.array([F] + gr + each))
    hold("row without the gradient", rowF[[0] + list(range(1 + nh, 1 + nh + p))], np.array([F] + each))
    if not np.all(np.isnan(rowF[1: 1 + nh])):
        bad.append("gradient slots written without the partials")
    finite = bool(np.all(np.isfinite(row)) and np.all(np.isfinite(Q2)) and np.all(np.isfinite(H)) and np.all(np.isfinite(H2))
                  and np.all(np.isfinite(Bs)) and np.all(np.isfinite(G.reshape(rows_pad, ld)[:nr, :m])))
    ok = not bad and ok_pad and finite
    print("sparse targets p %-2d m %-3d ld %-3d rows %-3d of %-3d nl %d  bit for bit against numpy in the stated order: %s  "
          "padding %s  finite %s  %s" % (p, m, ld, nr, rows_pad, nl, "all" if not bad else "NOT " + ", ".join(bad), ok_pad, finite,
                                         "ok" if ok else "BAD"))
    return ok


if __name__ == "__main__":
    sys.exit(host_check.main("sparse_targets_host_check", CASES, run))
