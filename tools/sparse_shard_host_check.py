"""The kernels of cugp_amd/csrc/sparse_shard_device.h on the CPU, without a GPU: k_sparse_shard_reduce, k_sparse_shard_sums
and k_sparse_finalize_sharded -- the text kernels.hip includes -- in a lock-step host emulation
(tools/sparse_shard_host_check.cpp) built with -fsanitize=address,undefined as a stand-alone program.  A case is a world of
W ranks with `per` slots each holding K shards (shard k in slot k // W of rank k % W: interleaved owners, and empty slots
where per * W > K), the library's slot [P mpad^2 | q mpad | y'y | n] behind a 16-double header, a shard's trace partials of
nb_uf blocks and nl + 1 columns, and the final sums over m inducing points padded to mpad.  NaN wherever a kernel must not
read -- the headers, the empty slots, the slot outside the reduced range, P and B^-1 off their diagonals, every vector
beyond m -- and heap blocks of exactly the library's sizes: a missing mask shows as NaN, an access beyond a buffer as a
sanitizer report.  Every result is compared BIT FOR BIT with plain loops in the stated order: the shards k = 0 .. K - 1 with
the first term copied; lane-strided ascending, then wave_sum; k_sparse_finalize_targets' expressions at p = 1.

    python tools/sparse_shard_host_check.py          # builds into a temporary directory; under a minute
"""
import os
import struct
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import host_check  # noqa: E402  (also puts the repository root and tests/ on the path)
from sparse_targets_host_check import block_sum, same, strided, tree  # noqa: E402

HDR = 16                                # SHARD_HDR of cugp_amd/csrc/handle.h
LOG2PI = 1.8378770664093453
# (K, W, per, mpad, the reduced range "P" | "tail" (q, y'y, n), nb_uf, nl, m, gradient)
CASES = ((5, 2, 3, 128, "P", 1, 1, 65, 1), (5, 2, 3, 256, "tail", 63, 1, 200, 1), (3, 1, 5, 128, "tail", 64, 3, 128, 1),
         (3, 1, 5, 256, "P", 65, 17, 130, 1), (1, 1, 1, 128, "P", 200, 1, 65, 0), (4, 2, 2, 128, "tail", 200, 4, 1, 1),
         (8, 8, 1, 128, "tail", 65, 1, 100, 1), (9, 8, 2, 128, "P", 64, 2, 128, 0))


def slot_of(k, W, per):
    """(rank, slot) of shard k: bcm.gather_row_index's convention."""
    return k % W, k // W


def run(exe, tmp, K, W, per, mpad, what, nb_uf, nl, m, grad):
    rng = np.random.default_rng(K * 1000 + W * 100 + per * 10 + nl + nb_uf)
    slot = mpad * mpad + mpad + 2
    off, ln = (0, mpad * mpad) if what == "P" else (mpad * mpad, mpad + 2)
    rstride = HDR + per * slot
    gathered = np.full((W, rstride), np.nan)
    shards = []
    for k in range(K):
        r, s = slot_of(k, W, per)
        v = rng.standard_normal(ln)
        gathered[r, HDR + s * slot + off: HDR + s * slot + off + ln] = v
        shards.append(v)
    ld, nt, nb_uu = mpad, mpad // 128, (mpad // 64) ** 2
    part_uf, part_uu = rng.standard_normal((nl + 1, nb_uf)), rng.standard_normal((nl + 1, nb_uu))
    P, Binv = np.full((ld, ld), np.nan), np.full((ld, ld), np.nan)
    dp, db = rng.uniform(1, 2, m), rng.uniform(0.1, 0.9, m)
    P[np.arange(m), np.arange(m)], Binv[np.arange(m), np.arange(m)] = dp, db
    Cp, Gm = np.full(ld, np.nan), np.full(ld, np.nan)
    Cp[:m], Gm[:m] = rng.standard_normal(m), rng.standard_normal(m)
    logdet, yyn = rng.standard_normal(nt), np.array([rng.uniform(100, 200), float(rng.integers(1, 2000))])
    sf2, s2 = float(rng.uniform(0.5, 2)), float(rng.uniform(0.05, 0.5))
    log_s2 = float(np.log(s2))
    suf = rng.standard_normal(nl + 1)
    grid = min((ln + 255) // 256, 7)                                 # (a short grid: the stride loop runs more than once)
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("15i", K, W, per, HDR, slot, off, ln, grid, nb_uf, nl, nb_uu, m, ld, nt, grad))
        for arr in (gathered, part_uf, P, Binv, Cp, Gm, logdet, yyn, np.array([sf2, s2, log_s2]), suf, part_uu):
            f.write(np.ascontiguousarray(arr, dtype=np.float64).tobytes())
    if not host_check.execute(exe, fin, fout, K, W, per, mpad, what):
        return False
    out = np.fromfile(fout)
    assert len(out) == ln + (nl + 1) + 2 * (nl + 4), "output size"
    red, sums, res, hres = out[:ln], out[ln: ln + nl + 1], out[ln + nl + 1: ln + 2 * nl + 5], out[ln + 2 * nl + 5:]
    # the plain loops
    want = shards[0].copy()
    for v in shards[1:]:
        want = want + v
    want_sums = np.array([tree(strided(part_uf[c], 64)) for c in range(nl + 1)])
    nh = nl + 2
    wres = np.full(nl + 4, np.nan)
    trp, tb, ldt = block_sum(dp), block_sum(1.0 - db), block_sum(logdet)
    cc, gg = block_sum(Cp[:m] * Cp[:m]), block_sum(Gm[:m] * Gm[:m])
    yy, n = float(yyn[0]), float(yyn[1])
    nsf = n * sf2
    F = ((((-0.5 * n * LOG2PI - ldt) - 0.5 * n * log_s2) - yy / (2.0 * s2)) + cc / (2.0 * s2 * s2)) - (nsf - trp) / (2.0 * s2)
    wres[0] = wres[1 + nh] = F
    if grad:
        s = np.array([suf[c] + tree(strided(part_uu[c], 64)) / 2.0 for c in range(nl + 1)])
        wres[1: 1 + nl] = -s[:nl]
        wres[1 + nl] = -(2.0 * s[nl] - nsf / s2)
        wres[2 + nl] = -(((tb - n) + (((yy - cc / s2) + (nsf - trp)) / s2)) - gg / (s2 * s2))
    checks = dict(reduce=same(red, want), sums=same(sums, want_sums), final=same(res, wres), pinned=same(hres, res),
                  finite=bool(np.all(np.isfinite(red)) and np.all(np.isfinite(sums)) and np.isfinite(res[0])))
    ok = all(checks.values())
    print("sparse-shard K %d W %d per %d mpad %-3d %-4s nb_uf %-3d nl %-2d m %-3d grad %d  " % (K, W, per, mpad, what, nb_uf, nl, m, grad)
          + "  ".join("%s: %s" % (k, "same bits" if v else "DIFFERENT") for k, v in checks.items()) + "  " + ("ok" if ok else "BAD"))
    return ok


if __name__ == "__main__":
    sys.exit(host_check.main("sparse_shard_host_check", CASES, run))
