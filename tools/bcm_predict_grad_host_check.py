"""The batched test-input gradient kernels and the device chain rule of a product of experts on the CPU, without a GPU: the
kernels' own text (cugp_amd/csrc/cov_device.h and bcm_grad_device.h, the headers kernels.hip includes) in a lock-step host
emulation (tools/bcm_predict_grad_host_check.cpp) built with -fsanitize=address,undefined.

  grad    k_predict_grad_batched<ARD, KIND> and k_predict_grad_finish_batched on three experts that share npad = 128 with
          n = 64, 64, 66 -- 1, 1 and 2 training tiles: the smallest shape at which the early return of a workgroup beyond
          its expert's tiles and the per-expert tile count can go wrong; at d = 3 also in the order 66, 64, 64, where a
          missing early return reads past the end of Ks and V -- at nt = 65 (two test tiles, the second ragged),
          d = 3 and 17 (DC + 1: a second feature chunk), with and without V, for SE-ARD, Matern-5/2-ARD and isotropic SE.
          alpha, Ks and V carry NaN wherever the kernels must not use them.  Every expert's slot of the rows must carry the
          BITS of the existing single-expert kernels (k_predict_grad, k_predict_grad_finish) run in the same emulation on
          the expert's slices; the m and v parts of the rows, and without V the dvar part, must be left untouched.
  reduce  k_poe_reduce_grad against the host path of cugp_bcm_predict_grad -- rows made as poe_row makes them through
          cugp_poe_combine, or the two sums and cugp_poe_finish for the reference's product, and cugp_poe_combine_grad
          (libcugp.so's host code, which needs no GPU) -- K = 1, 3, 5 experts over a world of 1 and 2 (expert k in rank
          k mod world's slot k / world, unused slots NaN), nt = 1 and 257, all five modes: bit for bit in all four
          outputs (both sides use the host's log here, so rbcm too); the status words copied; one expert under POE
          returns its own dmean exactly.

    python tools/bcm_predict_grad_host_check.py          # builds into a temporary directory
"""
import os
import struct
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import host_check  # noqa: E402  (also puts the repository root and tests/ on the path)

INSTANCES = {"se_ard": (0, 1), "matern52_ard": (2, 1), "se": (0, 0)}          # name -> (kind, ard)
NPAD, NT = 128, 65
# n per expert.  "last": the expert with two training tiles last; "first": the same experts with it first, so that the
# surplus workgroups of the LAST expert -- the ones the early return of k_predict_grad_batched stops -- would read Ks and V
# past the end of the heap blocks, where AddressSanitizer sees a missing guard (with it last they would stay inside)
# "small": experts of 1, 2 and 63 rows -- one live training row, two, and one short of a build tile, in one padded size
ORDERS = {"last": (64, 64, 66), "first": (66, 64, 64), "small": (1, 2, 63)}
CASES = tuple(("grad", inst, d, want_v, "last") for inst in INSTANCES for d in (3, 17) for want_v in (1, 0)) + \
        tuple(("grad", inst, 3, want_v, "first") for inst in INSTANCES for want_v in (1, 0)) + \
        tuple(("grad", inst, 3, 1, "small") for inst in INSTANCES) + \
        tuple(("reduce", K, world, nt) for K in (1, 3, 5) for world in (1, 2) for nt in (1, 257))
MODES = (-1, 0, 1, 2, 3)
SF2, SN2, ELL2 = 1.4918246976412703, 0.1353352832366127, 2.25


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def run_grad(exe, tmp, inst, d, want_v, order="last"):
    kind, ard = INSTANCES[inst]
    N_EXPERTS = ORDERS[order]
    rng = np.random.default_rng(100 * d + 10 * kind + ard)
    K, nt, npad, cpad = len(N_EXPERTS), NT, NPAD, (NT + 127) // 128 * 128
    w = rng.uniform(0.4, 0.9, d)
    Xt = rng.uniform(-2, 2, (nt, d))
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    Ks, V, experts = np.full((K, cpad, npad), np.nan), np.full((K, cpad, npad), np.nan), []
    for k, n in enumerate(N_EXPERTS):
        X = rng.uniform(-2, 2, (n, d))
        a = np.full(npad, np.nan)
        a[:n] = rng.standard_normal(n)
        experts.append((X, a))
        diff = Xt[:, None, :] - X[None, :, :]
        s = ((diff * w) ** 2).sum(2) if ard else (diff ** 2).sum(2) / ELL2
        if kind == 0:
            Ks[k, :nt, :n] = SF2 * np.exp(-0.5 * s)           # (the Matern kinds never read Ks: all NaN)
        V[k, :nt, :n] = rng.standard_normal((nt, n)) / n
    with open(fin, "wb") as f:
        f.write(struct.pack("9i", 0, K, d, npad, nt, cpad, kind, ard, want_v))
        f.write(struct.pack("%di" % K, *N_EXPERTS))
        f.write(struct.pack("3d", ELL2, SF2, SN2))
        for arr in [w] + [x for e in experts for x in e] + [Xt, Ks, V]:
            f.write(np.ascontiguousarray(arr, dtype=np.float64).tobytes())
    if not host_check.execute(exe, fin, fout, "grad", inst, d, want_v):
        return False
    slot = (2 + 2 * d) * nt
    out = np.fromfile(fout).reshape(2, K, slot)
    rows, single = out[0], out[1]
    g0, g1 = 2 * nt, 2 * nt + nt * d
    ok = bool(np.all(np.isnan(rows[:, :g0])))                                   # m and v: not these kernels' to write
    ok = ok and same_bits(rows[:, g0:g1], single[:, g0:g1]) and bool(np.all(np.isfinite(rows[:, g0:g1])))
    if want_v:
        ok = ok and same_bits(rows[:, g1:], single[:, g1:]) and bool(np.all(np.isfinite(rows[:, g1:])))
    else:
        ok = ok and bool(np.all(np.isnan(rows[:, g1:])))                        # the dvar part is left untouched
    # the experts differ: a slot filled from another expert's table entry or slice would not go unnoticed
    ok = ok and not same_bits(rows[0, g0:g1], rows[1, g0:g1]) and not same_bits(rows[1, g0:g1], rows[2, g0:g1])
    print("grad   %-13s d %-2d dvar %d   3 experts (n = %d, %d, %d), nt 65: slots against the single-expert kernels, bit for bit  %s"
          % ((inst, d, want_v) + N_EXPERTS + ("ok" if ok else "BAD",)))
    return ok


def host_path(gp, m, v, dm, dv, mode, with_noise):
    """cugp_bcm_predict_grad's host arithmetic on the experts' rows -> (mean, var, dmean, dvar)."""
    inv = 1.0 / v
    if mode < 0:
        sp, spm = np.zeros(m.shape[1]), np.zeros(m.shape[1])
        for k in range(len(m)):
            sp += inv[k]
            spm += inv[k] * m[k]
        mean, var = gp.poe_finish(sp, spm)
    else:
        mean, var = gp.poe_combine(np.stack([inv, inv * m], axis=1), mode, SF2, SN2, with_noise)
    return (mean, var) + gp.poe_combine_grad(m, v, dm, dv, mode, SF2)


def run_reduce(exe, tmp, K, world, nt, d=3):
    import cugp_amd.gp as gp
    rng = np.random.default_rng(1000 * K + 10 * world + nt)
    per = -(-K // world) + (1 if K == 3 else 0)               # (K = 3: one slot more than needed, never read)
    v = SF2 * rng.uniform(0.02, 1.0, (K, nt))
    v[rng.uniform(size=(K, nt)) < 0.15] = SF2                  # some experts exactly uninformative
    m, dm, dv = rng.standard_normal((K, nt)), rng.standard_normal((K, nt, d)), 0.3 * rng.standard_normal((K, nt, d))
    slot = (2 + 2 * d) * nt
    rstride = 2 + per * slot
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    ok = True
    for mode in MODES:
        vv = v + SN2 if mode < 0 else v                        # the reference's product takes the noisy variances
        g = np.full((world, rstride), np.nan)
        for r in range(world):
            g[r, 0], g[r, 1] = 0.0, len(range(r, K, world))
        for k in range(K):
            s = g[k % world, 2 + (k // world) * slot:][:slot]
            s[:nt], s[nt:2 * nt], s[2 * nt:2 * nt + nt * d], s[2 * nt + nt * d:] = m[k], vv[k], dm[k].ravel(), dv[k].ravel()
        for with_noise, want_dvar in ((1, 1), (0, 1), (1, 0)):
            with open(fin, "wb") as f:
                f.write(struct.pack("9i", 1, world, K, nt, d, per, mode, with_noise, want_dvar))
                f.write(struct.pack("2d", SF2, SN2))
                f.write(g.tobytes())
            if not host_check.execute(exe, fin, fout, "reduce", K, world, nt, mode):
                return False
            out = np.fromfile(fout)
            want = host_path(gp, m, vv, dm, dv, mode, with_noise)
            nd = nt * d
            got = (out[:nt], out[nt:2 * nt], out[2 * nt:2 * nt + nd].reshape(nt, d), out[2 * nt + nd:2 * nt + 2 * nd].reshape(nt, d))
            good = all(same_bits(a, b) for a, b in zip(got[:3], want[:3]))
            good = good and (same_bits(got[3], want[3]) if want_dvar else bool(np.all(np.isnan(got[3]))))
            good = good and same_bits(out[2 * nt + 2 * nd:], g[:, :2].ravel())
            if K == 1 and mode in (-1, 0):
                good = good and same_bits(got[2], dm[0])       # one expert under POE: its own gradient, exactly
            if not good:
                print("reduce K %d world %d nt %d mode %d with_noise %d want_dvar %d: differs from the host path" % (
                    K, world, nt, mode, with_noise, want_dvar))
            ok = ok and good
    print("reduce K %d world %d nt %-3d   five modes against cugp_poe_combine / cugp_poe_finish / cugp_poe_combine_grad, bit for bit  %s"
          % (K, world, nt, "ok" if ok else "BAD"))
    return ok


def run(exe, tmp, kernel, *case):
    return run_grad(exe, tmp, *case) if kernel == "grad" else run_reduce(exe, tmp, *case)


if __name__ == "__main__":
    sys.exit(host_check.main("bcm_predict_grad_host_check", CASES, run))
