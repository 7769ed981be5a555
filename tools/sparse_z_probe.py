"""What the gradient with respect to the inducing inputs costs on top of bound + gradient (one GPU; needs the built library):

    python tools/sparse_z_probe.py --json profiles/sparse_z_probe.json     # N = 1e5, 1e6; M = 512, 1024, 2048; D = 10; SE, SE-ARD
    python tools/sparse_z_probe.py --sizes 100000 --inducing 1024 --once   # one pass, for a rocprofv3 --kernel-trace --stats run

Per (family, N, M), medians of --reps calls at fresh hyper-parameter vectors, host clock around the synchronous call, in ms,
chunk_rows 16384:
  bound_grad     cugp_sparse_bound_grad
  bound_grad_z   cugp_sparse_bound_grad_z: the same sequence with k_trace_cross_z and k_trace_cross_z_finish behind every
                 k_trace_cross (one pair per chunk, one for the square)
  extra          bound_grad_z / bound_grad - 1
and the pass's shape (sparse_z_shape, replayed here): workgroups of the chunk's launch and row tiles per workgroup.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

CHUNK = 16384


def median_ms(fn, reps):
    ts = []
    for i in range(1 + reps):                                # (one warm-up call)
        t0 = time.perf_counter()
        fn(i)
        ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts[1:]))


def z_shape(rows_pad, mpad, d):
    """sparse_z_shape of sparse_gfx950.h: (row tiles, per workgroup, ranges per column tile)."""
    tiles, nct = rows_pad // 64, mpad // 64
    ranges = max(1, min(512 // nct, rows_pad // 256))
    while ranges > 1 and ranges * mpad * d * 8 > 1 << 30:
        ranges -= 1
    per = -(-tiles // ranges)
    return tiles, per, -(-tiles // per)


def model(n, m, d, ard, reps, once=False):
    import cugp_amd.gp as gp
    from conftest import synth
    X, y = synth(n, d, seed=15618)
    s = gp.SparseGP.from_subset(X, y, m, seed=0, ard=ard, chunk_rows=CHUNK)

    def hyper(i):
        ell = float(np.log(3.0)) + 1e-3 * i
        s.set_loghyperparam(([ell] * d if ard else [ell]) + [0.0, float(np.log(0.1))])
    if once:
        for i in range(3):
            hyper(i)
            print(n, m, "ard" if ard else "se", s.bound_grad_z()[0], flush=True)
        s.close()
        return None

    def bound_grad(i):
        hyper(100 + i)
        s.bound_grad()

    def bound_grad_z(i):
        hyper(200 + i)
        s.bound_grad_z()
    mp = -(-m // 128) * 128
    tiles, per, ranges = z_shape(min(n, CHUNK) // 128 * 128 or 128, mp, d)
    out = dict(family="se_ard" if ard else "se", n=n, m=m, d=d, chunks=len(s.plan()), z_workgroups=ranges * (mp // 64),
               z_row_tiles_per_workgroup=per)
    out["bound_grad_ms"] = median_ms(bound_grad, reps)
    out["bound_grad_z_ms"] = median_ms(bound_grad_z, reps)
    out["extra"] = out["bound_grad_z_ms"] / out["bound_grad_ms"] - 1.0
    F, g, gZ = s.bound_grad_z()
    out["F"], out["finite"] = F, bool(np.all(np.isfinite(g)) and np.all(np.isfinite(gZ)))
    s.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--inducing", type=int, nargs="+", default=[512, 1024, 2048])
    ap.add_argument("--families", nargs="+", default=["se", "se_ard"], choices=["se", "se_ard"])
    ap.add_argument("--dims", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--once", action="store_true", help="three evaluations with the Z gradient per case, nothing timed")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    rows = []
    for fam in args.families:
        for n in args.sizes:
            for m in args.inducing:
                r = model(n, m, args.dims, fam == "se_ard", args.reps, args.once)
                if r:
                    rows.append(r)
                    print(json.dumps(r), flush=True)
    if args.json and rows:
        from cugp_amd import capi
        doc = dict(build_id=(capi.lib().cugp_build_id() or b"unknown").decode(), reps=args.reps, chunk_rows=CHUNK, rows=rows)
        with open(args.json, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
