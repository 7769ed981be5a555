"""What p targets over one set of inducing points cost beside one (one GPU; needs the built library):

    python tools/sparse_targets_probe.py --json profiles/sparse_targets_probe.json   # N = 1e5, 1e6; M = 512, 1024, 2048; D = 10; SE
    python tools/sparse_targets_probe.py --sizes 100000 --inducing 1024 --targets 16 --once   # for a rocprofv3 --kernel-trace --stats run

Per (N, M), medians of --reps calls at fresh hyper-parameter vectors, host clock around the synchronous call, in ms,
chunk_rows 16384, on ONE handle in one process:
  single_ms / single_z_ms     cugp_sparse_bound_grad / cugp_sparse_bound_grad_z on the handle's own y
  targets[p].ms / .z_ms       cugp_sparse_bound_grad_targets / cugp_sparse_bound_grad_z_targets with p targets
  .over_single                targets[p].ms / single_ms: what p targets cost in single evaluations
  .over_p_singles             targets[p].ms / (p single_ms): below 1 where sharing beats p evaluations
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


def model(n, m, d, ps, reps, once=False):
    import cugp_amd.gp as gp
    from conftest import synth
    X, y = synth(n, d, seed=15618)
    s = gp.SparseGP.from_subset(X, y, m, seed=0, chunk_rows=CHUNK)
    rng = np.random.default_rng(11)
    Y = np.stack([y] + [np.roll(y, 7 * t) * (1 + 0.25 * t) + 0.3 * rng.standard_normal(n) for t in range(1, max(ps))], axis=1)
    count = [0]

    def hyper():
        count[0] += 1
        s.set_loghyperparam([float(np.log(3.0)) + 1e-3 * count[0], 0.0, float(np.log(0.1))])
    if once:
        s.set_targets(Y[:, : max(ps)])
        for _ in range(3):
            hyper()
            print(n, m, max(ps), s.bound_grad_z_targets()[0], flush=True)
        s.close()
        return None

    def timed(call):
        def fn(_):
            hyper()
            call()
        return median_ms(fn, reps)
    out = dict(family="se", n=n, m=m, d=d, chunks=len(s.plan()))
    out["single_ms"], out["single_z_ms"] = timed(s.bound_grad), timed(s.bound_grad_z)
    out["targets"] = {}
    for p in ps:
        s.set_targets(Y[:, :p])
        r = dict(ms=timed(s.bound_grad_targets), z_ms=timed(s.bound_grad_z_targets))
        r.update(over_single=r["ms"] / out["single_ms"], over_p_singles=r["ms"] / (p * out["single_ms"]),
                 z_over_single=r["z_ms"] / out["single_z_ms"], z_over_p_singles=r["z_ms"] / (p * out["single_z_ms"]))
        F, g, gZ, each = s.bound_grad_z_targets()
        r["F"], r["finite"] = F, bool(np.all(np.isfinite(g)) and np.all(np.isfinite(gZ)) and np.all(np.isfinite(each)))
        out["targets"][str(p)] = r
    s.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--inducing", type=int, nargs="+", default=[512, 1024, 2048])
    ap.add_argument("--targets", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--dims", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--once", action="store_true", help="three evaluations with the most targets per case, nothing timed")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    rows = []
    for n in args.sizes:
        for m in args.inducing:
            r = model(n, m, args.dims, args.targets, args.reps, args.once)
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
