"""Matern against the squared exponential on one GPU: milliseconds per log-likelihood + gradient evaluation of an SE, a
Matern 3/2 and a Matern 5/2 handle on the same data and hyper-parameters, interleaved call by call in one process
(after two warm-up evaluations and one 1000-point prediction and one 256-point joint covariance each).
Cases: N = 1500, 4096, 8192 with D = 10.

Per case, over --reps evaluations: the medians, the SE evaluation's spread (max - min) and the differences of the
medians.  The four kernels' own dispatch times come from running this same probe once under the profiler (a run of
its own, the program after the double dash; counters, if wanted, in yet another run):

    python tools/matern_probe.py [--reps 10] [--json profiles/matern_probe.json]
    rocprofv3 --kernel-trace --stats -d out -- python tools/matern_probe.py --reps 3
    (the k_build / k_cross / k_predict_cov_finish / k_trace lines of its kernel_stats: profiles/matern_kernel_stats.txt)

Acceptance: a Matern evaluation exceeds the SE evaluation by no more than the difference of
those kernels' dispatch times plus the SE evaluation's own spread.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

CASES = ((1500, 10), (4096, 10), (8192, 10))
KERNELS = ("se", "matern32", "matern52")


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--json", default="")
    args = ap.parse_args()

    import cugp_amd.gp as gp
    from cugp_amd import capi
    from conftest import synth

    hp = [float(np.log(3.0)), 0.0, float(np.log(0.1))]
    out = {"reps": args.reps, "build_id": capi.lib().cugp_build_id().decode(), "cases": []}
    for n, d in CASES:
        X, y = synth(n, d, seed=15618)
        hs = {k: gp.Covsum(n, d, 0, kernel=k) for k in KERNELS}
        for g in hs.values():
            g.set_data(X, y)
            g.set_loghyperparam(hp)

        def ev(g):
            g.enqueue(True)                 # a full evaluation whatever the handle holds
            return g.fetch()
        res = {}
        for _ in range(2):
            for k, g in hs.items():
                res[k] = ev(g)
        Xt = np.ascontiguousarray(X[:1000] * 0.5)    # k_cross and k_predict_cov_finish appear in a kernel trace
        for g in hs.values():
            g.compute_test_means_and_variances(X, y, Xt)
            g.compute_test_joint(X, y, Xt[:256])
        t = {k: [] for k in KERNELS}
        for _ in range(args.reps):
            for k, g in hs.items():
                t[k].append(timed(lambda: ev(g)))
        med = {k: statistics.median(v) for k, v in t.items()}
        row = {"n": n, "d": d, "se_ms": round(med["se"], 4), "matern32_ms": round(med["matern32"], 4),
               "matern52_ms": round(med["matern52"], 4), "se_spread_ms": round(max(t["se"]) - min(t["se"]), 4),
               "matern32_minus_se_ms": round(med["matern32"] - med["se"], 4),
               "matern52_minus_se_ms": round(med["matern52"] - med["se"], 4),
               "ll": {k: res[k][0] for k in KERNELS}}
        out["cases"].append(row)
        print(json.dumps(row), file=sys.stderr)
        for g in hs.values():
            g.close()
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
