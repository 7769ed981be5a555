"""Rational quadratic against SE-ARD on one GPU: milliseconds per log-likelihood + gradient evaluation of an SE-ARD handle,
an "rq_ard" handle (nh = d + 3) and an "rq" handle (one tied length scale, nh = 4) on the same data and length scales,
interleaved call by call in one process (after two warm-up evaluations each).  Cases: N = 1500 and 8192 with D = 10.

Per case, over --reps evaluations: the medians, the SE-ARD evaluation's spread (max - min) and the differences of the
medians.  The kernels' own dispatch times come from running the probe's --once mode under the profiler (a run of its own,
nothing else traced, the program after the double dash); --once evaluates every family --reps times at every size without
timing anything on the host:

    python tools/rq_probe.py [--reps 10] [--json profiles/rq_probe.json]
    rocprofv3 --kernel-trace --stats -d out -- python tools/rq_probe.py --once --reps 3

Acceptance (the rational quadratic section): consistency -- the difference between an RQ and the SE-ARD whole
evaluation equals the summed difference of their k_build, k_trace and k_finalize_ard launches in the kernel statistics,
within the SE-ARD evaluation's own spread over the repeats.  Anything beyond that would be a pass outside the covariance
function that got slower.  Not timed here: targets, leave-one-out, input gradients, the product of experts.
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

SIZES = (1500, 8192)
D = 10
THETA_ALPHA = 0.4
FAMILIES = (("se_ard", dict(ard=True)), ("rq_ard", dict(kernel="rq_ard")), ("rq", dict(kernel="rq")))


def stats(t):
    return {"median_ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4),
            "spread_ms": round(max(t) - min(t), 4)}


def theta(name):
    length, tail = float(np.log(3.0)), [0.0, float(np.log(0.1))]
    if name == "se_ard":
        return [length] * D + tail
    return ([length] * D if name == "rq_ard" else [length]) + [THETA_ALPHA] + tail


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--json", default="")
    ap.add_argument("--sizes", type=int, nargs="*", default=list(SIZES))
    ap.add_argument("--once", action="store_true", help="no host timing: the run a kernel trace is taken of")
    args = ap.parse_args()

    from cugp_amd import capi
    import cugp_amd.gp as gp
    from conftest import synth

    out = {"reps": args.reps, "build_id": capi.lib().cugp_build_id().decode(), "d": D, "theta_alpha": THETA_ALPHA, "cases": []}
    for n in args.sizes:
        X, y = synth(n, D, seed=15618)
        hs = {}
        for name, kw in FAMILIES:
            g = hs[name] = gp.Covsum(n, D, 0, **kw)
            g.set_data(X, y)
            g.set_loghyperparam(theta(name))

        def ev(g):
            g.enqueue(True)                 # a full evaluation whatever the handle holds
            return g.fetch()[0]
        t, ll = {v: [] for v in hs}, {}
        for i in range(2 + args.reps):      # two warm-up rounds (allocations, graph capture), the families in turn
            for v, g in hs.items():
                t0 = time.perf_counter()
                ll[v] = ev(g)
                if i >= 2:
                    t[v].append((time.perf_counter() - t0) * 1e3)
        row = {"n": n}
        if not args.once:
            row.update({v: stats(t[v]) for v in t})
            for v in ("rq_ard", "rq"):
                row[v]["minus_se_ard_ms"] = round(row[v]["median_ms"] - row["se_ard"]["median_ms"], 4)
        row["evaluations_per_family"] = 2 + args.reps
        row["ll"] = {v: float(ll[v]).hex() for v in ll}
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
