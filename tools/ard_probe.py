"""ARD against the isotropic kernel on one GPU: milliseconds per log-likelihood + gradient evaluation of an isotropic and
an ARD handle (all length scales equal, so both factor the same K), interleaved call by call in one process (after
two warm-up evaluations and one 1000-point prediction each).
Cases: N = 1500, 4096, 8192 with D = 10, and N = 8192 with D = 2 and 33.

Per case, over --reps evaluations: the medians, the isotropic evaluation's spread (max - min) and the difference of
the medians.  The kernels' own dispatch times come from running this same probe once under the profiler (a run of its
own, the program after the double dash):

    python tools/ard_probe.py [--reps 10] [--json profiles/ard_probe.json]
    rocprofv3 --kernel-trace --stats -d out -- python tools/ard_probe.py --reps 3

k_trace_ard reads the lower 64x64 tiles of K^-1 once, as k_trace does: bytes = tiles * 64 * 64 * 8, reported here per
case so that the profiler's time turns into a share of the 8 TB/s HBM peak.
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

CASES = ((1500, 10), (4096, 10), (8192, 10), (8192, 2), (8192, 33))
HBM_PEAK_TBS = 8.0


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
    out = {"reps": args.reps, "build_id": capi.lib().cugp_build_id().decode(), "hbm_peak_tbs": HBM_PEAK_TBS, "cases": []}
    for n, d in CASES:
        X, y = synth(n, d, seed=15618)
        gi = gp.Covsum(n, d, 0)
        ga = gp.Covsum(n, d, 0, ard=True)
        for g in (gi, ga):
            g.set_data(X, y)
        gi.set_loghyperparam(hp)
        ga.set_loghyperparam([hp[0]] * d + hp[1:])

        def ev(g):
            g.enqueue(True)                 # a full evaluation whatever the handle holds
            return g.fetch()
        for _ in range(2):
            ri, ra = ev(gi), ev(ga)
        Xt = np.ascontiguousarray(X[:1000] * 0.5)    # one prediction each: k_cross / k_cross_ard appear in a kernel trace
        gi.compute_test_means_and_variances(X, y, Xt)
        ga.compute_test_means_and_variances(X, y, Xt)
        ti, tr = [], []
        for _ in range(args.reps):
            ti.append(timed(lambda: ev(gi)))
            tr.append(timed(lambda: ev(ga)))
        tiles = (gi_npad(n) // 64) * (gi_npad(n) // 64 + 1) // 2
        row = {"n": n, "d": d, "iso_ms": round(statistics.median(ti), 4), "ard_ms": round(statistics.median(tr), 4),
               "iso_spread_ms": round(max(ti) - min(ti), 4), "ard_minus_iso_ms": round(statistics.median(tr) - statistics.median(ti), 4),
               "trace_bytes": tiles * 64 * 64 * 8,
               "ll_rel_diff": abs(ra[0] - ri[0]) / abs(ri[0]),
               "grad_rel_diff": float(np.max(np.abs(np.array([ra[1][:d].sum(), ra[1][d], ra[1][d + 1]]) - ri[1])) / np.max(np.abs(ri[1])))}
        out["cases"].append(row)
        print(json.dumps(row), file=sys.stderr)
        gi.close()
        ga.close()
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


def gi_npad(n):
    return (n + 127) // 128 * 128


if __name__ == "__main__":
    main()
