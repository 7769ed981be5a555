"""Appending observations (cugp_append) on one GPU: milliseconds per call against the full evaluation it replaces.

Models: N = 8192 rows, D = 10 (bench.py's) in a handle of capacity 8320, and N = 1500 in one of capacity 1664.  Per model
and k in {1, 128} (at N = 8192 both a single pass of cugp_append_plan; at N = 1500 the 128 rows cross row 1536: two passes),
both calls straight through the C ABI, medians over --reps rounds of, alternating in one process:
  append_ms   cugp_append of k rows to a handle that holds its inverse quantities for N rows.  A host clock around the call,
              which ends in a device synchronise.  Rows cannot be removed, so every round has a handle of its own; it is
              warmed up and then brought to a FRESH evaluated state at N rows: created with N - 1 rows, evaluated, one row
              appended (the first append of a handle allocates its scratch, grows X and creates the factor handle), then
              the hyper-parameters are moved away and back and the N rows are evaluated from scratch.
  eval_ms     cugp_loglik_grad from stale at N + k rows on a second handle of the same capacity (the hyper-parameters
              moved away and back in front of every call; the evaluation at the other point is not timed).
Conditions, reported as booleans under "conditions":
  the median 128-row append at N = 8192 takes at most a quarter of the median full evaluation measured beside it;
  the 1-row append takes no longer than the 128-row one.

    python tools/append_probe.py [--reps 20] [--json profiles/append_probe.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d out -- python tools/append_probe.py --trace-run
        (--trace-run: per model one warmed handle, evaluated at N, ONE 128-row append and ONE 1-row append on a second
         handle, nothing else: the kernel statistics of the append's launches -> profiles/append_kernel_stats.txt)
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

MODELS = ((8192, 10), (1500, 10))
KS = (1, 128)
PEAK_HBM = 8.0             # TB/s, MI355X


def capacity_for(n):
    return (n + 128 + 127) // 128 * 128


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default="")
    ap.add_argument("--trace-run", action="store_true")
    args = ap.parse_args()

    import cugp_amd.gp as gp
    from cugp_amd import capi
    from conftest import synth

    L = capi.lib()
    hp = np.array([np.log(3.0), 0.0, np.log(0.1)])
    away = hp + 0.05

    def warmed(X, y, n, cap):
        """A handle with a fresh evaluation at n rows whose first append (allocations) is behind it."""
        g = gp.Covsum(n - 1, X.shape[1], 0, npad_min=cap)
        g.set_loghyperparam(hp)
        g.set_data(X[:n - 1], y[:n - 1])
        g.loglik_grad()
        g.append(X[n - 1], y[n - 1])
        g.set_loghyperparam(away)
        g.loglik_grad()
        g.set_loghyperparam(hp)
        g.loglik_grad()
        return g

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    out = {"reps": args.reps, "build_id": capi.lib().cugp_build_id().decode(), "peak_hbm_tbs": PEAK_HBM, "cases": []}
    for n, d in MODELS:
        cap = capacity_for(n)
        X, y = synth(n + 128, d, seed=15618)
        if args.trace_run:
            for k in KS:
                g = warmed(X, y, n, cap)
                g.append(X[n: n + k], y[n: n + k])
                g.close()
            continue
        for k in KS:
            f = gp.Covsum(n + k, d, 0, npad_min=cap)
            f.set_data(X[:n + k], y[:n + k])

            ll_c, gr_c = C.c_double(), np.empty(3)
            Xk, yk = np.ascontiguousarray(X[n: n + k]), np.ascontiguousarray(y[n: n + k])

            def full():
                f.set_loghyperparam(hp)
                return timed(lambda: capi.check(L.cugp_loglik_grad(f.handle, C.byref(ll_c), capi.ptr(gr_c))))
            f.set_loghyperparam(hp)
            f.loglik_grad()
            ta, te, lls = [], [], []
            for rep in range(args.reps + 2):                         # two warm-up rounds
                g = warmed(X, y, n, cap)
                t = timed(lambda: capi.check(L.cugp_append(g.handle, capi.ptr(Xk), capi.ptr(yk), k)))
                g.n, g._data_key = n + k, None                       # (the wrapper's bookkeeping, by hand)
                lls.append(g.loglik_grad()[0])
                g.close()
                f.set_loghyperparam(away)
                f.loglik_grad()
                e = full()
                if rep >= 2:
                    ta.append(t)
                    te.append(e)
            ll_full = f.loglik_grad()[0]
            f.close()
            row = {"n": n, "d": d, "capacity": cap, "k": k, "append_ms": round(statistics.median(ta), 4),
                   "append_ms_min": round(min(ta), 4), "eval_ms": round(statistics.median(te), 4),
                   "eval_ms_min": round(min(te), 4), "ratio": round(statistics.median(ta) / statistics.median(te), 4),
                   "ll_append": lls[-1], "ll_full": ll_full}
            out["cases"].append(row)
            print(json.dumps(row), file=sys.stderr)
    if args.trace_run:
        return
    by = {(r["n"], r["k"]): r for r in out["cases"]}
    out["conditions"] = {
        "append128_at_8192_within_a_quarter_of_eval": by[8192, 128]["append_ms"] <= 0.25 * by[8192, 128]["eval_ms"],
        "append1_no_longer_than_append128_at_8192": by[8192, 1]["append_ms"] <= by[8192, 128]["append_ms"],
        "append1_no_longer_than_append128_at_1500": by[1500, 1]["append_ms"] <= by[1500, 128]["append_ms"],
    }
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
