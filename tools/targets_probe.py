"""Multi-target regression against what a user could do before it, on one GPU: milliseconds per evaluation (LL + gradient
at a new theta every call), interleaved call by call in one process after two warm-up rounds.
Cases: D = 10, N = 1500, 4096, 8192, m = 1, 4, 16, 64 targets (tests/truth_targets.py's, on synth data).

    a  one loglik_grad_targets: the handle's own evaluation + Z, A, the one-pass gradient, the final sums
    b  one single-target loglik_grad on the same handle
    c  m single-target evaluations, cugp_set_data(X, Y[t]) + loglik_grad for each t: all a user of a library without
       the targets calls can do
    pt / p1  predict_targets against the single-target prediction at 1000 test points, on a valid handle

Per case, over --reps calls: medians, min, max and spread (max - min) of each, a - b, and c / a.  The new kernels' own
dispatch times come from running the same probe once under the profiler (a run of its own, no counters, the program
after the double dash); --trace-csv turns that run's kernel trace into median dispatch times per (N, m) -- the launches
of a kernel appear in the probe's order, (2 + reps) evaluations per case:

    python tools/targets_probe.py [--reps 10] [--json profiles/targets_probe.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d out -- python tools/targets_probe.py --reps 3
    python tools/targets_probe.py --reps 3 --trace-csv out/.../..._kernel_trace.csv

--single: the existing single-target evaluation alone (LL + gradient at a new theta every call, medians of --reps after two
warm-ups, the LL at the base theta to 17 digits), with --lib on another libcugp.so (the parent commit's, which lacks the
targets calls): the alternating-process comparison of this build against its parent.
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

NS = (1500, 4096, 8192)
MS = (1, 4, 16, 64)
D = 10
NT = 1000
NEW = ("k_targets_alpha", "k_trace_targets", "k_finalize_targets", "k_targets_mean",
       "k_targets_mean_finish")


def stats(t):
    return {"median_ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4),
            "spread_ms": round(max(t) - min(t), 4)}


def npad(n):
    return (n + 127) // 128 * 128


def trace_report(path, reps, ns, ms):
    """Median dispatch time (End - Start, microseconds) of every new kernel, and of the k_predict_gemm launch that forms
    Z = Y L^-T (told from a prediction's by its grid: one 128-row tile of targets), per (N, m) of a probe run."""
    import csv
    import re
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    acc = {}
    for r in rows:
        name = re.sub(r"^void |cugp::|<.*$|\(.*$", "", r["Kernel_Name"])
        us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3
        if name in NEW:
            acc.setdefault(name, []).append(us)
        elif name == "k_predict_gemm":
            gx = int(r["Grid_Size_X"]) // 256
            if any(gx == 2 * (npad(n) // 128) for n in ns):
                acc.setdefault("k_predict_gemm(Z)", []).append(us)
    cases = [(n, m) for n in ns for m in ms]
    out = []
    for name, v in sorted(acc.items()):
        per = len(v) // len(cases)
        if per * len(cases) != len(v) or per == 0:
            out.append({"kernel": name, "launches": len(v), "median_us": round(statistics.median(v), 2),
                        "note": "launch count is no multiple of the case count: not split by case"})
            continue
        for i, (n, m) in enumerate(cases):
            g = v[i * per: (i + 1) * per]
            out.append({"kernel": name, "n": n, "m": m, "launches": per, "median_us": round(statistics.median(g), 2),
                        "min_us": round(min(g), 2), "max_us": round(max(g), 2)})
    print(json.dumps(out, indent=1))


def single_probe(args, ns):
    from cugp_amd import capi
    if args.lib:                                     # another build: bind what it has
        import ctypes
        capi.LIB_PATH = os.path.abspath(args.lib)
        capi._share_torch_hip_runtime()
        other = ctypes.CDLL(capi.LIB_PATH)
        capi.SIGNATURES = {k: v for k, v in capi.SIGNATURES.items() if hasattr(other, k)}
    import cugp_amd.gp as gp
    from conftest import synth
    hp = [float(np.log(3.0)), 0.0, float(np.log(0.1))]
    out = {"reps": args.reps, "build_id": capi.lib().cugp_build_id().decode(), "lib": args.lib or "tree", "single": []}
    for n in ns:
        X, y = synth(n, D, seed=15618)
        g = gp.Covsum(n, D, 0)
        g.set_data(X, y)
        t = []
        for i in range(2 + args.reps):
            g.set_loghyperparam([hp[0] + 1e-4 * (i + 1), hp[1], hp[2]])
            t0 = time.perf_counter()
            g.loglik_grad()
            if i >= 2:
                t.append((time.perf_counter() - t0) * 1e3)
        g.set_loghyperparam(hp)
        ll, gr = g.loglik_grad()
        row = dict(n=n, ll="%.17g" % ll, g=["%.17g" % v for v in gr], **stats(t))
        out["single"].append(row)
        g.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--single", action="store_true", help="the single-target evaluation alone (with --lib: on another library)")
    ap.add_argument("--lib", default="", help="--single: another libcugp.so to load instead of the tree's")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--json", default="")
    ap.add_argument("--ns", default=",".join(map(str, NS)))
    ap.add_argument("--ms", default=",".join(map(str, MS)))
    ap.add_argument("--trace-csv", default="", help="a rocprofv3 kernel trace of a probe run with the same --reps / --ns / --ms")
    args = ap.parse_args()
    ns, ms = [int(v) for v in args.ns.split(",")], [int(v) for v in args.ms.split(",")]
    if args.trace_csv:
        return trace_report(args.trace_csv, args.reps, ns, ms)
    if args.single:
        return single_probe(args, ns)

    import cugp_amd.gp as gp
    import truth_targets
    from cugp_amd import capi
    from conftest import synth

    hp = [float(np.log(3.0)), 0.0, float(np.log(0.1))]
    out = {"reps": args.reps, "build_id": capi.lib().cugp_build_id().decode(), "d": D, "nt": NT, "cases": []}
    for n in ns:
        X, y = synth(n, D, seed=15618)
        Xt = np.ascontiguousarray(X[:NT] * 0.5)
        Yall = truth_targets.targets(y, max(ms))
        g = gp.Covsum(n, D, 0)
        g.set_data(X, y)
        step = [0]

        def theta():
            step[0] += 1
            return [hp[0] + 1e-4 * step[0], hp[1], hp[2]]

        def run_a():
            g.set_loghyperparam(theta())
            return g.loglik_grad_targets()[0]

        def run_b():
            g.set_loghyperparam(theta())
            return g.loglik_grad()[0]

        for m in ms:
            Y = Yall[:m]
            g.set_targets(Y.T)

            def run_c():
                g.set_loghyperparam(theta())
                ll = 0.0
                for t in range(m):
                    g.set_data(X, Y[t])
                    ll = ll + g.loglik_grad()[0]
                return ll
            t = {k: [] for k in ("a", "b", "c", "pt", "p1")}
            for i in range(2 + args.reps):           # two warm-up rounds (allocations, graph capture), then the timed ones
                for k, fn in (("a", run_a), ("b", run_b), ("c", run_c)):
                    t0 = time.perf_counter()
                    fn()
                    if i >= 2:
                        t[k].append((time.perf_counter() - t0) * 1e3)
                g.loglik_grad_targets()              # both predictions from a valid handle: the N^2 part alone
                for k, fn in (("pt", lambda: g.predict_targets(Xt)), ("p1", lambda: g.compute_test_means_and_variances(None, None, Xt))):
                    t0 = time.perf_counter()
                    fn()
                    if i >= 2:
                        t[k].append((time.perf_counter() - t0) * 1e3)
            # the same theta through both paths: the LL digits side by side
            g.set_loghyperparam(hp)
            ll_a = g.loglik_grad_targets()[0]
            ll_c = 0.0
            for tg in range(m):
                g.set_data(X, Y[tg])
                ll_c = ll_c + g.loglik_grad()[0]
            row = {"n": n, "m": m}
            row.update({k: stats(v) for k, v in t.items()})
            a, b, c = (statistics.median(t[k]) for k in "abc")
            row.update(a_minus_b_ms=round(a - b, 4), c_over_a=round(c / a, 3), c_minus_a_ms=round(c - a, 4),
                       ll_targets="%.15g" % ll_a, ll_single_sum="%.15g" % ll_c,
                       trace_bytes=(npad(n) // 64) * (npad(n) // 64 + 1) // 2 * 64 * 64 * 8,
                       outer_flop=2.0 * m * ((npad(n) // 64) * (npad(n) // 64 + 1) // 2) * 64 * 64)
            out["cases"].append(row)
            print(json.dumps(row), file=sys.stderr)
        g.close()
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
