"""ARD against the isotropic kernel on one GPU: milliseconds per log-likelihood + gradient evaluation of an isotropic and
an ARD handle (all length scales equal, so both factor the same K), interleaved call by call in one process (after
two warm-up evaluations and one 1000-point prediction each).
Cases: N = 1500, 4096, 8192 with D = 10, and N = 8192 with D = 2 and 33.

Per case, over --reps evaluations: the medians, the isotropic evaluation's spread (max - min) and the difference of
the medians.  The kernels' own dispatch times come from running this same probe once under the profiler (a run of its
own, the program after the double dash):

    python tools/ard_probe.py [--reps 10] [--json profiles/ard_probe.json]
    rocprofv3 --kernel-trace --stats -d out -- python tools/ard_probe.py --reps 3

k_trace<true, 0> (ARD) reads the lower 64x64 tiles of K^-1 once, as k_trace<false, 0> does: bytes = tiles * 64 * 64 * 8, reported here per
case so that the profiler's time turns into a share of the 8 TB/s HBM peak.

--bcm: the ARD product of experts instead, at 16 x 1500 and 4 x 6000 rows with D = 10, per evaluation (LL + gradient at a
new theta every time), interleaved call by call in one process:
    a  an ARD BCM (gp.BCM(ard=True): the experts as one group of shared launches)
    b  the same experts as 16 (4) single ARD handles, each enqueued before the first is fetched -- what a user can do
       without the ARD BCM
    c  the isotropic BCM of the same shape
--variants picks among them (a library without cugp_bcm_create_ard runs b and c); --lib loads another libcugp.so (the
parent commit's, for the alternating-process comparison); --trace-csv turns a rocprofv3 kernel trace of a --variants ac run
into mean dispatch times of k_trace<true, 0>, k_finalize_ard and k_trace<false, 0> per shape (the grid's y extent tells the shapes apart):

    python tools/ard_probe.py --bcm [--reps 10] [--json out.json] [--lib other/libcugp.so] [--variants abc]
    rocprofv3 --kernel-trace --output-format csv -d out -- python tools/ard_probe.py --bcm --reps 3 --variants ac
    python tools/ard_probe.py --trace-csv out/.../..._kernel_trace.csv
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


BCM_SHAPES = ((16, 1500), (4, 6000))
BCM_D = 10


def stats(t):
    return {"median_ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4),
            "spread_ms": round(max(t) - min(t), 4)}


def bcm_probe(args):
    from cugp_amd import capi
    if args.lib:                                     # another build: bind what it has (an older one lacks the ARD BCM)
        import ctypes
        capi.LIB_PATH = os.path.abspath(args.lib)
        capi._share_torch_hip_runtime()
        other = ctypes.CDLL(capi.LIB_PATH)
        capi.SIGNATURES = {k: v for k, v in capi.SIGNATURES.items() if hasattr(other, k)}
    import cugp_amd.gp as gp
    from conftest import synth
    variants = [v for v in args.variants if v != "a" or "cugp_bcm_create_ard" in capi.SIGNATURES]
    hp = [float(np.log(3.0)), 0.0, float(np.log(0.1))]
    out = {"reps": args.reps, "build_id": capi.lib().cugp_build_id().decode(), "d": BCM_D, "variants": "".join(variants),
           "shapes": []}
    for K, n in BCM_SHAPES:
        X, y = synth(K * n, BCM_D, seed=15618)
        made, run = [], {}
        if "a" in variants:
            ba = gp.BCM.split(X, y, K, ard=True)
            made.append(ba)
            run["a"] = lambda e, ba=ba: (ba.set_BCM_log_hyperparam([hp[0] + e] * BCM_D + hp[1:]), ba.loglik_grad())[1][0]
        if "b" in variants:
            hs = [gp.Covsum(n, BCM_D, 0, ard=True) for _ in range(K)]
            for k, g in enumerate(hs):
                g.set_data(X[k * n: (k + 1) * n], y[k * n: (k + 1) * n])
            made += hs

            def run_b(e, hs=hs):
                for g in hs:
                    g.set_loghyperparam([hp[0] + e] * BCM_D + hp[1:])
                for g in hs:
                    g.enqueue(True)
                ll = 0.0
                for g in hs:
                    ll = ll + g.fetch()[0]
                return ll
            run["b"] = run_b
        if "c" in variants:
            bc = gp.BCM.split(X, y, K)
            made.append(bc)
            run["c"] = lambda e, bc=bc: (bc.set_BCM_log_hyperparam([hp[0] + e] + hp[1:]), bc.loglik_grad())[1][0]
        t, ll = {v: [] for v in run}, {}
        for i in range(2 + args.reps):               # two warm-up rounds (allocations, graph capture), then the timed ones
            e = 1e-3 * (i + 1)
            for v, fn in run.items():
                t0 = time.perf_counter()
                ll[v] = fn(e)
                if i >= 2:
                    t[v].append((time.perf_counter() - t0) * 1e3)
        row = {"experts": K, "rows": n}
        row.update({v: stats(t[v]) for v in t})
        row["ll"] = {v: float(ll[v]).hex() for v in ll}
        out["shapes"].append(row)
        print(json.dumps(row), file=sys.stderr)
        for m in made:
            m.close()
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


def trace_report(path):
    """Mean dispatch time (End - Start, microseconds) of the trace and finalize kernels of a --bcm --variants ac run per
    shape: batched launches carry the expert count in the grid's y extent."""
    import csv
    import re
    acc = {}
    for r in csv.DictReader(open(path)):
        name = re.sub(r"^void |cugp::|\(.*$", "", r["Kernel_Name"])
        if name not in ("k_trace<false, 0>", "k_trace<true, 0>", "k_finalize_ard", "k_finalize"):
            continue
        gy = int(r["Grid_Size_Y"]) // max(1, int(r["Workgroup_Size_Y"]))
        a = acc.setdefault((name, gy), [])
        a.append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3)
    out = [{"kernel": k, "experts": gy, "launches": len(v), "mean_us": round(sum(v) / len(v), 2),
            "median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}
           for (k, gy), v in sorted(acc.items())]
    print(json.dumps(out, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--json", default="")
    ap.add_argument("--bcm", action="store_true", help="the ARD product of experts against single handles and the isotropic BCM")
    ap.add_argument("--variants", default="abc")
    ap.add_argument("--lib", default="", help="--bcm: another libcugp.so to load instead of the tree's")
    ap.add_argument("--trace-csv", default="", help="a rocprofv3 kernel trace of a --bcm run: dispatch times per shape")
    args = ap.parse_args()
    if args.trace_csv:
        return trace_report(args.trace_csv)
    if args.bcm:
        return bcm_probe(args)

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
        Xt = np.ascontiguousarray(X[:1000] * 0.5)    # one prediction each: k_cross<false, 0> / k_cross<true, 0> appear in a kernel trace
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
