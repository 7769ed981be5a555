"""The combination rules against today's product-of-experts prediction on one GPU: milliseconds per call at 16 x 1500 and
4 x 6000 rows, D = 10, 1000 test points, a world of one (a communicator without id), interleaved call by call in one
process after two warm-up rounds:

    base   cugp_bcm_predict_allgather (noisy rows, k_poe_reduce) -- what every library has
    poe / gpoe / bcm / rbcm   cugp_bcm_predict_allgather_mode (latent rows, k_poe_reduce_mode) -- where the library has it

    python tools/poe_modes_probe.py [--reps 20] [--json out.json] [--lib other/libcugp.so]

--alternate PARENT_LIB [--rounds 3]: the comparison with the parent commit's library in ALTERNATING fresh processes (parent,
this build, parent, ...), one JSON document with, per round and shape,
    (a) the parent's base call, (b) this build's base call, (c) this build's call in each mode
and the two conditions of DESIGN.md section 17:  (b) - (a) within (a)'s own max - min spread of the same round;
(c) - (a) at most the difference of the two reduce kernels' dispatch times (--reduce-diff-us, from the profiler run below)
plus that spread.

The reduce kernels' own dispatch times come from one profiler run of this probe, no counters (a run of its own, the
program after the double dash), and --kernel-stats turns its statistics file into the two lines kept under profiles/:

    rocprofv3 --kernel-trace --stats --output-format csv -d out -- python tools/poe_modes_probe.py --reps 3
    python tools/poe_modes_probe.py --kernel-stats out/.../..._kernel_stats.csv
"""
import argparse
import csv
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

SHAPES = ((16, 1500), (4, 6000))
D = 10
NT = 1000
MODES = ("poe", "gpoe", "bcm", "rbcm")


def stats(t):
    return {"median_ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4),
            "spread_ms": round(max(t) - min(t), 4)}


def probe(args):
    from cugp_amd import capi
    if args.lib:                                     # another build: bind what it has (the parent lacks the mode calls)
        import ctypes
        capi.LIB_PATH = os.path.abspath(args.lib)
        capi._share_torch_hip_runtime()
        other = ctypes.CDLL(capi.LIB_PATH)
        capi.SIGNATURES = {k: v for k, v in capi.SIGNATURES.items() if hasattr(other, k)}
    import cugp_amd.gp as gp
    from conftest import synth
    modes = MODES if "cugp_bcm_predict_allgather_mode" in capi.SIGNATURES else ()
    hp = [float(np.log(3.0)), 0.0, float(np.log(0.1))]
    out = {"reps": args.reps, "build_id": capi.lib().cugp_build_id().decode(), "d": D, "nt": NT, "shapes": []}
    for K, n in SHAPES:
        X, y = synth(K * n, D, seed=15618)
        Xt = np.ascontiguousarray(synth(NT, D, seed=7)[0])
        b = gp.BCM.split(X, y, K)
        b.set_BCM_log_hyperparam(hp)
        b.loglik_grad()                              # the experts up to date: the calls below are predictions alone
        comm = gp.Comm(None, 0, 1, 0)
        sf2, sn2 = gp.prior_scalars(hp) if modes else (0.0, 0.0)
        run = {"base": lambda: comm.predict_allgather(b, K, K, Xt)}
        for mode in modes:
            run[mode] = lambda mode=mode: comm.predict_allgather(b, K, K, Xt, combine=mode, with_noise=True, sf2=sf2, sn2=sn2)
        t, last = {v: [] for v in run}, {}
        for i in range(2 + args.reps):               # two warm-up rounds (allocations), then the timed ones
            for v, fn in run.items():
                t0 = time.perf_counter()
                last[v] = fn()
                if i >= 2:
                    t[v].append((time.perf_counter() - t0) * 1e3)
        row = {"experts": K, "rows": n}
        row.update({v: stats(t[v]) for v in t})
        row["var0"] = {v: float(last[v][1][0]).hex() for v in last}
        out["shapes"].append(row)
        print(json.dumps(row), file=sys.stderr)
        comm.close()
        b.close()
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


def alternate(args):
    """Parent and this build in alternating fresh processes; the conditions per round and shape."""
    rounds = []
    for r in range(args.rounds):
        docs = {}
        for who, lib in (("parent", args.alternate), ("this", "")):
            cmd = [sys.executable, os.path.abspath(__file__), "--reps", str(args.reps)] + (["--lib", lib] if lib else [])
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                print(p.stderr[-3000:], file=sys.stderr)
                raise SystemExit("the %s run of round %d failed (%d)" % (who, r, p.returncode))
            docs[who] = json.loads(p.stdout.strip().splitlines()[-1])
        shapes = []
        for sa, sb in zip(docs["parent"]["shapes"], docs["this"]["shapes"]):
            a, b = sa["base"], sb["base"]
            row = {"experts": sa["experts"], "rows": sa["rows"], "a_parent_base": a, "b_this_base": b,
                   "b_minus_a_ms": round(b["median_ms"] - a["median_ms"], 4),
                   "b_within_a_spread": abs(b["median_ms"] - a["median_ms"]) <= a["spread_ms"], "c": {}}
            for mode in MODES:
                if mode in sb:
                    diff = sb[mode]["median_ms"] - a["median_ms"]
                    row["c"][mode] = dict(sb[mode], minus_a_ms=round(diff, 4),
                                          within=diff <= args.reduce_diff_us * 1e-3 + a["spread_ms"])
            shapes.append(row)
            print(json.dumps(row), file=sys.stderr)
        rounds.append({"round": r, "parent_build_id": docs["parent"]["build_id"], "build_id": docs["this"]["build_id"],
                       "shapes": shapes})
    out = {"reps": args.reps, "d": D, "nt": NT, "reduce_diff_us": args.reduce_diff_us, "rounds": rounds}
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


def kernel_stats(path):
    """The two reduce kernels' rows of a rocprofv3 --stats kernel statistics file."""
    for r in csv.DictReader(open(path)):
        name = r.get("Name", "")
        if "k_poe_reduce" in name:
            print("%-60s calls %6s  total %12s ns  average %10s ns  min %8s  max %8s" % (
                name[:60], r.get("Calls"), r.get("TotalDurationNs"), r.get("AverageNs"), r.get("MinNs"), r.get("MaxNs")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default="")
    ap.add_argument("--lib", default="", help="another libcugp.so to load instead of the tree's")
    ap.add_argument("--alternate", default="", help="the parent commit's libcugp.so: alternate it with this build")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reduce-diff-us", type=float, default=0.0,
                    help="--alternate: dispatch time of k_poe_reduce_mode minus k_poe_reduce, from the profiler run")
    ap.add_argument("--kernel-stats", default="", help="a rocprofv3 --stats kernel statistics csv: the reduce kernels' rows")
    args = ap.parse_args()
    if args.kernel_stats:
        return kernel_stats(args.kernel_stats)
    if args.alternate:
        return alternate(args)
    return probe(args)


if __name__ == "__main__":
    main()
