"""The input gradients of a product of experts on one GPU: milliseconds per call of cugp_bcm_predict_grad at 16 x 1500 rows,
D = 10, for nt = 1, 64 and 1000 test points -- medians of --reps (20) calls with a host clock around the C call, after two
warm-up calls (allocations), the experts up to date:

    single   cugp_bcm_predict_grad (one process; this build: one group of batched launches per device set)
    comm     cugp_bcm_predict_grad_allgather through a world-of-one communicator without id (where the library has it)

    python tools/bcm_predict_grad_probe.py [--reps 20] [--json out.json] [--lib other/libcugp.so]

--alternate PARENT_LIB [--rounds 3]: the comparison with the parent commit's library in ALTERNATING fresh processes (parent,
this build, parent, ...), one JSON document with per nt the medians of every round and the two conditions of the DESIGN
section: with spread = max - min of the PARENT's medians across the rounds,
    (1) this build's single median (the median of its rounds' medians) <= the parent's + spread   (asserted at nt = 1, 1000)
    (2) this build's comm median <= this build's single median + spread

--kernel-stats FILE: the rows of k_predict_grad_batched in a rocprofv3 --kernel-trace --stats statistics csv (a run of its
own, no counters, the program after the double dash), with the bytes the launch moves by its shapes (--nt of that run) and
their share of the HBM peak (--hbm-gbs):

    rocprofv3 --kernel-trace --stats --output-format csv -d out -- python tools/bcm_predict_grad_probe.py --reps 3 --nts 1000
    python tools/bcm_predict_grad_probe.py --kernel-stats out/.../..._kernel_stats.csv --nt 1000
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

K, N, D = 16, 1500, 10
NTS = (1, 64, 1000)
MODE = 3                                             # CUGP_COMBINE_RBCM: the rule with the most host arithmetic


def stats(t):
    return {"median_ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4)}


def grad_bytes(nt, want_var=True):
    """Bytes one k_predict_grad_batched launch moves, from its shapes (SE: G from Ks): per expert and 64 x 64 tile the Ks
    tile and (dvar) the V tile, the tile's X and Xt rows, alpha, and the partial sums it writes."""
    tiles_t, tiles_i = -(-nt // 64), -(-N // 64)
    per_tile = 64 * 64 * 8 * (2 if want_var else 1) + 2 * 64 * D * 8 + 64 * 8 + 64 * D * 8 * (2 if want_var else 1)
    return K * tiles_t * tiles_i * per_tile


def probe(args):
    import ctypes
    from cugp_amd import capi
    if args.lib:                                     # another build: bind what it has (the parent lacks the new calls)
        capi.LIB_PATH = os.path.abspath(args.lib)
        capi._share_torch_hip_runtime()
        other = ctypes.CDLL(capi.LIB_PATH)
        capi.SIGNATURES = {k: v for k, v in capi.SIGNATURES.items() if hasattr(other, k)}
    import cugp_amd.gp as gp
    from cugp_amd.capi import ptr
    from conftest import synth
    L = capi.lib()
    has_comm = "cugp_bcm_predict_grad_allgather" in capi.SIGNATURES
    hp = [float(np.log(3.0)), 0.0, float(np.log(0.1))]
    X, y = synth(K * N, D, seed=15618)
    b = gp.BCM.split(X, y, K)
    b.set_BCM_log_hyperparam(hp)
    b.loglik_grad()                                  # the experts up to date: the calls below are predictions alone
    comm = gp.Comm(None, 0, 1, 0)
    sf2, sn2 = gp.prior_scalars(hp)
    out = {"reps": args.reps, "build_id": L.cugp_build_id().decode(), "experts": K, "rows": N, "d": D, "mode": MODE, "nts": []}
    for nt in args.nts:
        Xt = np.ascontiguousarray(synth(nt, D, seed=7)[0])
        m, v, dm, dv = np.empty(nt), np.empty(nt), np.empty((nt, D)), np.empty((nt, D))
        run = {"single": lambda: L.cugp_bcm_predict_grad(b._h, ptr(Xt), nt, MODE, 1, ptr(m), ptr(v), ptr(dm), ptr(dv))}
        if has_comm:
            run["comm"] = lambda: L.cugp_bcm_predict_grad_allgather(b._h, comm._h, K, K, ptr(Xt), nt, D, MODE, 1, sf2, sn2,
                                                                    ptr(m), ptr(v), ptr(dm), ptr(dv))
        t = {w: [] for w in run}
        for i in range(2 + args.reps):
            for w, fn in run.items():
                t0 = time.perf_counter()
                rc = fn()
                dt = (time.perf_counter() - t0) * 1e3
                if rc != 0:
                    raise SystemExit("%s failed (%d): %s" % (w, rc, L.cugp_last_error().decode()))
                if i >= 2:
                    t[w].append(dt)
        row = {"nt": nt, "dmean00": float(dm[0, 0]).hex()}
        row.update({w: stats(t[w]) for w in t})
        if "cugp_bcm_predict_grad_form" in capi.SIGNATURES:
            row["form"] = b.predict_grad_form
        out["nts"].append(row)
        print(json.dumps(row), file=sys.stderr)
    comm.close()
    b.close()
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


def alternate(args):
    """Parent and this build in alternating fresh processes; the two conditions per nt."""
    docs = {"parent": [], "this": []}
    for r in range(args.rounds):
        for who, lib in (("parent", args.alternate), ("this", "")):
            cmd = [sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--nts"] + [str(n) for n in args.nts] + \
                  (["--lib", lib] if lib else [])
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                print(p.stderr[-3000:], file=sys.stderr)
                raise SystemExit("the %s run of round %d failed (%d)" % (who, r, p.returncode))
            docs[who].append(json.loads(p.stdout.strip().splitlines()[-1]))
    rows, ok = [], True
    for i, nt in enumerate(args.nts):
        pa = [d["nts"][i]["single"]["median_ms"] for d in docs["parent"]]
        ts = [d["nts"][i]["single"]["median_ms"] for d in docs["this"]]
        tc = [d["nts"][i]["comm"]["median_ms"] for d in docs["this"]]
        spread = max(pa) - min(pa)
        a, s, c = statistics.median(pa), statistics.median(ts), statistics.median(tc)
        row = {"nt": nt, "parent_single_medians_ms": pa, "this_single_medians_ms": ts, "this_comm_medians_ms": tc,
               "parent_spread_ms": round(spread, 4), "parent_ms": round(a, 4), "this_single_ms": round(s, 4),
               "this_comm_ms": round(c, 4), "gain": round(a / s, 3),
               "single_within": s <= a + spread, "comm_within": c <= s + spread,
               "same_bits_as_parent": docs["parent"][0]["nts"][i]["dmean00"] == docs["this"][0]["nts"][i]["dmean00"],
               "form": docs["this"][0]["nts"][i].get("form")}
        ok = ok and row["single_within"] and row["comm_within"]
        rows.append(row)
        print(json.dumps(row), file=sys.stderr)
    out = {"reps": args.reps, "rounds": args.rounds, "experts": K, "rows": N, "d": D, "mode": MODE,
           "parent_build_id": docs["parent"][0]["build_id"], "build_id": docs["this"][0]["build_id"], "nts": rows,
           "conditions_hold": ok}
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    return 0 if ok else 1


def kernel_stats(args):
    """k_predict_grad_batched's rows of a rocprofv3 --stats kernel statistics file, with bytes / time against the HBM peak."""
    nbytes = grad_bytes(args.nt)
    for r in csv.DictReader(open(args.kernel_stats)):
        name = r.get("Name", "")
        if "k_predict_grad_batched" in name:
            avg = float(r.get("AverageNs") or 0)
            gbs = nbytes / avg if avg else 0.0
            print("%-48s calls %6s  average %10.0f ns  %d bytes by shape (nt %d)  %.0f GB/s = %.1f %% of %.0f GB/s" % (
                name[:48], r.get("Calls"), avg, nbytes, args.nt, gbs, 100.0 * gbs / args.hbm_gbs, args.hbm_gbs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--nts", type=int, nargs="+", default=list(NTS))
    ap.add_argument("--json", default="")
    ap.add_argument("--lib", default="", help="another libcugp.so to load instead of the tree's")
    ap.add_argument("--alternate", default="", help="the parent commit's libcugp.so: alternate it with this build")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--kernel-stats", default="", help="a rocprofv3 --stats kernel statistics csv")
    ap.add_argument("--nt", type=int, default=1000, help="--kernel-stats: the test points of the profiled run")
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="--kernel-stats: the HBM peak (MI355X: 8 TB/s)")
    args = ap.parse_args()
    if args.kernel_stats:
        return kernel_stats(args)
    if args.alternate:
        return alternate(args)
    return probe(args)


if __name__ == "__main__":
    sys.exit(main())
