"""Timings of the matrix-free exact GP (gp.IterativeGP) on one GPU -> profiles/iter_probe.json.  D = 10, SE and RQ-ARD.
apply at N for t = 1, 16 and 64, one after the other (not interleaved): each the median of --reps calls after one warm-up
call of its own, in seconds and covariance entries per second, host packing and copies included -- the call as a user makes
it.  fit, predict (the mean at --nt points, the variance at the first --ntvar of them) and the 8192-row comparison of
fit's alpha with Covsum.get_alpha() are SINGLE calls without a warm-up: their times include first-use allocations, and
exact_seconds_first_call the exact handle's first evaluation.  Read them as orders of magnitude, with the sweep counts.

    python tools/iter_probe.py [--n 100000] [--reps 3] [--big 0] [--out profiles/iter_probe.json]

--precond r [r ...]: instead of the above, the pivoted-Cholesky preconditioner at each rank r (0: none)
-> profiles/iter_precond_probe.json.  Per family and rank: the build (set_precond + precond_info: factor, Gram product, the
r x r factorisation and Q, with their two host waits; the first call with its allocations, then the median of --reps
rebuilds), one M^-1 V at t = 16 and one K V beside it (medians, host packing included), fit at tol 1e-8 and the variance at
--ntvar points (single calls: sweeps and wall time).  --dims sets D (the length scales stay those of D = 10).

    python tools/iter_probe.py --precond 0 64 256 [--dims 10] [--n 100000]

--grad: instead of the above, the gradient -> profiles/iter_grad_probe.json.  Per family: grad_forms and
apply at t = 16 and t = 64 (tp = 16 | 64), medians of --reps calls after a warm-up call, wall time with the host's packing
(grad_forms packs two blocks, apply one and unpacks one); fit, then loglik_grad with 15 and with 63 Rademacher probes at tol
1e-8: SINGLE calls without a warm-up.  --kernel-stats DIR adds the device times of k_cov_grad* and k_cov_apply* from the
*kernel_stats.csv files a separate `rocprofv3 --kernel-trace --stats -d DIR -- python tools/iter_probe.py --grad --forms-only`
left there (average per launch, the warm-up launch included), as covariance entries per second.

--precision: instead of the above, the mixed mode -> profiles/iter_mixed_probe.json.  Per family:
apply(precision="fp32") beside apply at t = 1, 16 and 64, alternating in one process, medians of --reps calls after a
warm-up call each (wall time with the host's packing); fit at tol 1e-8 in the fp64 and in the mixed mode with solve_stats
(SINGLE calls; the fp64 one pays the first-use allocations).  --applies-only: the products alone, nothing written (for a
kernel trace; --ts 16 64 there, so that the 16-column kernels' averages are those of t = 16); --kernel-stats DIR adds the
device times of k_cov_apply* and their fp64 / fp32 ratios from the *kernel_stats.csv files a separate
`rocprofv3 --kernel-trace --stats -f csv -d DIR -- python tools/iter_probe.py --precision --applies-only --ts 16 64` left
there (-f csv: rocprofv3's default output is a rocpd database, which kernel_stats does not read).

--xgrad: instead of the above, the test-input gradients -> profiles/iter_xgrad_probe.json.  Per family:
input_grad at 64 test points with a weight vector each (one mean-and-variance launch of k_cov_xgrad), input_grad at --nt
points with one weight vector (one mean-only launch) and apply at t = 16 beside them: medians of --reps calls after a warm-up
call, wall time with the host's packing; then fit and predict_grad at 64 points at tol 1e-8 beside predict's variance there
(SINGLE calls).  --launches-only: the three launches alone, nothing written (for a kernel trace, with --reps 12 or more);
--kernel-stats DIR adds the device times of k_cov_xgrad* and k_cov_apply* from such a trace's *kernel_trace.csv: per kernel the
median, smallest and largest of its launches with the FIRST one (the warm-up call's) dropped, and covariance entries per
second from the median -- the common unit: each kernel computes one entry per (i, j).

--paths: instead of the above, the pathwise posterior draws -> profiles/iter_paths_probe.json.  Per
family and feature count m (--features), s = 64 paths: features_apply over the n training rows and over --nt test rows with
apply and apply_cross at t = 64 beside them (medians of --reps calls after a warm-up call, wall time with the host's packing;
feature entries n m and covariance entries n n per second); then fit beside sample_paths (paths_fit: one 64-column solve) at
tol 1e-8 -- SINGLE calls --, and paths(Xt) beside predict's mean at --nt points (medians after a warm-up).  --launches-only:
the products alone, nothing written (for a kernel trace); --kernel-stats DIR adds the device times of k_rff_apply* and
k_cov_apply* from such traces' *kernel_trace.csv, per kernel and launch shape (the grid tells the shapes apart): DIR/m<m>
holds the trace of `... --paths --launches-only --features <m>`, one run per feature count.

--paths-grad: instead of the above, the input gradients of the sample paths ->
profiles/iter_paths_grad_probe.json.  Per family, s = 64 paths over --nt points with m = the first of --features: paths.grad's
data term ("update") and feature term ("prior"), apply_cross at t = 64 (k_cov_apply4's cross product of the same call shape)
and input_grad with ONE weight vector (one k_cov_xgrad launch: a caller without paths.grad needs s of them): medians of
--reps calls after a warm-up call, wall time with the host's packing.  --launches-only: the calls alone, nothing written (for a
kernel trace, with --reps 12); --lib PATH loads another libcugp.so (the parent commit's) and runs what it has.
--kernel-stats DIR adds the device times from the *kernel_trace.csv under DIR/new and DIR/parent (one traced run of
`... --paths-grad --launches-only --reps 12` each, the second with --lib): per kernel the median, smallest and largest of its
launches with the FIRST dropped; the data term's entry rate (nt n entries; every entry is computed once per chunk of four
dimensions) beside k_cov_apply4's, and s times the parent's k_cov_xgrad launch with its finish beside the one new launch.

--varcache: instead of the above, the variance cache -> profiles/iter_varcache_probe.json.  Per family
and rank (--ranks): the build's wall time and predict(var="cached") at --nt points (medians of --reps after a warm-up), the
products taken, and at the first --ntvar points (var_cached - var_exact) / var_exact against predict(var=True).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import synth  # noqa: E402
from cugp_amd import capi, gp  # noqa: E402

D = 10
THETA = {"se": [1.5, 0.0, -1.0], "rq_ard": np.linspace(1.3, 1.7, D).tolist() + [0.4, 0.0, -1.0]}


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), out


def precond_probe(a):
    d = a.dims
    theta = {"se": THETA["se"], "rq_ard": np.linspace(1.3, 1.7, d).tolist() + [0.4, 0.0, -1.0]}
    res = {"build_id": capi.lib().cugp_build_id().decode(), "n": a.n, "d": d, "ntvar": a.ntvar, "reps": a.reps, "tol": 1e-8,
           "families": {}}
    X, y = synth(a.n, d=d)
    Xt = synth(a.ntvar, d=d, seed=7)[0]
    V = np.random.default_rng(0).standard_normal((16, a.n))
    for fam, th in theta.items():
        g = gp.IterativeGP(a.n, d, kernel=fam)
        g.set_data(X, y)
        g.set_loghyper(th)
        res["families"][fam] = {}
        for rank in a.precond:
            def build():
                g.set_precond(rank)
                return g.precond_info()
            t0 = time.perf_counter()
            info = build()
            r = {"info": info, "plan": g.precond_plan(a.n, rank), "build_seconds_first_call": time.perf_counter() - t0}
            r["apply_K_t16_seconds"] = timed(lambda: g.apply(V), a.reps)[0]
            if info["achieved"]:
                r["build_seconds"] = timed(build, a.reps)[0]
                r["apply_Minv_t16_seconds"] = timed(lambda: g.precond_apply(V), a.reps)[0]
            t0 = time.perf_counter()
            fi = g.fit(1e-8, 2000, 10)
            r["fit"] = {"seconds": time.perf_counter() - t0, "sweeps": fi[0], "rel_residual": fi[1], "converged": fi[2]}
            t0 = time.perf_counter()
            pi = g.predict(Xt, True, 1e-8, 2000, 10)[2]
            r["predict_var"] = {"seconds": time.perf_counter() - t0, "sweeps_max": float(pi[:, 0].max()), "converged": float(pi[:, 2].min())}
            print(fam, "rank", rank, r, flush=True)
            res["families"][fam][str(rank)] = r
        g.close()
    res["not_measured"] = ["the build split into factor / Gram / Q (one wall time per build)",
                           "device time of k_pc_project + finish + k_pc_correct without the host's packing and copies"]
    out = a.out if not a.out.endswith("iter_probe.json") else os.path.join(ROOT, "profiles", "iter_precond_probe.json")
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


def kernel_stats(root, n):
    """{kernel: {calls, average_seconds, entries_per_s}} of the k_cov_grad* / k_cov_apply* rows of rocprofv3's kernel statistics"""
    import csv
    import glob
    out = {}
    for path in glob.glob(os.path.join(root, "**", "*kernel_stats.csv"), recursive=True):
        with open(path) as f:
            for row in csv.DictReader(f):
                name = row.get("Name", "")
                if ("k_cov_grad" in name or "k_cov_apply" in name) and "finish" not in name:
                    avg = float(row["AverageNs"]) * 1e-9
                    out[name.replace("cugp::", "").split("(")[0].replace("void ", "")] = {
                        "calls": int(row["Calls"]), "average_seconds": avg, "entries_per_s": float(n) * n / avg}
    return out


def kernel_trace_times(root, entries):
    """{kernel: {timed_launches, median_seconds, min_seconds, max_seconds, entries_per_s}} of the k_cov_xgrad* / k_cov_apply*
    dispatches in rocprofv3's kernel trace, each kernel's FIRST launch (the warm-up call's) dropped; entries: kernel name ->
    the entries one launch computes; entries_per_s from the median"""
    import csv
    import glob
    runs = {}
    for path in glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            for row in csv.DictReader(f):
                name = row.get("Kernel_Name", "")
                if ("k_cov_xgrad" in name or "k_cov_apply" in name) and "finish" not in name:
                    short = name.replace("cugp::", "").split("(")[0].replace("void ", "")
                    runs.setdefault(short, []).append((int(row["Start_Timestamp"]), int(row["End_Timestamp"])))
    out = {}
    for short, r in runs.items():
        secs = [(e - s) * 1e-9 for s, e in sorted(r)[1:]]
        if secs:
            med = float(np.median(secs))
            out[short] = {"timed_launches": len(secs), "median_seconds": med, "min_seconds": min(secs), "max_seconds": max(secs),
                          "entries_per_s": entries(short) / med}
    return out


def grad_probe(a):
    res = {"build_id": capi.lib().cugp_build_id().decode(), "n": a.n, "d": D, "reps": a.reps, "tol": 1e-8, "families": {}}
    X, y = synth(a.n, d=D)
    rng = np.random.default_rng(0)
    for fam, th in THETA.items():
        g = gp.IterativeGP(a.n, D, kernel=fam)
        g.set_data(X, y)
        g.set_loghyper(th)
        r = {"plan": g.plan(a.n, a.n)}
        for t in (16, 64):
            U, V = rng.standard_normal((t, a.n)), rng.standard_normal((t, a.n))
            sg, sa = timed(lambda: g.grad_forms(U, V), a.reps)[0], timed(lambda: g.apply(V), a.reps)[0]
            r["t%d" % t] = {"grad_forms_seconds": sg, "grad_forms_entries_per_s": float(a.n) * a.n / sg, "apply_seconds": sa,
                            "apply_entries_per_s": float(a.n) * a.n / sa}
            print(fam, "t", t, r["t%d" % t], flush=True)
        if not a.forms_only:
            t0 = time.perf_counter()
            fi = g.fit(1e-8, 2000, 10)
            r["fit"] = {"seconds": time.perf_counter() - t0, "sweeps": fi[0], "converged": fi[2]}
            for probes in (15, 63):
                t0 = time.perf_counter()
                gr, info = g.loglik_grad(probes, np.random.default_rng(1), 1e-8, 2000, 10)
                r["loglik_grad_%d" % probes] = {"seconds": time.perf_counter() - t0, "sweeps_max": float(info["solves"][:, 0].max()),
                                                "converged": float(info["solves"][:, 2].min()), "g": gr.tolist()}
            print(fam, {k: v for k, v in r.items() if k.startswith(("fit", "loglik"))}, flush=True)
        g.close()
        res["families"][fam] = r
    if a.kernel_stats:
        res["kernels"] = kernel_stats(a.kernel_stats, a.n)
    res["single_unwarmed_calls"] = ["fit", "loglik_grad_15", "loglik_grad_63"]
    res["not_measured"] = ["counters", "the device time of the probes' solves apart from the forms",
                           "d > 16 (the feature-chunk grid dimension)"]
    if a.forms_only:
        return
    out = a.out if not a.out.endswith("iter_probe.json") else os.path.join(ROOT, "profiles", "iter_grad_probe.json")
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


def precision_probe(a):
    res = {"build_id": capi.lib().cugp_build_id().decode(), "n": a.n, "d": D, "reps": a.reps, "tol": 1e-8, "families": {}}
    X, y = synth(a.n, d=D)
    rng = np.random.default_rng(0)
    for fam, th in THETA.items():
        g = gp.IterativeGP(a.n, D, kernel=fam)
        g.set_data(X, y)
        g.set_loghyper(th)
        r = {"plan": g.plan(a.n, a.n), "apply": {}}
        for t in a.ts:
            V = rng.standard_normal((t, a.n))
            g.apply(V), g.apply(V, precision="fp32")
            t64, t32 = [], []
            for _ in range(a.reps):
                for ts, prec in ((t64, "fp64"), (t32, "fp32")):
                    t0 = time.perf_counter()
                    g.apply(V, precision=prec)
                    ts.append(time.perf_counter() - t0)
            s64, s32 = float(np.median(t64)), float(np.median(t32))
            r["apply"][str(t)] = {"fp64_seconds": s64, "fp32_seconds": s32, "ratio": s64 / s32}
            print(fam, "t", t, r["apply"][str(t)], flush=True)
        if not a.applies_only:
            for mode in ("fp64", "mixed"):
                g.set_precision(mode)
                t0 = time.perf_counter()
                fi = g.fit(1e-8, 4000, 10)
                r["fit_" + mode] = {"seconds": time.perf_counter() - t0, "sweeps": fi[0], "residual": fi[1], "converged": fi[2],
                                    "stats": g.solve_stats()}
                print(fam, mode, r["fit_" + mode], flush=True)
            r["fit_ratio"] = r["fit_fp64"]["seconds"] / r["fit_mixed"]["seconds"]
        g.close()
        res["families"][fam] = r
    if a.applies_only:
        return
    res["not_measured"] = ["counters", "the variance and loglik_grad in the mixed mode", "d > 16", "other families than SE and RQ-ARD",
                           "cycle_drop other than the default"]
    if a.kernel_stats:
        res["kernels"] = ks = kernel_stats(a.kernel_stats, a.n)
        # k_cov_apply32<...> beside k_cov_apply<...> of the same instantiation: device time fp64 / fp32, the warm-up launch included
        twin = {k: k.replace("k_cov_apply4", "k_cov_apply32_4").replace("k_cov_apply<", "k_cov_apply32<") for k in ks if "apply32" not in k}
        res["kernel_ratios"] = {k: ks[k]["average_seconds"] / ks[t]["average_seconds"] for k, t in twin.items() if t in ks}
    else:
        res["not_measured"].insert(0, "device times of the two product kernels (no --kernel-stats): the ratios are wall times "
                                      "with the host's packing and copies")
    out = a.out if not a.out.endswith("iter_probe.json") else os.path.join(ROOT, "profiles", "iter_mixed_probe.json")
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


def xgrad_probe(a):
    res = {"build_id": capi.lib().cugp_build_id().decode(), "n": a.n, "d": D, "nt": a.nt, "reps": a.reps, "tol": 1e-8, "families": {}}
    X, y = synth(a.n, d=D)
    Xt = synth(a.nt, d=D, seed=7)[0]
    rng = np.random.default_rng(0)
    W, V = rng.standard_normal((64, a.n)), rng.standard_normal((16, a.n))
    for fam, th in THETA.items():
        g = gp.IterativeGP(a.n, D, kernel=fam)
        g.set_data(X, y)
        g.set_loghyper(th)
        r = {"plan_var": g.plan(64, a.n), "plan_mean": g.plan(a.nt, a.n), "plan_apply": g.plan(a.n, a.n)}
        for key, fn, ent in (("var_nt64", lambda: g.input_grad(Xt[:64], W), 64.0 * a.n),
                             ("mean_nt%d" % a.nt, lambda: g.input_grad(Xt, W[:1]), float(a.nt) * a.n),
                             ("apply_t16", lambda: g.apply(V), float(a.n) * a.n)):
            sec = timed(fn, a.reps)[0]
            r[key] = {"seconds": sec, "entries_per_s": ent / sec}
        print(fam, r, flush=True)
        if not a.launches_only:
            t0 = time.perf_counter()
            fi = g.fit(1e-8, 2000, 10)
            r["fit"] = {"seconds": time.perf_counter() - t0, "sweeps": fi[0], "converged": fi[2]}
            for key, fn in (("predict_var_nt64", lambda: g.predict(Xt[:64], True, 1e-8, 2000, 10)[2]),
                            ("predict_grad_nt64", lambda: g.predict_grad(Xt[:64], tol=1e-8, max_iter=2000, check_every=10)[4]),
                            ("predict_grad_mean_only_nt%d" % a.nt, lambda: g.predict_grad(Xt, want_var=False, want_var_grad=False)[4])):
                t0 = time.perf_counter()
                info = fn()
                r[key] = {"seconds": time.perf_counter() - t0}
                if info is not None:
                    r[key].update(sweeps_max=float(info[:, 0].max()), converged=float(info[:, 2].min()), stats=g.solve_stats())
            print(fam, {k: v for k, v in r.items() if k.startswith(("fit", "predict"))}, flush=True)
        g.close()
        res["families"][fam] = r
    if a.launches_only:
        return
    if a.kernel_stats:
        # (the trace holds three launch shapes: the kernel's name tells them apart)
        res["kernels"] = kernel_trace_times(a.kernel_stats, lambda k: (float(a.n) * a.n if "apply" in k else 64.0 * a.n
                                                                      if k.endswith("true>") else float(a.nt) * a.n))
    res["single_unwarmed_calls"] = ["fit", "predict_var_nt64", "predict_grad_nt64", "predict_grad_mean_only_nt%d" % a.nt]
    res["not_measured"] = ["counters", "d > 16 (the feature-chunk grid dimension)", "other families than SE and RQ-ARD",
                           "forced splits"] + ([] if a.kernel_stats else ["device times (no --kernel-stats): wall times with the host's packing"])
    out = a.out if not a.out.endswith("iter_probe.json") else os.path.join(ROOT, "profiles", "iter_xgrad_probe.json")
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


def paths_trace_times(root, shapes, m, n):
    """{kernel @ shape: {timed_launches, median_seconds, min_seconds, max_seconds, entries_per_s}} of the k_rff_apply* / k_cov_apply*
    dispatches of a kernel trace; shapes: workgroups of the grid's x dimension (row blocks) -> (label, rows); entries: rows * m
    feature entries, rows * n covariance entries; each shape's first launch (the warm-up call's) dropped"""
    import csv
    import glob
    runs = {}
    for path in glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            for row in csv.DictReader(f):
                name = row.get("Kernel_Name", "")
                blocks = int(row["Grid_Size_X"]) // int(row["Workgroup_Size_X"])
                if ("k_rff_apply" in name or "k_cov_apply" in name) and "finish" not in name and blocks in shapes:
                    short = name.replace("cugp::", "").split("(")[0].replace("void ", "")
                    runs.setdefault((short, blocks, int(row["Grid_Size_Y"])), []).append((int(row["Start_Timestamp"]), int(row["End_Timestamp"])))
    out = {}
    for (short, blocks, split), r in sorted(runs.items()):
        secs = [(e - s) * 1e-9 for s, e in sorted(r)[1:]]
        if secs:
            med = float(np.median(secs))
            out["%s @ %s, split %d" % (short, shapes[blocks][0], split)] = {
                "timed_launches": len(secs), "median_seconds": med, "min_seconds": min(secs), "max_seconds": max(secs),
                "entries_per_s": float(shapes[blocks][1]) * (m if "rff" in short else n) / med}
    return out


def paths_probe(a):
    res = {"build_id": capi.lib().cugp_build_id().decode(), "n": a.n, "d": D, "nt": a.nt, "s": 64, "reps": a.reps, "tol": 1e-8,
           "families": {}}
    X, y = synth(a.n, d=D)
    Xt = synth(a.nt, d=D, seed=7)[0]
    rng = np.random.default_rng(0)
    V = rng.standard_normal((64, a.n))
    for fam, th in THETA.items():
        g = gp.IterativeGP(a.n, D, kernel=fam)
        g.set_data(X, y)
        g.set_loghyper(th)
        r = {"apply_t64_seconds": timed(lambda: g.apply(V), a.reps)[0], "apply_cross_t64_seconds": timed(lambda: g.apply_cross(Xt, V), a.reps)[0]}
        r["apply_t64_entries_per_s"] = float(a.n) * a.n / r["apply_t64_seconds"]
        draws = {}
        for m in a.features:
            Om = gp.spectral_frequencies(fam, D, m, rng, np.exp(th[-3]) if fam.startswith("rq") else None)
            draws[m] = (Om, rng.uniform(0, 2 * np.pi, m), rng.standard_normal((64, m)))
            st = timed(lambda: g.features_apply(None, *draws[m], g._origin), a.reps)[0]
            sq = timed(lambda: g.features_apply(Xt, *draws[m], g._origin), a.reps)[0]
            r["m%d" % m] = {"features_train_seconds": st, "features_train_entries_per_s": float(a.n) * m / st,
                            "features_test_seconds": sq, "features_test_entries_per_s": float(a.nt) * m / sq}
            print(fam, "m", m, r["m%d" % m], flush=True)
        if not a.launches_only:
            t0 = time.perf_counter()
            fi = g.fit(1e-8, 2000, 10)
            r["fit"] = {"seconds": time.perf_counter() - t0, "sweeps": fi[0], "converged": fi[2]}
            r["predict_mean_seconds"] = timed(lambda: g.predict(Xt, var=False), a.reps)[0]
            Eps = rng.standard_normal((64, a.n))
            for m in a.features:
                t0 = time.perf_counter()
                paths = g.sample_paths(64, Omega=draws[m][0], b=draws[m][1], W=draws[m][2], Eps=Eps, tol=1e-8, max_iter=2000, check_every=10)
                r["m%d" % m]["paths_fit"] = {"seconds": time.perf_counter() - t0, "sweeps_max": float(paths.info[:, 0].max()),
                                             "converged": float(paths.info[:, 2].min()), "stats": g.solve_stats()}
                r["m%d" % m]["paths_eval_seconds"] = timed(lambda: paths(Xt), a.reps)[0]
                print(fam, "m", m, r["m%d" % m]["paths_fit"], r["m%d" % m]["paths_eval_seconds"], flush=True)
            print(fam, r["fit"], r["predict_mean_seconds"], flush=True)
        g.close()
        res["families"][fam] = r
    if a.launches_only:
        return
    if a.kernel_stats:
        shapes = {(a.n + 63) // 64: ("%d training rows" % a.n, a.n), (a.nt + 63) // 64: ("%d test rows" % a.nt, a.nt)}
        res["kernels"] = {"m%d" % m: paths_trace_times(os.path.join(a.kernel_stats, "m%d" % m), shapes, m, a.n) for m in a.features}
    res["single_unwarmed_calls"] = ["fit", "paths_fit"]
    res["not_measured"] = ["counters", "d > 16 (the feature chunk loop)", "other families than SE and RQ-ARD", "forced splits",
                           "s other than 64"] + ([] if a.kernel_stats else ["device times (no --kernel-stats): wall times with the host's packing"])
    out = a.out if not a.out.endswith("iter_probe.json") else os.path.join(ROOT, "profiles", "iter_paths_probe.json")
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


def grad_trace_times(root):
    """{kernel: {timed_launches, median_seconds, min_seconds, max_seconds}} of the gradient kernels and k_cov_apply4 in a kernel
    trace, each kernel's first launch dropped"""
    import csv
    import glob
    runs = {}
    for path in glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            for row in csv.DictReader(f):
                name = row.get("Kernel_Name", "")
                if any(k in name for k in ("k_cov_xgrad", "k_rff_grad", "k_paths_grad_finish", "k_cov_apply4")):
                    short = name.replace("cugp::", "").split("(")[0].replace("void ", "")
                    runs.setdefault(short, []).append((int(row["Start_Timestamp"]), int(row["End_Timestamp"])))
    out = {}
    for short, r in sorted(runs.items()):
        secs = [(e - s) * 1e-9 for s, e in sorted(r)[1:]]
        if secs:
            out[short] = {"timed_launches": len(secs), "median_seconds": float(np.median(secs)), "min_seconds": min(secs),
                          "max_seconds": max(secs)}
    return out


def paths_grad_probe(a):
    new, m = "cugp_iter_paths_grad" in capi.SIGNATURES, a.features[0]
    res = {"build_id": capi.lib().cugp_build_id().decode(), "n": a.n, "d": D, "nt": a.nt, "s": 64, "m": m, "reps": a.reps, "families": {}}
    X, y = synth(a.n, d=D)
    Xt = synth(a.nt, d=D, seed=7)[0]
    rng = np.random.default_rng(0)
    V = rng.standard_normal((64, a.n))
    for fam, th in THETA.items():
        g = gp.IterativeGP(a.n, D, kernel=fam)
        g.set_data(X, y)
        g.set_loghyper(th)
        Om = gp.spectral_frequencies(fam, D, m, rng, np.exp(th[-3]) if fam.startswith("rq") else None)
        r = {"apply_cross_t64_seconds": timed(lambda: g.apply_cross(Xt, V), a.reps)[0],
             "input_grad_one_vector_seconds": timed(lambda: g.input_grad(Xt, V[:1]), a.reps)[0]}
        if new:
            paths = gp.SamplePaths(g, Om, rng.uniform(0, 2 * np.pi, m), rng.standard_normal((64, m)), V, g._origin, None)
            r["grad_update_seconds"] = timed(lambda: paths.grad(Xt, "update"), a.reps)[0]
            r["grad_prior_seconds"] = timed(lambda: paths.grad(Xt, "prior"), a.reps)[0]
        print(fam, r, flush=True)
        g.close()
        res["families"][fam] = r
    if a.launches_only:
        return
    if a.kernel_stats:
        k = {w: grad_trace_times(os.path.join(a.kernel_stats, w)) for w in ("new", "parent")}
        res["kernels"] = k
        res["data_term"] = {}
        for fam, tag in (("se", "<false, 0>"), ("rq_ard", "<true, 3>")):
            cols, app = k["new"].get("k_cov_xgrad_cols4" + tag), k["new"].get("k_cov_apply4" + tag)
            one, fin = k["parent"].get("k_cov_xgrad" + tag[:-1] + ", false>"), k["parent"].get("k_cov_xgrad_finish")
            if cols and app and one and fin:
                route = 64 * (one["median_seconds"] + fin["median_seconds"])
                res["data_term"][fam] = {
                    "entries_per_s": float(a.nt) * a.n / cols["median_seconds"], "cov_apply4_entries_per_s": float(a.nt) * a.n / app["median_seconds"],
                    "seconds": cols["median_seconds"], "cov_apply4_seconds": app["median_seconds"],
                    "s_launches_of_k_cov_xgrad_seconds": route, "s_launches_over_one_launch": route / cols["median_seconds"]}
    res["not_measured"] = ["counters", "d > 16 at scale (the chunk loop)", "other families than SE and RQ-ARD", "forced splits",
                           "s other than 64", "k_paths_grad_finish per call kind (one median over both)"] + (
                               [] if a.kernel_stats else ["device times (no --kernel-stats): wall times with the host's packing"])
    out = a.out if not a.out.endswith("iter_probe.json") else os.path.join(ROOT, "profiles", "iter_paths_grad_probe.json")
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


def varcache_probe(a):
    """--varcache: the variance cache -> profiles/iter_varcache_probe.json.  Per family and rank: the
    build's wall time (median of --reps after a warm-up), products taken, predict(var="cached") at --nt points (the same), and
    at the first --ntvar points the exact variance of predict(var=True) (one unwarmed call per family) beside the cached one:
    the largest and the median (var_cached - var_exact) / var_exact."""
    res = {"build_id": capi.lib().cugp_build_id().decode(), "n": a.n, "d": D, "nt": a.nt, "ntvar": a.ntvar, "reps": a.reps,
           "tol": 1e-8, "families": {}}
    X, y = synth(a.n, d=D)
    Xt = synth(a.nt, d=D, seed=7)[0]
    for fam, th in THETA.items():
        g = gp.IterativeGP(a.n, D, kernel=fam)
        g.set_data(X, y)
        g.set_loghyper(th)
        g.fit(1e-8, 2000, 10)
        t0 = time.perf_counter()
        exact = g.predict(Xt[:a.ntvar], True, 1e-8, 2000, 10)[1]
        r = {"exact_var_seconds": time.perf_counter() - t0, "ranks": {}}
        for rank in a.ranks:
            sec, info = timed(lambda: g.variance_cache(rank, rng=np.random.default_rng(0)), a.reps)
            psec, out = timed(lambda: g.predict(Xt, var="cached"), a.reps)
            rel = (out[1][:a.ntvar] - exact) / exact
            r["ranks"][rank] = {"build_seconds": sec, "info": info, "predict_cached_seconds": psec, "rel_excess_max": float(rel.max()),
                                "rel_excess_median": float(np.median(rel)), "rel_excess_min": float(rel.min())}
            print(fam, rank, r["ranks"][rank], flush=True)
        g.close()
        res["families"][fam] = r
    res["not_measured"] = ["device times of k_cov_var (no kernel trace)", "the 16-tile width of k_cov_var (not built)",
                           "k_cov_var against four apply_cross launches", "other families than SE and RQ-ARD", "nt = 1e5"]
    out = a.out if not a.out.endswith("iter_probe.json") else os.path.join(ROOT, "profiles", "iter_varcache_probe.json")
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--varcache", action="store_true", help="the variance cache's probe (its own mode)")
    ap.add_argument("--ranks", type=int, nargs="+", default=[64, 256, 512], help="... the cache's ranks")
    ap.add_argument("--paths-grad", action="store_true", help="the sample paths' input gradients (its own mode)")
    ap.add_argument("--lib", default="", help="... another libcugp.so to load instead of the tree's (the parent commit's)")
    ap.add_argument("--paths", action="store_true", help="the pathwise draws' probe (its own mode)")
    ap.add_argument("--features", type=int, nargs="+", default=[1024, 4096], help="... feature counts m")
    ap.add_argument("--xgrad", action="store_true", help="the test-input gradients' probe (its own mode)")
    ap.add_argument("--launches-only", action="store_true", help="... the three launches alone, nothing written (for a kernel trace)")
    ap.add_argument("--precision", action="store_true", help="the mixed-mode probe (its own mode)")
    ap.add_argument("--applies-only", action="store_true", help="... the products alone, nothing written (for a kernel trace)")
    ap.add_argument("--ts", type=int, nargs="+", default=[1, 16, 64], help="... the products' column counts")
    ap.add_argument("--grad", action="store_true", help="the gradient probe (its own mode)")
    ap.add_argument("--forms-only", action="store_true", help="... grad_forms and apply alone, nothing written (for a kernel trace)")
    ap.add_argument("--kernel-stats", default=None, help="... a directory with rocprofv3's kernel statistics of such a run")
    ap.add_argument("--precond", type=int, nargs="+", default=None, help="ranks of the preconditioner probe (its own mode)")
    ap.add_argument("--dims", type=int, default=D, help="input dimension of the preconditioner probe")
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--big", type=int, default=0, help="one apply (t = 16, SE) at this many rows, e.g. 1000000")
    ap.add_argument("--nt", type=int, default=1000, help="test points of the predictions")
    ap.add_argument("--ntvar", type=int, default=64, help="... of which the first ntvar get a variance (64 share one solve)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "iter_probe.json"))
    a = ap.parse_args()
    if a.lib:                                          # another build: bind what it has
        import ctypes
        capi.LIB_PATH = os.path.abspath(a.lib)
        capi._share_torch_hip_runtime()
        other = ctypes.CDLL(capi.LIB_PATH)
        capi.SIGNATURES = {k: v for k, v in capi.SIGNATURES.items() if hasattr(other, k)}
    if a.varcache:
        return varcache_probe(a)
    if a.paths_grad:
        return paths_grad_probe(a)
    if a.precond is not None:
        return precond_probe(a)
    if a.grad:
        return grad_probe(a)
    if a.precision:
        return precision_probe(a)
    if a.xgrad:
        return xgrad_probe(a)
    if a.paths:
        return paths_probe(a)
    res = {"build_id": capi.lib().cugp_build_id().decode(), "n": a.n, "nt": a.nt, "ntvar": a.ntvar, "d": D, "reps": a.reps, "families": {}}
    X, y = synth(a.n, d=D)
    Xt = synth(a.nt, d=D, seed=7)[0]
    rng = np.random.default_rng(0)
    for fam, th in THETA.items():
        g = gp.IterativeGP(a.n, D, kernel=fam)
        g.set_data(X, y)
        g.set_loghyper(th)
        r = {"plan": g.plan(a.n, a.n), "apply": {}}
        for t in (1, 16, 64):
            V = rng.standard_normal((t, a.n))
            s, _ = timed(lambda: g.apply(V), a.reps)
            r["apply"][str(t)] = {"seconds": s, "entries_per_s": float(a.n) * a.n / s}
            print(fam, "apply t", t, r["apply"][str(t)], flush=True)
        t0 = time.perf_counter()
        info = g.fit(1e-8, 1000, 10)
        r["fit"] = {"seconds": time.perf_counter() - t0, "sweeps": info[0], "rel_residual": info[1], "converged": info[2]}
        print(fam, "fit", r["fit"], flush=True)
        t0 = time.perf_counter()
        g.predict(Xt, var=False)
        r["predict_mean"] = {"seconds": time.perf_counter() - t0}
        t0 = time.perf_counter()
        _, _, pi = g.predict(Xt[:a.ntvar], True, 1e-8, 1000, 10)
        r["predict_var"] = {"seconds": time.perf_counter() - t0, "sweeps_max": float(pi[:, 0].max()),
                                 "converged": float(pi[:, 2].min())}
        print(fam, "predict", r["predict_mean"], r["predict_var"], flush=True)
        g.close()
        res["families"][fam] = r
    n8 = 8192
    X8, y8 = synth(n8, d=D)
    c = gp.Covsum(n8, D)
    c.set_loghyperparam(THETA["se"])
    t0 = time.perf_counter()
    c.loglik_grad(X8, y8)
    a8 = c.get_alpha()
    exact_s = time.perf_counter() - t0
    g = gp.IterativeGP(n8, D, kernel="se")
    g.set_data(X8, y8)
    g.set_loghyper(THETA["se"])
    t0 = time.perf_counter()
    info = g.fit(1e-10, 1000, 10)
    res["n8192"] = {"fit_seconds": time.perf_counter() - t0, "exact_seconds_first_call": exact_s, "sweeps": info[0],
                    "alpha_max_abs_diff": float(np.max(np.abs(g.alpha() - a8))), "alpha_max_abs": float(np.max(np.abs(a8)))}
    if a.big:
        Xb, yb = synth(a.big, d=D)
        g = gp.IterativeGP(a.big, D, kernel="se")
        g.set_data(Xb, yb)
        g.set_loghyper(THETA["se"])
        V = rng.standard_normal((16, a.big))
        t0 = time.perf_counter()
        g.apply(V)
        s = time.perf_counter() - t0
        res["big"] = {"n": a.big, "t": 16, "seconds_first_call": s, "entries_per_s": float(a.big) ** 2 / s}
    res["not_measured"] = ["k_build / k_cross entries per second at 8192 rows (kernel time alone)", "device time without the host's packing"]
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
