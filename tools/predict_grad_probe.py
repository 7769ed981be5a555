"""Gradients of the prediction with respect to the test inputs (cugp_predict_grad) on one GPU: milliseconds per call
against the marginal prediction and against the finite-difference loop it replaces, the tile pass against HBM bandwidth
and the second triangular product against the fp64 MFMA peak.  Models: N = 8192 rows, D = 10 (bench.py's) and N = 1500;
nt in {100, 1000, 6200} test points.

Per (model, nt), medians over --reps calls, the variants interleaved call by call, the handle's inverse already valid:
  predict_ms           cugp_predict (mean + marginal variance)
  grad_ms              cugp_predict_grad with dmean and dvar (a second triangular product V = W L^-1 per pass)
  grad_mean_only_ms    cugp_predict_grad with dvar = NULL (no second product)
  fd_ms                2 d calls of cugp_predict at x* +- h e_c: what a caller without the analytic gradient pays
Then, at profiling level 4 (every timed launch by its own dispatch events), per call of each form:
  k_predict_grad       kind 13: ms per launch, the bytes it must read (Ks and, with dvar, V: nt x npad x 8 each) over that,
                       as a share of the part's HBM bandwidth (8 TB/s)
  v_product            kind 9 with dvar minus kind 9 without: k_targets_alpha's ms and its algorithmic flop (cpad npad^2)
                       over that, as a share of the fp64 MFMA peak (78.6 TF/s, bench.py's)

    python tools/predict_grad_probe.py [--reps 10] [--json out.json]
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

MODELS = ((8192, 10), (1500, 10))
NTS = (100, 1000, 6200)
KIND_PREDICT, KIND_PGRAD = 9, 13
PEAK_FP64_MFMA = 78.6      # TF/s, MI355X (as bench.py)
PEAK_HBM = 8.0             # TB/s, MI355X
FD_STEP = 1e-6


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

    L = capi.lib()
    P = capi.ptr
    hp = np.array([np.log(3.0), 0.0, np.log(0.1)])
    out = {"peak_fp64_mfma_tflops": PEAK_FP64_MFMA, "peak_hbm_tbs": PEAK_HBM, "reps": args.reps,
           "build_id": L.cugp_build_id().decode(), "cases": []}
    for n, d in MODELS:
        X, y = synth(n, d, seed=15618)
        g = gp.Covsum(n, d, 0)
        g.set_data(X, y)
        g.set_loghyperparam(hp)
        g.loglik_grad()
        for nt in NTS:
            Xt = np.ascontiguousarray(np.random.default_rng(nt).uniform(-10, 10, (nt, d)))
            shifted = []
            for c in range(d):
                for sgn in (1.0, -1.0):
                    Z = Xt.copy()
                    Z[:, c] += sgn * FD_STEP
                    shifted.append(Z)
            m, var, dm, dv = np.empty(nt), np.empty(nt), np.empty((nt, d)), np.empty((nt, d))

            def fd():
                for Z in shifted:
                    capi.check(L.cugp_predict(g.handle, P(Z), nt, P(m), P(var)))
            calls = {
                "predict_ms": lambda: capi.check(L.cugp_predict(g.handle, P(Xt), nt, P(m), P(var))),
                "grad_ms": lambda: capi.check(L.cugp_predict_grad(g.handle, P(Xt), nt, 1, P(m), P(var), P(dm), P(dv))),
                "grad_mean_only_ms": lambda: capi.check(L.cugp_predict_grad(g.handle, P(Xt), nt, 1, P(m), P(var), P(dm), None)),
                "fd_ms": fd,
            }
            for fn in calls.values():            # warm-up: every shape, scratch allocated
                fn()
            res = {k: [] for k in calls}
            for _ in range(args.reps):
                for k, fn in calls.items():
                    res[k].append(timed(fn))
            row = {"n": n, "d": d, "nt": nt}
            row.update({k: round(statistics.median(v), 4) for k, v in res.items()})
            # the launches alone, each timed by its own dispatch events
            g.set_profiling(4)
            prof = {}
            for form in ("grad_ms", "grad_mean_only_ms"):
                for kind in (KIND_PREDICT, KIND_PGRAD):
                    g.kernel_stats(reset=True, kind=kind)
                for _ in range(args.reps):
                    calls[form]()
                prof[form] = {kind: g.kernel_stats(reset=True, kind=kind) for kind in (KIND_PREDICT, KIND_PGRAD)}
            g.set_profiling(0)
            for form, key in (("grad_ms", "k_predict_grad"), ("grad_mean_only_ms", "k_predict_grad_mean_only")):
                ks = prof[form][KIND_PGRAD]
                ms = ks["sum_ms"] / args.reps
                row[key] = {"launches_per_call": ks["launches"] / args.reps, "ms_per_call": round(ms, 4),
                            "bytes_per_call": ks["flop"] / args.reps,
                            "tbs": round(ks["flop"] / args.reps / ms / 1e9, 3) if ms > 0 else None,
                            "share_of_hbm": round(ks["flop"] / args.reps / ms / 1e9 / PEAK_HBM, 3) if ms > 0 else None}
            a, b = prof["grad_ms"][KIND_PREDICT], prof["grad_mean_only_ms"][KIND_PREDICT]
            vms, vfl = (a["sum_ms"] - b["sum_ms"]) / args.reps, (a["flop"] - b["flop"]) / args.reps
            row["v_product"] = {"launches_per_call": (a["launches"] - b["launches"]) / args.reps, "ms_per_call": round(vms, 4),
                                "flop_per_call": vfl, "tflops": round(vfl / vms / 1e9, 2) if vms > 0 else None,
                                "share_of_peak": round(vfl / vms / 1e9 / PEAK_FP64_MFMA, 3) if vms > 0 else None,
                                "k_predict_gemm_ms_per_call": round(b["sum_ms"] / args.reps, 4)}
            out["cases"].append(row)
            print(json.dumps(row), file=sys.stderr)
        g.close()
    line = json.dumps(out)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
