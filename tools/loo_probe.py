"""What leave-one-out cross-validation costs beside an evaluation (one GPU; needs the built library):

    python tools/loo_probe.py --json profiles/loo_probe.json          # N = 1500, 4096, 8192, D = 10, SE and SE-ARD
    python tools/loo_probe.py --sizes 8192 --families se --once      # one pass, for a rocprofv3 --kernel-trace --stats run

Per size and family, medians of --reps calls, host clock around the synchronous call, in ms:
  eval        cugp_loglik_grad at a fresh hyper-parameter vector: the evaluation every LOO call of a stale handle runs first
  loo_obj     cugp_loo(g = NULL) on the evaluated handle: k_loo_point, k_loo_sum and one host wait
  loo_grad    cugp_loo with the gradient on the evaluated handle: + k_loo_mirror_scale, k_loo_bsum, k_loo_product,
              k_trace_loo, k_loo_finalize
  predict     cugp_loo_predict on the evaluated handle (three copies of n doubles)
and from the library's own per-launch timing (profiling level 3, its event pairs around each launch):
  product_ms  one k_loo_product launch; product_tflops and its fraction of the fp64 MFMA spec (78.6 TFLOP/s), beside
  lauum_*     the same for k_lauum<4> / <2> of the evaluation on the same handle (the shares of K^-1: the same tile product
              at shorter, non-uniform K)
  textbook_ms ARD: d + 2 launches of k_loo_product timed one after the other -- what GPML 5.13 as written would launch,
              one N^3 product per hyper-parameter -- beside the one launch of the fused formulation
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

PEAK = 78.6
KIND_LAUUM4, KIND_LAUUM2, KIND_LOO = 4, 5, 14


def median_ms(fn, reps):
    ts = []
    for i in range(2 + reps):                                # (two warm-up calls)
        t0 = time.perf_counter()
        fn(i)
        ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts[2:]))


def stats(g, kinds):
    ms = fl = n = 0.0
    for k in kinds:
        s = g.kernel_stats(reset=True, kind=k)
        ms, fl, n = ms + s["sum_ms"], fl + s["flop"], n + s["launches"]
    return ms, fl, n


def probe(n, d, family, reps):
    import cugp_amd.gp as gp
    from conftest import synth
    X, y = synth(n, d, seed=15618)
    ard = family == "ard"
    g = gp.Covsum(n, d, 0, ard=ard)
    g.set_data(X, y)

    def hyper(i):
        g.set_loghyperparam([float(np.log(3.0)) + 1e-3 * i] * (d if ard else 1) + [0.0, float(np.log(0.1))])

    def evaluate(i):
        hyper(i)
        g.loglik_grad()
    out = dict(n=n, d=d, family=family, nh=g.nh)
    out["eval_ms"] = median_ms(evaluate, reps)
    out["loo_obj_ms"] = median_ms(lambda i: g.loo(want_grad=False), reps)
    out["loo_grad_ms"] = median_ms(lambda i: g.loo(), reps)
    out["predict_ms"] = median_ms(lambda i: g.loo_predict(), reps)
    lpl, gr = g.loo()
    out["lpl"], out["grad_finite"] = lpl, bool(np.all(np.isfinite(gr)))
    # per-launch timing by the library's own events
    g.set_profiling(3)
    hyper(reps + 3)
    g.loglik_grad()
    stats(g, (KIND_LOO,))
    lms, lfl, ln = stats(g, (KIND_LAUUM4, KIND_LAUUM2))
    g.loo()
    pms, pfl, pn = stats(g, (KIND_LOO,))
    out.update(product_ms=pms / max(pn, 1), product_tflops=pfl / pms / 1e9 if pms else None,
               lauum_ms=lms, lauum_launches=ln, lauum_tflops=lfl / lms / 1e9 if lms else None)
    for k in ("product", "lauum"):
        out[k + "_frac_of_spec"] = out[k + "_tflops"] / PEAK if out[k + "_tflops"] else None
    if ard:
        for _ in range(g.nh):
            g.loo()
        tms, _, tn = stats(g, (KIND_LOO,))
        out.update(textbook_ms=tms, textbook_launches=tn)
    g.set_profiling(0)
    g.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1500, 4096, 8192])
    ap.add_argument("--families", nargs="+", default=["se", "ard"], choices=["se", "ard"])
    ap.add_argument("--dims", type=int, default=10)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--once", action="store_true", help="one evaluation and one gradient call per case, nothing timed")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    rows = []
    for n in args.sizes:
        for family in args.families:
            if args.once:
                import cugp_amd.gp as gp
                from conftest import synth
                X, y = synth(n, args.dims, seed=15618)
                g = gp.Covsum(n, args.dims, 0, ard=family == "ard")
                g.set_data(X, y)
                g.set_loghyperparam([float(np.log(3.0))] * (args.dims if family == "ard" else 1) + [0.0, float(np.log(0.1))])
                for _ in range(3):
                    print(n, family, g.loo()[0], flush=True)
                g.close()
                continue
            r = probe(n, args.dims, family, args.reps)
            rows.append(r)
            print(json.dumps(r), flush=True)
    if args.json and rows:
        from cugp_amd import capi
        doc = dict(build_id=(capi.lib().cugp_build_id() or b"unknown").decode(), peak_tflops=PEAK, reps=args.reps, rows=rows)
        with open(args.json, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
