"""Joint predictive covariance and posterior draws (cugp_predict_cov, cugp_predict_sample) on one GPU: milliseconds per
call against the marginal prediction, and k_predict_cov's rate against the fp64 MFMA peak.  Models: N = 8192 rows,
D = 10 (bench.py's) and N = 1500; nt in {100, 1000, 6200} test points; draws of nsamples in {1, 64, 1000}.

Per (model, nt), medians over --reps calls, the variants interleaved call by call, the handle's inverse already valid:
  predict_ms           cugp_predict (mean + marginal variance)
  cov_ms               cugp_predict_cov (mean + the nt x nt covariance, copied to the host and mirrored there)
  cov_device_ms        the same computation left on the device (cugp_predict_cov_device: one host wait, no copy)
  sample_ms[ns]        cugp_predict_sample with ns draws (the factorisation and the draws included)
Then, at profiling level 4 (every k_predict_cov launch timed by its own dispatch events), k_predict_cov alone:
  flop_launched = 2 * (lower output tiles as launched) * tile^2 * kend   (kend = N rounded up to 16)
  flop_nt2n     = nt^2 * N                                           (the lower triangle's multiply-adds, x2)
each over the kernel's duration, and flop_launched's rate over the fp64 MFMA peak of the part, 78.6 TF/s (bench.py's;
the library's own probe, cugp_mfma_peak_tflops, one dependent chain per wave, is recorded beside it and reads lower
than what the tile kernels reach).

    python tools/pred_joint_probe.py [--reps 10] [--json out.json]
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
NTS = (100, 1000, 6200)
NSAMPLES = (1, 64, 1000)
KIND_COV = 12
TUNE_COV_SPLIT = 20
PEAK_FP64_MFMA = 78.6      # TF/s, MI355X (as bench.py)


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def cov_shape(nt, n, aim):
    """the launch shape predict_cov_shape (predict_gfx950.h) picks (tile edge, lower tiles, kend, split)"""
    ntpad = (nt + 127) // 128 * 128
    t128 = (ntpad // 128) * (ntpad // 128 + 1) // 2
    wm = 2 if (aim > 0 and 4 * t128 <= aim) else 4
    edge = 32 * wm
    tiles = (ntpad // edge) * (ntpad // edge + 1) // 2
    kend = (n + 15) // 16 * 16
    split = aim // (1 if wm == 2 else 2) // tiles
    split = max(1, min(split, kend // 256, 64))
    while split > 1 and (split - 1) * ntpad * ntpad * 8 > (1 << 30):
        split -= 1
    kstep = ((kend + split - 1) // split + 15) // 16 * 16
    split = (kend + kstep - 1) // kstep
    return edge, tiles, kend, split


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--json", default="")
    args = ap.parse_args()

    import cugp_amd.gp as gp
    from cugp_amd import capi
    from conftest import synth

    L = capi.lib()
    hook = L.cugp_predict_cov_device
    hook.restype = C.c_int
    hook.argtypes = [C.c_void_p, capi._dp, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int)]
    peak = PEAK_FP64_MFMA
    hp = np.array([np.log(3.0), 0.0, np.log(0.1)])
    out = {"peak_fp64_mfma_tflops": peak, "peak_probe_tflops": round(gp.mfma_peak_tflops(0), 2), "reps": args.reps, "build_id": L.cugp_build_id().decode(),
           "cases": []}
    for n, d in MODELS:
        X, y = synth(n, d, seed=15618)
        g = gp.Covsum(n, d, 0)
        g.set_data(X, y)
        g.set_loghyperparam(hp)
        g.loglik_grad()
        v = C.c_int()
        capi.check(L.cugp_get_handle_tuning(g.handle, TUNE_COV_SPLIT, C.byref(v)))
        aim = v.value
        for nt in NTS:
            Xt = np.ascontiguousarray(np.random.default_rng(nt).uniform(-10, 10, (nt, d)))
            m, var = np.empty(nt), np.empty(nt)
            cov = np.empty((nt, nt))
            dptr, ld = C.c_void_p(), C.c_int()
            Z = {ns: np.ascontiguousarray(np.random.default_rng(ns).standard_normal((ns, nt))) for ns in NSAMPLES}
            S = {ns: np.empty((ns, nt)) for ns in NSAMPLES}
            calls = {
                "predict_ms": lambda: capi.check(L.cugp_predict(g.handle, capi.ptr(Xt), nt, capi.ptr(m), capi.ptr(var))),
                "cov_ms": lambda: capi.check(L.cugp_predict_cov(g.handle, capi.ptr(Xt), nt, 1, capi.ptr(m), capi.ptr(cov))),
                "cov_device_ms": lambda: capi.check(hook(g.handle, capi.ptr(Xt), nt, 1, C.byref(dptr), C.byref(ld))),
            }
            for ns in NSAMPLES:
                calls["sample_ms_%d" % ns] = (lambda ns=ns: capi.check(L.cugp_predict_sample(
                    g.handle, capi.ptr(Xt), nt, 1, 0.0, ns, capi.ptr(Z[ns]), capi.ptr(S[ns]))))
            for fn in calls.values():            # warm-up: every shape, scratch allocated
                fn()
                fn()
            res = {k: [] for k in calls}
            for _ in range(args.reps):
                for k, fn in calls.items():
                    res[k].append(timed(fn))
            row = {"n": n, "d": d, "nt": nt}
            row.update({k: round(statistics.median(v), 4) for k, v in res.items()})
            # the kernel alone, every launch timed by its own dispatch events
            g.set_profiling(4)
            g.kernel_stats(reset=True, kind=KIND_COV)
            for _ in range(args.reps):
                calls["cov_device_ms"]()
            ks = g.kernel_stats(reset=True, kind=KIND_COV)
            g.set_profiling(0)
            edge, tiles, kend, split = cov_shape(nt, n, aim)
            kms = ks["sum_ms"] / max(ks["launches"], 1)
            fl = ks["flop"] / max(ks["launches"], 1)
            row.update({"k_predict_cov": {"tile": edge, "lower_tiles": tiles, "kend": kend, "split": split,
                                          "workgroups": tiles * split, "launches": ks["launches"],
                                          "ms": round(kms, 4), "flop_launched": fl,
                                          "tflops_launched": round(fl / kms / 1e9, 2) if kms > 0 else None,
                                          "tflops_nt2n": round(nt * nt * n / kms / 1e9, 2) if kms > 0 else None,
                                          "share_of_peak": round(fl / kms / 1e9 / peak, 3) if kms > 0 else None}})
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
