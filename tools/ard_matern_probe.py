"""ARD x Matern against SE-ARD on one GPU: milliseconds per log-likelihood + gradient evaluation of an SE-ARD handle and of
Matern-3/2 and Matern-5/2 ARD handles on the same data and theta, interleaved call by call in one process (after two
warm-up evaluations and one 1000-point prediction each).
Cases: N = 1500, 4096, 8192 with D = 10; then 16 x 1500 rows as a BCM of each family (one group of shared launches).

Per case, over --reps evaluations: the medians, the SE-ARD evaluation's spread (max - min) and the differences of the
medians.  The kernels' own dispatch times come from running this same probe once under the profiler (a run of its own, no
counters, the program after the double dash):

    python tools/ard_matern_probe.py [--reps 10] [--json profiles/ard_matern_probe.json]
    rocprofv3 --kernel-trace --stats -d out -- python tools/ard_matern_probe.py --reps 3

--lib loads another libcugp.so (the parent commit's, for the alternating-process comparison of the existing paths): only
the symbols it has are bound, and the families it lacks are left out -- the SE-ARD and the isotropic Matern-5/2 handle
remain.

Acceptance (the form of section 13): a Matern-ARD evaluation exceeds the SE-ARD one by no more than
the difference of the build and trace kernels' dispatch times plus the SE-ARD evaluation's own spread.
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

SIZES = (1500, 4096, 8192)
D = 10
BCM_SHAPE = (16, 1500)
FAMILIES = (("se_ard", dict(ard=True)), ("matern32_ard", dict(kernel="matern32_ard")),
            ("matern52_ard", dict(kernel="matern52_ard")), ("matern52", dict(kernel="matern52")))


def stats(t):
    return {"median_ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4),
            "spread_ms": round(max(t) - min(t), 4)}


def interleaved(run, reps):
    """run: name -> fn(i) -> LL.  Two warm-up rounds (allocations, graph capture), then reps timed rounds, the families
    in turn inside every round."""
    t, ll = {v: [] for v in run}, {}
    for i in range(2 + reps):
        for v, fn in run.items():
            t0 = time.perf_counter()
            ll[v] = fn(i)
            if i >= 2:
                t[v].append((time.perf_counter() - t0) * 1e3)
    return t, ll


def row_of(t, ll):
    row = {v: stats(t[v]) for v in t}
    for v in t:
        if v.endswith("_ard") and v != "se_ard":
            row[v]["minus_se_ard_ms"] = round(row[v]["median_ms"] - row["se_ard"]["median_ms"], 4)
    row["ll"] = {v: float(ll[v]).hex() for v in ll}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--json", default="")
    ap.add_argument("--sizes", type=int, nargs="*", default=list(SIZES))
    ap.add_argument("--no-bcm", action="store_true")
    ap.add_argument("--lib", default="", help="another libcugp.so to load instead of the tree's")
    args = ap.parse_args()

    from cugp_amd import capi
    if args.lib:                                     # another build: bind what it has
        import ctypes
        capi.LIB_PATH = os.path.abspath(args.lib)
        capi._share_torch_hip_runtime()
        other = ctypes.CDLL(capi.LIB_PATH)
        capi.SIGNATURES = {k: v for k, v in capi.SIGNATURES.items() if hasattr(other, k)}
    import cugp_amd.gp as gp
    from conftest import synth
    have = "cugp_create_ard_kernel" in capi.SIGNATURES
    families = [f for f in FAMILIES if have or f[0] in ("se_ard", "matern52")]

    hp = [float(np.log(3.0))] * D + [0.0, float(np.log(0.1))]
    out = {"reps": args.reps, "build_id": capi.lib().cugp_build_id().decode(), "lib": args.lib or "tree", "d": D,
           "cases": [], "bcm": None}
    for n in args.sizes:
        X, y = synth(n, D, seed=15618)
        Xt = np.ascontiguousarray(X[:1000] * 0.5)
        hs = {}
        for name, kw in families:
            g = hs[name] = gp.Covsum(n, D, 0, **kw)
            g.set_data(X, y)
            g.set_loghyperparam(hp if g.ard else [hp[0]] + hp[D:])

        def ev(g):
            g.enqueue(True)                 # a full evaluation whatever the handle holds
            return g.fetch()[0]
        for g in hs.values():               # one prediction each: the cross-covariance kernels appear in a kernel trace
            ev(g)
            g.compute_test_means_and_variances(X, y, Xt)
        t, ll = interleaved({v: (lambda i, g=g: ev(g)) for v, g in hs.items()}, args.reps)
        row = dict(n=n, **row_of(t, ll))
        out["cases"].append(row)
        print(json.dumps(row), file=sys.stderr)
        for g in hs.values():
            g.close()
    if not args.no_bcm:
        K, n = BCM_SHAPE
        X, y = synth(K * n, D, seed=15618)
        bs = {name: gp.BCM.split(X, y, K, **kw) for name, kw in families if name.endswith("_ard")}

        def evb(b, i):                      # a new theta every time: nothing to reuse
            b.set_BCM_log_hyperparam([hp[0] + 1e-3 * (i + 1)] * D + hp[D:])
            return b.loglik_grad()[0]
        t, ll = interleaved({v: (lambda i, b=b: evb(b, i)) for v, b in bs.items()}, args.reps)
        out["bcm"] = dict(experts=K, rows=n, **row_of(t, ll))
        print(json.dumps(out["bcm"]), file=sys.stderr)
        for b in bs.values():
            b.close()
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
