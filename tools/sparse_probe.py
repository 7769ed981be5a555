"""What the sparse variational model costs (one GPU; needs the built library):

    python tools/sparse_probe.py --json profiles/sparse_probe.json       # N = 1e5, 1e6; M = 512, 1024, 2048; D = 10, SE
    python tools/sparse_probe.py --sizes 100000 --inducing 1024 --once   # one pass, for a rocprofv3 --kernel-trace --stats run

Per (N, M), medians of --reps calls, host clock around the synchronous call, in ms:
  bound        cugp_sparse_bound at a fresh hyper-parameter vector: the inner evaluation over Z, every chunk's
               cross-covariance, triangular product and Gram product, B's factorisation, the final sums
  bound_grad   cugp_sparse_bound_grad at a fresh vector: + a second pass over the chunks (weights and rectangular trace)
  predict      1000 test points on the evaluated handle
  gflop        algorithmic, multiply + add: N M^2 (the triangular product, half a full one) + N M^2 (the Gram product's
               lower tiles) for the bound; the gradient adds the triangular product a second time and 2 N M^2 (weights)
and the products alone, best of 5 by HIP events (cugp_bench_la): the Gram product of one 16384-row chunk against M
(k_sparse_gram and its fixed-order sum), and the plain NT product C = K K^T at n = 4096 -- what an fp64 tile product
reaches on the same card in the same visit; tools/loo_probe.py gives k_loo_product beside them.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

PEAK = 78.6
CHUNK = 16384


def median_ms(fn, reps):
    ts = []
    for i in range(1 + reps):                                # (one warm-up call)
        t0 = time.perf_counter()
        fn(i)
        ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts[1:]))


def bench_la(op, n):
    from cugp_amd import capi
    ms = C.c_double()
    capi.check(capi.lib().cugp_bench_la(op, n, 0, 5, C.byref(ms)))
    return ms.value


def gram_alone(m):
    mp = -(-m // 128) * 128
    tiles = (mp // 128) * (mp // 128 + 1) // 2
    ms = bench_la(5, m)
    tf = 2.0 * tiles * 128 * 128 * CHUNK / ms / 1e9
    return dict(m=m, gram_ms=ms, gram_tflops=tf, gram_frac_of_spec=tf / PEAK)


def model(n, m, d, reps, once=False):
    import cugp_amd.gp as gp
    from conftest import synth
    X, y = synth(n, d, seed=15618)
    s = gp.SparseGP.from_subset(X, y, m, seed=0)
    Xt = np.ascontiguousarray(X[:1000] * 0.5)

    def hyper(i):
        s.set_loghyperparam([float(np.log(3.0)) + 1e-3 * i, 0.0, float(np.log(0.1))])
    if once:
        for i in range(3):
            hyper(i)
            print(n, m, s.bound_grad()[0], flush=True)
        s.close()
        return None

    def bound(i):
        hyper(i)
        s.bound()

    def bound_grad(i):
        hyper(100 + i)
        s.bound_grad()
    out = dict(n=n, m=m, d=d, chunks=len(s.plan()), split=s.plan()[0][3])
    out["bound_ms"] = median_ms(bound, reps)
    out["bound_grad_ms"] = median_ms(bound_grad, reps)
    out["predict_1000_ms"] = median_ms(lambda i: s.predict(Xt), reps)
    F, g = s.bound_grad()
    out["F"], out["grad_finite"] = F, bool(np.all(np.isfinite(g)))
    out["bound_gflop"] = 2.0 * n * m * m / 1e9
    out["bound_grad_gflop"] = 5.0 * n * m * m / 1e9
    out["bound_tflops"] = out["bound_gflop"] / out["bound_ms"]
    out["bound_grad_tflops"] = out["bound_grad_gflop"] / out["bound_grad_ms"]
    s.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--inducing", type=int, nargs="+", default=[512, 1024, 2048])
    ap.add_argument("--dims", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--once", action="store_true", help="three gradient evaluations per case, nothing timed")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    rows, products = [], []
    if not args.once:
        plain = bench_la(4, 4096)
        products.append(dict(plain_nt_n=4096, plain_nt_ms=plain, plain_nt_tflops=2.0 * 4096 ** 3 / plain / 1e9,
                             plain_nt_frac_of_spec=2.0 * 4096 ** 3 / plain / 1e9 / PEAK))
        print(json.dumps(products[-1]), flush=True)
        for m in args.inducing:
            products.append(gram_alone(m))
            print(json.dumps(products[-1]), flush=True)
    for n in args.sizes:
        for m in args.inducing:
            r = model(n, m, args.dims, args.reps, args.once)
            if r:
                rows.append(r)
                print(json.dumps(r), flush=True)
    if args.json and rows:
        from cugp_amd import capi
        doc = dict(build_id=(capi.lib().cugp_build_id() or b"unknown").decode(), peak_tflops=PEAK, reps=args.reps,
                   chunk_rows=CHUNK, products=products, rows=rows)
        with open(args.json, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
