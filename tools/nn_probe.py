"""Timings and model quality of the nearest-neighbour (Vecchia) GP on one MI355X -> profiles/nn_probe.json.
    python tools/nn_probe.py [--quick] [--quality]
Timing: D = 3 and 10, SE and RQ-ARD, N = 1e5 and 1e6 (--quick: 1e5 only), m = 15, 31, 63: loglik and loglik_grad as the median
of 5 warmed calls (host wall clock around the call: launch, sums, copy and wait), predict at 1000 points; covariance entries per
second = N (m + 1)(m + 2) / 2 useful lower-triangle entries per second of loglik (the kernel evaluates N MP^2), beside the
3.0e11 (SE) and 1.4e11 (RQ-ARD) k_cov_apply reaches.  The index rows of the timing runs are NOT nearest neighbours (a brute-force
search at 1e6 rows is out of reach): row i gathers m distinct rows scattered over a window of 4 m rows at a random earlier
place, which costs the gathers what true neighbours of shuffled rows cost.  Device times come from a separate
    rocprofv3 --kernel-trace --stats -- python tools/nn_probe.py --quick
--quality: at N = 1e5, D = 3, SE, true nearest neighbours (gp.nn_neighbors): LL against IterativeGP.loglik at the same theta and
predict's variance against IterativeGP.predict's exact variance at 64 points; reported, not asserted."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cugp_amd import gp  # noqa: E402

REACHED = {"se": 3.0e11, "rq_ard": 1.4e11}


def theta(kernel, d):
    return [0.9, 0.2, -1.0] if kernel == "se" else np.linspace(0.7, 1.3, d).tolist() + [0.4, 0.2, -1.0]


def scattered(n, m, rng):
    idx = np.full((n, m), -1, dtype=np.int32)
    off = (np.arange(m) * 4)[None, :] + rng.integers(0, 4, (n, m))
    start = (rng.random(n) * np.maximum(np.arange(n) - 4 * m + 1, 1)).astype(np.int64)
    full = np.arange(n) >= 4 * m
    idx[full] = (start[:, None] + off)[full]
    for i in range(min(n, 4 * m)):
        idx[i, :min(i, m)] = np.arange(min(i, m))
    return idx


def median_ms(fn, reps=5):
    fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ts))


def timing(sizes):
    rng = np.random.default_rng(1)
    rows = []
    for d in (3, 10):
        for n in sizes:
            X = rng.uniform(-4, 4, (n, d))
            y = np.sin(X[:, 0]) + 0.1 * rng.standard_normal(n)
            Xt = rng.uniform(-4, 4, (1000, d))
            for m in (15, 31, 63):
                idx = scattered(n, m, rng)
                idx_t = rng.integers(0, n // m, (1000, m)).astype(np.int32) * m + np.arange(m, dtype=np.int32)[None, :]
                for kernel in ("se", "rq_ard"):
                    g = gp.NeighborGP(n, m, d, kernel=kernel)
                    g.set_data(X, y)
                    g.set_neighbors(idx)
                    g.set_loghyper(theta(kernel, d))
                    r = dict(kernel=kernel, d=d, n=n, m=m, loglik_ms=median_ms(g.loglik), loglik_grad_ms=median_ms(g.loglik_grad),
                             predict_1000_ms=median_ms(lambda: g.predict(Xt, idx_t)))
                    r["entries_per_s"] = n * (m + 1) * (m + 2) / 2 / (r["loglik_ms"] * 1e-3)
                    r["k_cov_apply_entries_per_s"] = REACHED[kernel]
                    g.close()
                    rows.append(r)
                    print(json.dumps(r), flush=True)
    return rows


def quality():
    n, d, m = 100000, 3, 31
    rng = np.random.default_rng(2)
    X = rng.uniform(-4, 4, (n, d))
    y = np.sin(X[:, 0]) + 0.1 * rng.standard_normal(n)
    Xt, hp = rng.uniform(-4, 4, (64, d)), theta("se", d)
    g = gp.NeighborGP(n, m, d)
    g.set_data(X, y)
    g.set_neighbors(gp.nn_neighbors(X, m))
    g.set_loghyper(hp)
    ll = g.loglik()
    _, var = g.predict(Xt)
    g.close()
    it = gp.IterativeGP(n, d)
    it.set_data(X, y)
    it.set_loghyper(hp)
    it.set_precond(256)
    exact_ll = it.loglik(16, rng=np.random.default_rng(3), grad=False, tol=1e-6)["ll"]
    _, exact_var, _ = it.predict(Xt, tol=1e-8)
    it.close()
    excess = var / exact_var - 1.0
    return dict(n=n, d=d, m=m, kernel="se", ll_neighbor=ll, ll_iterative_slq=float(exact_ll),
                var_excess_min=float(excess.min()), var_excess_median=float(np.median(excess)), var_excess_max=float(excess.max()))


if __name__ == "__main__":
    out = {"timing": timing((100000,) if "--quick" in sys.argv else (100000, 1000000))}
    out["quality"] = quality() if "--quality" in sys.argv else "not measured"
    with open(os.path.join(ROOT, "profiles", "nn_probe.json"), "w") as f:
        json.dump(out, f, indent=1)
