"""Hand-over block size (TUNE_PIPE_BLOCK, key 3) x factorisation-stream priority (TUNE_STREAM_PRIO, key 15) at one or more
sizes: a fresh handle per variant, the variants interleaved round by round on one board; wall time per LL+grad evaluation.
Per size: each variant's per-round figures, its median, and its difference from the default variant's median set against
the default variant's own spread over the rounds (A against A).  Key 15: 0 = the library's rule, 1 = the factorisation's
stream at the highest priority, 4 = no stream gets a priority (libraries without the rule: 0 and 4 are the same).
    python tools/handover_prio_sweep.py [--rounds 3] [--evals 10] [--prio 0,1] [--blocks -1,4,5,6,8] n [n ...]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cugp_amd.gp as gp                                  # noqa: E402
from cugp_amd import capi                                 # noqa: E402
from conftest import synth                                # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--evals", type=int, default=10)
ap.add_argument("--prio", default="0,1")
ap.add_argument("--blocks", default="-1,4,5,6,8")
ap.add_argument("sizes", type=int, nargs="+")
a = ap.parse_args()
prios = [int(v) for v in a.prio.split(",")]
blocks = [int(v) for v in a.blocks.split(",")]
hp = np.array([np.log(3.0), 0.0, np.log(0.1)])
L = capi.lib()
for n in a.sizes:
    X, y = synth(n)
    variants = [(w, p) for p in prios for w in blocks]
    res = {v: [] for v in variants}
    for rnd in range(a.rounds):
        for w, p in variants:
            capi.check(L.cugp_set_tuning(15, p))
            capi.check(L.cugp_set_tuning(3, w))
            g = gp.Covsum(n, 10)
            g.set_data(X, y)
            for it in range(3):
                g.set_loghyperparam(hp + 1e-3 * it)
                g.loglik_grad()
            t0 = time.perf_counter()
            for it in range(a.evals):
                g.set_loghyperparam(hp + 1e-4 * it)
                g.loglik_grad()
            res[(w, p)].append((time.perf_counter() - t0) * 1e3 / a.evals)
            g.close()
    capi.check(L.cugp_set_tuning(15, 0))
    capi.check(L.cugp_set_tuning(3, -1))
    base = res[variants[0]]
    bmed, spread = statistics.median(base), max(base) - min(base)
    print("n = %d (%d tiles): default variant %.3f ms, its spread over %d rounds %.3f ms" % (n, (n + 127) // 128, bmed, a.rounds, spread))
    for (w, p), r in res.items():
        d = statistics.median(r) - bmed
        print("  block %2d prio %d : %s | median %.3f | vs default %+.3f ms (%+.2f %%) %s"
              % (w, p, " ".join("%.3f" % v for v in r), statistics.median(r), d, 100 * d / bmed,
                 "beyond the spread" if abs(d) > spread else "inside the spread"), flush=True)
