#!/usr/bin/env python3
"""Generate tests/golden/truth/<case>.json: the extended-precision truth (tests/truth.py) and the fp64 noise level of
the sizes where the truth is too slow to compute inside a test.  CPU only, deterministic; inputs come from `synth`
seeds or from the committed data_*.npz.

    python tests/golden/make_truth.py                  # every case and its 300-row sibling
    python tests/golden/make_truth.py --case n2049     # one case (and its sibling)
    python tests/golden/make_truth.py --standin        # the fixture rows of the stand-in table in docs/ACCURACY.md

Each file holds scalars and short vectors only, as 21-digit decimal strings (an 80-bit long double round-trips):
LL, the gradient, mean and variance at the 64 test points, and per quantity the noise level (the largest error of the
CPU oracle over the data as given and 7 row permutations), the oracle's error on the data as given and its largest
error over the 7 permutations alone.  The sibling
<case>_n300.json is the same generator at 300 rows; tests/test_truth_cpu.py regenerates it and compares every
string, so this file cannot drift from the fixtures.  "seconds" (how long the case took) is informative only.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import truth  # noqa: E402
from conftest import HP_BCM, HP_DENSE, synth  # noqa: E402

OUT = os.path.join(HERE, "truth")
NT = 64
SIBLING_ROWS = 300

# name -> n, d, hyper-parameters, box half-width of synth (chosen so K is far from diagonal), experts (0: one GP)
CASES = {
    "n2049": dict(n=2049, d=10, hp=[0.9, 0.2, -1.0], scale=2.0, experts=0),       # 17 tiles
    "n4200": dict(n=4200, d=10, hp=HP_DENSE, scale=10.0, experts=0),              # 33 tiles, the classic schedule's largest
    "bcm3x1500": dict(n=4500, d=None, hp=HP_BCM, data="data_si24000.npz", experts=3),
}


def make_test_points(X, d, scale, seed=7):
    """64 test points in the training box, one of which is a training row."""
    Xt = synth(NT, d=d, seed=seed, scale=scale)[0]
    Xt[5] = X[len(X) // 2]
    return Xt


def inputs(name, n=None):
    """-> (X, y, Xt, hp, experts) of a case, or of its sibling with `n` rows."""
    c = CASES[name]
    n = c["n"] if n is None else n
    if "data" in c:
        dat = np.load(os.path.join(HERE, c["data"]))
        X, y = np.ascontiguousarray(dat["X"][:n]), np.ascontiguousarray(dat["y"][:n])
        lo, hi = X.min(0), X.max(0)
        Xt = lo + (hi - lo) * np.random.default_rng(7).uniform(0, 1, (NT, X.shape[1]))
        Xt[5] = X[n // 2]
    else:
        X, y = synth(n, d=c["d"], seed=3 * c["n"] + c["d"], scale=c["scale"])
        Xt = make_test_points(X, c["d"], c["scale"])
    return X, y, np.ascontiguousarray(Xt), list(c["hp"]), c["experts"]


def dec(v):
    if np.ndim(v):
        return [dec(x) for x in v]
    return np.format_float_scientific(truth.LD(v), precision=20, unique=False)


def compute(name, n=None, oracle=None):
    """Everything the fixture stores, as strings (no timing)."""
    if oracle is None:
        from oracle.oracle_py import Oracle
        oracle = Oracle()
    X, y, Xt, hp, experts = inputs(name, n)
    if experts:
        t = truth.bcm_truth(X, y, hp, experts, Xt)
        tll, tg, tm, tv = t["ll"], t["grad"], t["mean"], t["var"]

        def evaluate(Xp, yp):
            b = oracle.bcm(Xp, yp, experts, hp)
            try:
                return (b.loglik()[0], b.grad()) + tuple(b.predict(Xt))
            finally:
                b.close()
        noise, first, rest = truth.noise_level(oracle, X, y, hp, Xt, tll, tg, tm, tv, evaluate=evaluate,
                                         parts=truth.bcm_rows(len(y), experts))
    else:
        t = truth.Truth(X, y, hp, keep=False)
        tll, tg = t.ll, t.grad
        tm, tv = t.predict(Xt)
        noise, first, rest = truth.noise_level(oracle, X, y, hp, Xt, tll, tg, tm, tv)
    return dict(case=name, n=len(y), d=X.shape[1], hp=[float(h) for h in hp], experts=experts, nt=NT,
                ll=dec(tll), grad=dec(tg), mean=dec(tm), var=dec(tv),
                noise={q: dec(noise[q]) for q in truth.QUANTITIES},
                oracle_as_given={q: dec(first[q]) for q in truth.QUANTITIES},
                oracle_permuted={q: dec(rest[q]) for q in truth.QUANTITIES})


def load(name, n=None):
    """A committed fixture with its numbers parsed back into longdouble / float."""
    path = os.path.join(OUT, name + ("" if n is None else "_n%d" % n) + ".json")
    with open(path) as f:
        raw = json.load(f)
    out = dict(raw)
    out["ll"] = truth.LD(raw["ll"])
    for k in ("grad", "mean", "var"):
        out[k] = np.array([truth.LD(s) for s in raw[k]], dtype=truth.LD)
    for k in ("noise", "oracle_as_given", "oracle_permuted"):
        out[k] = {q: float(s) for q, s in raw[k].items()}
    out["raw"] = raw
    return out


def standin_ratios(name):
    """Stand-in error / max(noise, floor) of a committed fixture case: its row of the table in docs/ACCURACY.md."""
    f = load(name)
    X, y, Xt, hp, experts = inputs(name)
    st = truth.standin_bcm(X, y, hp, experts, Xt) if experts else truth.standin(X, y, hp, Xt)
    e = truth.errors(*st, f["ll"], f["grad"], f["mean"], f["var"])
    fl = truth.floors(truth.scales(hp, f["ll"], f["grad"], f["mean"]))
    return {q: e[q] / max(f["noise"][q], fl[q]) for q in truth.QUANTITIES}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", action="append", choices=sorted(CASES))
    ap.add_argument("--sibling-only", action="store_true")
    ap.add_argument("--standin", action="store_true", help="print the stand-in / yardstick ratios of the committed "
                    "fixtures instead of generating them")
    a = ap.parse_args()
    os.makedirs(OUT, exist_ok=True)
    for name in a.case or sorted(CASES):
        if a.standin:
            print("%-10s " % name + "  ".join("%s %.2f" % kv for kv in standin_ratios(name).items()))
            continue
        for n in (SIBLING_ROWS,) if a.sibling_only else (SIBLING_ROWS, None):
            t0 = time.time()
            r = compute(name, n)
            r["seconds"] = round(time.time() - t0, 1)
            path = os.path.join(OUT, name + ("" if n is None else "_n%d" % n) + ".json")
            with open(path, "w") as f:
                json.dump(r, f, indent=1)
                f.write("\n")
            print("%s: %d rows, %.1f s -> %s" % (name, r["n"], r["seconds"], os.path.relpath(path, ROOT)), flush=True)


if __name__ == "__main__":
    main()
