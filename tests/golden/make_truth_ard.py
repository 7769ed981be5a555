#!/usr/bin/env python3
"""Generate tests/golden/truth_ard/<case>.json: the extended-precision ARD truth (tests/truth_ard.py) and its fp64
yardstick at a size where the truth is too slow to compute inside a test.  CPU only, deterministic; inputs come from
`synth` seeds.

    python tests/golden/make_truth_ard.py              # every case

Same format as tests/golden/make_truth.py: scalars and short vectors as 21-digit decimal strings -- LL, the d + 2
gradient components, mean and variance at the 64 test points, and per quantity of truth_ard.QUANTITIES the yardstick
(the CPU oracle on the scaled copy X / l, the data as given and 7 row permutations), the oracle's error on the data as
given and its largest error over the permutations alone.  "standin": the stand-in's ratio to the yardstick (the
fixture's row of the table in docs/ACCURACY.md).  "seconds" is informative only.
"""
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
import truth_ard as ta  # noqa: E402
from conftest import synth  # noqa: E402
from make_truth import dec  # noqa: E402

OUT = os.path.join(HERE, "truth_ard")
NT = 64

# name -> n, d, theta_l, theta_f, theta_n, box half-width of synth (K far from diagonal)
CASES = {
    "n2049_d10": dict(n=2049, d=10, th=np.linspace(0.6, 1.2, 10).tolist(), tf=0.2, tn=-1.0, scale=2.0),   # 17 tiles
}


def inputs(name):
    """-> (X, y, Xt, hp) of a case."""
    c = CASES[name]
    X, y = synth(c["n"], d=c["d"], seed=3 * c["n"] + c["d"], scale=c["scale"])
    Xt = synth(NT, d=c["d"], seed=7, scale=c["scale"])[0]
    Xt[5] = X[len(X) // 2]
    return X, y, np.ascontiguousarray(Xt), list(c["th"]) + [c["tf"], c["tn"]]


def compute(name, oracle=None):
    if oracle is None:
        from oracle.oracle_py import Oracle
        oracle = Oracle()
    X, y, Xt, hp = inputs(name)
    t = ta.TruthARD(X, y, hp)
    tm, tv = t.predict(Xt)
    noise, first, rest = ta.noise_level_ard(oracle, X, y, hp, Xt, t.ll, t.grad, tm, tv)
    fl = ta.floors_ard(ta.scales_ard(hp, t.ll, t.grad, tm))
    se = ta.errors_ard(*ta.standin_ard(X, y, hp, Xt), t.ll, t.grad, tm, tv)
    K = t.K.astype(np.float64)
    return dict(case=name, n=len(y), d=X.shape[1], hp=[float(h) for h in hp], nt=NT,
                ll=dec(t.ll), grad=dec(t.grad), mean=dec(tm), var=dec(tv),
                noise={q: dec(noise[q]) for q in ta.QUANTITIES},
                oracle_as_given={q: dec(first[q]) for q in ta.QUANTITIES},
                oracle_permuted={q: dec(rest[q]) for q in ta.QUANTITIES},
                standin={q: round(se[q] / max(noise[q], fl[q]), 2) for q in ta.QUANTITIES},
                cond=float("%.3g" % np.linalg.cond(K)), share_above_1e_3=round(float(np.mean(np.abs(K) > 1e-3)), 3))


def load(name):
    """A committed fixture with its numbers parsed back into longdouble / float."""
    with open(os.path.join(OUT, name + ".json")) as f:
        raw = json.load(f)
    out = dict(raw)
    out["ll"] = truth.LD(raw["ll"])
    for k in ("grad", "mean", "var"):
        out[k] = np.array([truth.LD(s) for s in raw[k]], dtype=truth.LD)
    for k in ("noise", "oracle_as_given", "oracle_permuted"):
        out[k] = {q: float(s) for q, s in raw[k].items()}
    return out


def main():
    os.makedirs(OUT, exist_ok=True)
    for name in sorted(CASES):
        t0 = time.time()
        r = compute(name)
        r["seconds"] = round(time.time() - t0, 1)
        path = os.path.join(OUT, name + ".json")
        with open(path, "w") as f:
            json.dump(r, f, indent=1)
            f.write("\n")
        print("%s: %d rows, %.1f s -> %s" % (name, r["n"], r["seconds"], os.path.relpath(path, ROOT)), flush=True)


if __name__ == "__main__":
    main()
