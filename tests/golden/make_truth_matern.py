#!/usr/bin/env python3
"""Generate tests/golden/truth_matern/<case>.json: the extended-precision Matern truth (tests/truth_matern.py) and its
fp64 yardstick at a size where the truth is too slow to compute inside a test.  CPU only, deterministic; inputs come
from `synth` seeds.

    python tests/golden/make_truth_matern.py              # every case

Same format as tests/golden/make_truth_ard.py: scalars and short vectors as 21-digit decimal strings -- LL, the three
gradient components, mean and variance at the 64 test points, and per quantity of truth.QUANTITIES the yardstick (the
fp64 Matern K through the CPU oracle's linear algebra, the data as given and 7 row permutations), the oracle's error on
the data as given and its largest error over the permutations alone.  "standin": the stand-in's ratio to the
yardstick (the fixture's row of the table in docs/ACCURACY.md).  "seconds" is informative only.
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
import truth_matern as tm  # noqa: E402
from conftest import synth  # noqa: E402
from make_truth import dec  # noqa: E402

OUT = os.path.join(HERE, "truth_matern")
NT = 64

# name -> n, d, kind, hyper-parameters, box half-width of synth (K far from diagonal)
CASES = {
    "n2049_m52": dict(n=2049, d=10, kind=tm.MATERN52, hp=[1.6, 0.2, -1.0], scale=2.0),   # 17 tiles
}


def inputs(name):
    """-> (X, y, Xt, hp, kind) of a case."""
    c = CASES[name]
    X, y = synth(c["n"], d=c["d"], seed=3 * c["n"] + c["d"], scale=c["scale"])
    Xt = synth(NT, d=c["d"], seed=7, scale=c["scale"])[0]
    Xt[5] = X[len(X) // 2]
    return X, y, np.ascontiguousarray(Xt), list(c["hp"]), c["kind"]


def compute(name, oracle=None):
    if oracle is None:
        from oracle.oracle_py import Oracle
        oracle = Oracle()
    X, y, Xt, hp, kind = inputs(name)
    t = tm.TruthMatern(X, y, hp, kind)
    tmean, tvar = t.predict(Xt)
    noise, first, rest, _ = tm.noise_level_matern(oracle, X, y, hp, Xt, kind, t, tmean, tvar)
    fl = truth.floors(truth.scales(hp, t.ll, t.grad, tmean))
    se = truth.errors(*tm.standin_matern(X, y, hp, Xt, kind), t.ll, t.grad, tmean, tvar)
    K = t.K.astype(np.float64)
    return dict(case=name, n=len(y), d=X.shape[1], kind=kind, hp=[float(h) for h in hp], nt=NT,
                ll=dec(t.ll), grad=dec(t.grad), mean=dec(tmean), var=dec(tvar),
                noise={q: dec(noise[q]) for q in tm.QUANTITIES},
                oracle_as_given={q: dec(first[q]) for q in tm.QUANTITIES},
                oracle_permuted={q: dec(rest[q]) for q in tm.QUANTITIES},
                standin={q: round(se[q] / max(noise[q], fl[q]), 2) for q in tm.QUANTITIES},
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
