#!/usr/bin/env python3
"""Generate the fixtures under tests/golden/truth*/: the extended-precision truth (tests/truth.py) and the fp64 noise
level of the sizes where the truth is too slow to compute inside a test, for every covariance family.  CPU only,
deterministic; inputs come from `synth` seeds or from the committed data_*.npz.

    python tests/golden/make_truth.py                  # every case and its 300-row sibling
    python tests/golden/make_truth.py --case n2049     # one case (and its sibling)
    python tests/golden/make_truth.py --check          # recompute, compare with the committed files, write nothing
    python tests/golden/make_truth.py --standin        # the fixture rows of the stand-in tables in docs/ACCURACY.md

Each file holds scalars and short vectors only, as 21-digit decimal strings (an 80-bit long double round-trips):
LL, the gradient, mean and variance at the 64 test points, and per quantity of the family the noise level (the largest
error of the family's yardstick evaluation -- truth.yardstick -- over the data as given and 7 row permutations), its
error on the data as given and its largest error over the 7 permutations alone.  The ARD and Matern files also carry
three informative keys: "standin" (the stand-in's ratio to the yardstick: the fixture's row of the table in
docs/ACCURACY.md), "cond" and "share_above_1e_3" of K.  The sibling <case>_n300.json is the same generator at 300 rows,
without the informative keys (they are of the BLAS they were computed with); tests/test_truth_cpu.py regenerates it and
compares every string, so this file cannot drift from the fixtures.  "seconds" (how long the case took) is informative
only; --check compares every other key and exits non-zero on a difference.
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

NT = truth.NT
SIBLING_ROWS = 300

# name -> its directory, family (truth.FAMILIES), n, d, hyper-parameters, box half-width of synth (chosen so K is far
# from diagonal); experts: a BCM over that many; informative: with the stand-in row, cond and share of K
CASES = {
    "n2049": dict(dir="truth", family="se", n=2049, d=10, hp=[0.9, 0.2, -1.0], scale=2.0, experts=0),      # 17 tiles
    "n4200": dict(dir="truth", family="se", n=4200, d=10, hp=HP_DENSE, scale=10.0, experts=0),  # 33 tiles, the classic schedule's largest
    "bcm3x1500": dict(dir="truth", family="se", n=4500, d=None, hp=HP_BCM, data="data_si24000.npz", experts=3),
    "n2049_d10": dict(dir="truth_ard", family="ard", n=2049, d=10, hp=np.linspace(0.6, 1.2, 10).tolist() + [0.2, -1.0],
                      scale=2.0, informative=True),
    "n2049_m52": dict(dir="truth_matern", family="matern52", kind=truth.MATERN52, n=2049, d=10, hp=[1.6, 0.2, -1.0],
                      scale=2.0, informative=True),
}


def path(name, n=None):
    return os.path.join(HERE, CASES[name]["dir"], name + ("" if n is None else "_n%d" % n) + ".json")


def inputs(name, n=None):
    """-> (X, y, Xt, cov, experts) of a case, or of its sibling with `n` rows."""
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
        Xt = truth.points(X, c["d"], c["scale"])
    return X, y, np.ascontiguousarray(Xt), truth.FAMILIES[c["family"]][1](c["hp"]), c.get("experts", 0)


def dec(v):
    if np.ndim(v):
        return [dec(x) for x in v]
    return np.format_float_scientific(truth.LD(v), precision=20, unique=False)


def standin_ratios(X, y, Xt, cov, experts, tll, tg, tm, tv, noise):
    """Stand-in error / max(noise, floor) per quantity of the family, for a case's `inputs` and its truth."""
    st = truth.standin_bcm(cov, X, y, experts, Xt) if experts else truth.standin(cov, X, y, Xt)
    e = truth.errors(cov, *st, tll, tg, tm, tv)
    fl = truth.floors(cov, truth.scales(cov, tll, tg, tm))
    return {q: e[q] / max(noise[q], fl[q]) for q in cov.quantities}


def compute(name, n=None, oracle=None):
    """Everything the fixture stores, as strings (no timing)."""
    if oracle is None:
        from oracle.oracle_py import Oracle
        oracle = Oracle()
    c = CASES[name]
    X, y, Xt, cov, experts = inputs(name, n)
    informative = c.get("informative") and n is None
    if experts:
        t = truth.bcm_truth(X, y, cov, experts, Xt)
        tll, tg, tm, tv = t["ll"], t["grad"], t["mean"], t["var"]
        noise, first, rest = truth.bcm_yardstick(oracle, cov, X, y, experts, Xt, t)
    else:
        t = truth.Truth(X, y, cov, keep=bool(informative))
        tll, tg = t.ll, t.grad
        tm, tv = t.predict(Xt)
        noise, first, rest = truth.yardstick(oracle, cov, X, y, Xt, t, tm, tv)
    r = dict(case=name, n=len(y), d=X.shape[1])
    if "kind" in c:
        r["kind"] = c["kind"]
    r["hp"] = cov.hp
    if "experts" in c:
        r["experts"] = experts
    r.update(nt=NT, ll=dec(tll), grad=dec(tg), mean=dec(tm), var=dec(tv),
             noise={q: dec(noise[q]) for q in cov.quantities},
             oracle_as_given={q: dec(first[q]) for q in cov.quantities},
             oracle_permuted={q: dec(rest[q]) for q in cov.quantities})
    if informative:
        K = t.K.astype(np.float64)
        ratios = standin_ratios(X, y, Xt, cov, experts, tll, tg, tm, tv, noise)
        r.update(standin={q: round(v, 2) for q, v in ratios.items()}, cond=float("%.3g" % np.linalg.cond(K)),
                 share_above_1e_3=round(float(np.mean(np.abs(K) > 1e-3)), 3))
    return r


def load(name, n=None):
    """A committed fixture with its numbers parsed back into longdouble / float."""
    with open(path(name, n)) as f:
        raw = json.load(f)
    out = dict(raw)
    out["ll"] = truth.LD(raw["ll"])
    for k in ("grad", "mean", "var"):
        out[k] = np.array([truth.LD(s) for s in raw[k]], dtype=truth.LD)
    for k in ("noise", "oracle_as_given", "oracle_permuted"):
        out[k] = {q: float(s) for q, s in raw[k].items()}
    out["raw"] = raw
    return out


def standin_row(name, n=None):
    """The stand-in ratios of a committed fixture (or of its sibling): its row of the table in docs/ACCURACY.md."""
    f = load(name, n)
    return standin_ratios(*inputs(name, n), f["ll"], f["grad"], f["mean"], f["var"], f["noise"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", action="append", choices=sorted(CASES))
    ap.add_argument("--sibling-only", action="store_true")
    ap.add_argument("--check", action="store_true", help="recompute and compare every key but \"seconds\" with the "
                    "committed files; write nothing, exit 1 on a difference")
    ap.add_argument("--standin", action="store_true", help="print the stand-in / yardstick ratios of the committed "
                    "fixtures instead of generating them")
    a = ap.parse_args()
    differ = 0
    for name in a.case or sorted(CASES):
        if a.standin:
            print("%-10s " % name + "  ".join("%s %.2f" % kv for kv in standin_row(name).items()))
            continue
        for n in (SIBLING_ROWS,) if a.sibling_only else (SIBLING_ROWS, None):
            rel = os.path.relpath(path(name, n), ROOT)
            if a.check and not os.path.exists(path(name, n)):
                differ += 1
                print("%s: %s is missing" % (name, rel), flush=True)
                continue
            t0 = time.time()
            r = compute(name, n)
            seconds = round(time.time() - t0, 1)
            if a.check:
                want = dict(load(name, n)["raw"])
                want.pop("seconds")
                bad = sorted(k for k in set(r) | set(want) if r.get(k) != want.get(k))
                differ += bool(bad)
                print("%s: %d rows, %.1f s, %s %s" % (name, r["n"], seconds, rel, "differs in %s" % bad if bad else "is reproduced"), flush=True)
                continue
            r["seconds"] = seconds
            os.makedirs(os.path.dirname(path(name, n)), exist_ok=True)
            with open(path(name, n), "w") as f:
                json.dump(r, f, indent=1)
                f.write("\n")
            print("%s: %d rows, %.1f s -> %s" % (name, r["n"], seconds, rel), flush=True)
    sys.exit(1 if differ else 0)


if __name__ == "__main__":
    main()
