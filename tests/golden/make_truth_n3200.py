#!/usr/bin/env python3
"""The 3200-row fixture (25 tiles: the smallest size at which a lone handle can hand its inverse over in every block
size cugp_pipe_block_for returns, 1 ... 16) of tests/test_gpu_handover_rule.py, by the generator of the other fixtures
(tests/golden/make_truth.py: same truth, same yardstick, same file format).  CPU only, deterministic.

    python tests/golden/make_truth_n3200.py            # writes tests/golden/truth/n3200.json (about a quarter of an hour)

The case is registered with make_truth only while one of its functions runs, so the cases that tests/test_truth_cpu.py
regenerates stay the ones make_truth.py lists.
"""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import make_truth  # noqa: E402
from conftest import HP_DENSE  # noqa: E402

NAME = "n3200"
CASE = dict(dir="truth", family="se", n=3200, d=10, hp=HP_DENSE, scale=10.0, experts=0)


def _call(fn, *args):
    make_truth.CASES[NAME] = CASE
    try:
        return fn(NAME, *args)
    finally:
        del make_truth.CASES[NAME]


def inputs():
    return _call(make_truth.inputs)


def load():
    return _call(make_truth.load)


if __name__ == "__main__":
    t0 = time.time()
    r = _call(make_truth.compute)
    r["seconds"] = round(time.time() - t0, 1)
    out = _call(make_truth.path)
    with open(out, "w") as f:
        json.dump(r, f, indent=1)
        f.write("\n")
    print("%s: %d rows, %.1f s -> %s" % (NAME, r["n"], r["seconds"], os.path.relpath(out, make_truth.ROOT)))
