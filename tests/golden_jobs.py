"""The reference-generated jobs under tests/golden/golden_r2 and the parity tolerances they are compared at -- TEST
INFRASTRUCTURE shared by tests/test_gpu_golden_configs.py and the ARD test of the same golden (tests/test_gpu_ard.py).

Tolerances (fp64): log-likelihood |d| <= 1e-8 max(1, |LL|); gradients per component |d_i| <= 1e-6 |g_i| + 1e-9 max|g|.
"""
import json
import os

import numpy as np

from conftest import GOLDEN

R2 = os.path.join(GOLDEN, "golden_r2")


def job(name):
    p = os.path.join(R2, name + ".json")
    # a committed fixture that has gone missing is a FAILURE, not a skip: every job listed by
    # `make_golden.py --job list` (tests/golden/run_jobs.sh) is in the tree (tests/test_oracle_golden.py checks the list)
    assert os.path.exists(p), "golden_r2/%s.json is missing (tests/golden/run_jobs.sh generates it in the build container)" % name
    with open(p) as f:
        return json.load(f)


def ll_close(a, b):
    return abs(a - b) <= 1e-8 * max(1.0, abs(b))


def grad_close(a, b, rel=1e-6, floor=1e-9):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return bool(np.all(np.abs(a - b) <= rel * np.abs(b) + floor * max(1.0, np.max(np.abs(b)))))
