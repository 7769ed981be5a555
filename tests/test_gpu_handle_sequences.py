"""Seeded call sequences on the library's handles (tests/handle_sequences.py): after every call on one long-lived handle,
what it returned is compared bit for bit with the same call on a fresh twin brought to the same logical state by the
canonical route.  One test per (subject shape, seed); `pytest -s` prints one SEQ line per step and the wall time of each
test (docs/ACCURACY.md, "Handle state: seeded call sequences", keeps the measured times).

No tuning, profiling or environment setting is touched.  Regressions found by a sequence are kept as fixed, named call
lists at the end of this file.
"""
import time

import pytest

import handle_sequences as hs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gp_mod():
    import cugp_amd.gp as gp
    return gp


@pytest.mark.parametrize("name,seed", hs.CASES, ids=["%s-%d" % c for c in hs.CASES])
def test_sequence(gp_mod, name, seed):
    sub = hs.SUBJECTS[name]
    t0 = time.perf_counter()
    ops = hs.run(sub, gp_mod, seed)
    print("SEQTIME %s %d: %d steps in %.2f s" % (name, seed, len(ops), time.perf_counter() - t0))
    assert len(ops) == sub.steps
