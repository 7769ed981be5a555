"""Chain-first streams: which handles put their factorisation stream at the device's highest priority (kernels.h
TUNE_STREAM_PRIO = 0: evaluated alone, inverse beside the factorisation, at least TUNE_PRIO_MIN_NT tile rows), and that
no result depends on it -- the order of the launches on every stream is fixed, priorities only move WHEN they run.

The keys are set per handle (cugp_set_handle_tuning re-creates the handle's streams where the answer changes); the
process defaults are never touched.  Data as in test_gpu_launch_paths: d = 3 in a box of 16, K far from diagonal, so a
launch that ran before its operands were final would move every result far beyond the last bit.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import synth
from cugp_amd import capi

pytestmark = pytest.mark.gpu

PIPE_BLOCK, STREAM_PRIO, PRIO_MIN_NT = 3, 15, 21            # kernels.h TUNE_*
PRIO_RULE, PRIO_ON, PRIO_OFF = 0, 1, 4                      # TUNE_STREAM_PRIO: by the rule, chain first, no priorities
MIN_NT = 25                                                 # the rule's threshold in these tests (default: 64 tile rows)
D, SCALE = 3, 8.0
HP = np.array([0.9, 0.2, -1.0])
HP_OTHER = HP + np.array([0.3, -0.2, 0.25])


@pytest.fixture(scope="module")
def gp_mod():
    import cugp_amd.gp as gp
    return gp


def evaluate(g):
    g.set_loghyperparam(HP_OTHER)                           # nothing is answered from what the handle holds
    g.loglik_grad()
    g.set_loghyperparam(HP)
    ll, gr = g.loglik_grad()
    return ll, np.asarray(gr), g.get_K_inverse()


# 18 tiles: below the threshold; 25: the threshold itself; 49: the two-speed factorisation with its wide far passes
@pytest.mark.parametrize("n,by_rule", [(2304, False), (3200, True), (6272, True)])
def test_results_do_not_depend_on_priority(gp_mod, n, by_rule):
    X, y = synth(n, d=D, seed=n, scale=SCALE)
    g = gp_mod.Covsum(n, D)
    try:
        g.set_data(X, y)
        assert not g.chain_first()                          # the default threshold is beyond all three sizes
        g.set_tuning(PRIO_MIN_NT, MIN_NT)
        assert g.chain_first() == by_rule
        rule = evaluate(g)
        assert g.chain_first() == by_rule                   # ... and an evaluation changes nothing about it
        g.set_tuning(STREAM_PRIO, PRIO_ON)
        assert g.chain_first()
        on = evaluate(g)
        g.set_tuning(STREAM_PRIO, PRIO_OFF)
        assert not g.chain_first()
        off = evaluate(g)
        g.set_tuning(STREAM_PRIO, PRIO_RULE, own=False)     # back to the process default: the rule again
        assert g.chain_first() == by_rule
        assert np.all(np.isfinite(off[1])) and np.isfinite(off[0])
        for what, r in (("rule", rule), ("forced on", on)):
            assert r[0] == off[0], (what, r[0], off[0])
            assert np.array_equal(r[1], off[1]), (what, r[1], off[1])
            assert np.array_equal(r[2], off[2]), (what, "K^-1")
    finally:
        g.close()


def test_rule_needs_the_hand_over(gp_mod):
    """Without the inverse beside the factorisation nothing competes with the chain: no priority."""
    n = 3200
    X, y = synth(n, d=D, seed=n, scale=SCALE)
    g = gp_mod.Covsum(n, D)
    try:
        g.set_data(X, y)
        g.set_tuning(PRIO_MIN_NT, MIN_NT)
        assert g.chain_first()
        g.set_overlap(False)
        assert not g.chain_first()
        g.set_overlap(True)
        assert g.chain_first()
        g.set_tuning(PIPE_BLOCK, 0)                         # everything behind the factorisation on one stream
        assert not g.chain_first()
    finally:
        g.close()


def test_grouped_experts_take_no_priority(gp_mod):
    """Two 1500-row experts (12 tiles) with the threshold forced below their size: alone each handle would run chain
    first; as experts of a BCM, and as members of a cugp_group, they report that they do not -- before and after the
    pair is evaluated."""
    n = 1500
    X, y = synth(2 * n, d=D, seed=2 * n, scale=SCALE)
    alone = gp_mod.Covsum(n, D)
    try:
        alone.set_data(X[:n], y[:n])
        alone.set_tuning(PRIO_MIN_NT, 8)
        assert alone.chain_first()
    finally:
        alone.close()
    b = gp_mod.BCM.split(X, y, 2)
    try:
        experts = [b.expert(k) for k in range(2)]
        for e in experts:
            e.set_tuning(PRIO_MIN_NT, 8)
            assert not e.chain_first()
        b.set_BCM_log_hyperparam(HP)
        ll, gr, _ = b.loglik_grad()
        assert np.isfinite(ll) and np.all(np.isfinite(gr))
        assert not any(e.chain_first() for e in experts)
    finally:
        b.close()
    lib = capi.lib()
    lib.cugp_group_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_void_p)]
    lib.cugp_group_destroy.argtypes = [C.c_void_p]
    lib.cugp_group_destroy.restype = None
    hs = [gp_mod.Covsum(n, D) for _ in range(2)]
    grp = C.c_void_p()
    try:
        for i, g in enumerate(hs):
            g.set_data(X[i * n: (i + 1) * n], y[i * n: (i + 1) * n])
            g.set_tuning(PRIO_MIN_NT, 8)
            assert g.chain_first()
        capi.check(lib.cugp_group_create((C.c_void_p * 2)(*[g.handle for g in hs]), 2, C.byref(grp)))
        assert not any(g.chain_first() for g in hs)
    finally:
        if grp:
            lib.cugp_group_destroy(grp)
        for g in hs:
            g.close()
