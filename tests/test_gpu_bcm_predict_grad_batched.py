"""The input gradients of a product of experts on the batched path and across ranks (cugp_bcm_predict_grad on
cugp_group_predict_grad_enqueue; cugp_bcm_predict_grad_allgather with k_poe_reduce_grad).

  batched = expert by expert   BCM.predict_grad must carry, in all four outputs and all five modes, the bits of
                               cugp_predict_grad on every cugp_bcm_expert handle (latent or noisy as the mode requires)
                               followed by the host rules (poe_combine / poe_finish, poe_combine_grad) -- `per_expert`
                               below is that computation, shared by the tests
  fallback                     the same bits when the experts cannot share launches (predict_grad_form == 1)
  the communicator form        a world of one: b.predict_grad's bits for the rules without a transcendental; rbcm (each
                               side's own log) is held to the bounds the existing suite gives that difference:
                               mean / var to truth_poe_modes' yardstick and floors, dmean / dvar to tpg.bcm_case's truth,
                               yardstick and floor, both at tpg.factor(cov) -- truth.F / F_ARD / F_MATERN as they stand
The shapes are the smallest at which the batched kernels can go wrong: experts of one padded size with 1, 1 and 2
training tiles (n = 64, 64, 66), one test point, a ragged second test tile (65), two 128-row test tiles (200), a second
feature chunk (d = 17), and 4 passes against one."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import truth
import truth_poe_modes as tpm
import truth_predict_grad as tpg
from accuracy import Report
from conftest import ROOT, synth
from cugp_amd import capi

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not truth.EXTENDED, reason="numpy.longdouble is not an extended-precision type here")]

TUNE_PRED_CHUNK = 19                                                # kernels.h TUNE_*
MODES = (None, "poe", "gpoe", "bcm", "rbcm")
BITWISE = (None, "poe", "gpoe", "bcm")                             # no transcendental: host and device agree bit for bit
HP_ARD17 = list(np.linspace(0.8, 1.6, 17)) + [0.2, -1.0]


@pytest.fixture(scope="module")
def gp_mod():
    import cugp_amd.gp as gp
    return gp


@pytest.fixture(scope="module")
def comm1(gp_mod):
    c = gp_mod.Comm(None, 0, 1, 0)            # a world of one without an id: no RCCL
    yield c
    c.close()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def all_same(r, w):
    return len(r) == len(w) == 4 and all(same_bits(a, b) for a, b in zip(r, w))


def per_expert(gp_mod, b, Xt, combine, with_noise=True):
    """cugp_predict_grad on each cugp_bcm_expert handle -- noisy for the reference's product, else latent -- then the host
    rules in expert order: what cugp_bcm_predict_grad computed before the batched path."""
    ex = [b.expert(k).predict_grad(Xt, with_noise=combine is None) for k in range(len(b.rows))]
    m, v, dm, dv = (np.stack([e[i] for e in ex]) for i in range(4))
    sf2, sn2 = b.prior_scalars()
    inv = 1.0 / v
    if combine is None:
        sp, spm = np.zeros(len(Xt)), np.zeros(len(Xt))
        for k in range(len(ex)):
            sp += inv[k]
            spm += inv[k] * m[k]
        mean, var = gp_mod.poe_finish(sp, spm)
    else:
        mean, var = gp_mod.poe_combine(np.stack([inv, inv * m], axis=1), combine, sf2, sn2, with_noise)
    return (mean, var) + gp_mod.poe_combine_grad(m, v, dm, dv, combine, sf2)


def truth_bcm(gp_mod, name, nt=tpg.BCM_NT, **kw):
    """A case of truth_poe_modes.CASES as a BCM with its hyper-parameters set -> (b, Xt, cov)."""
    X, y, Xt, cov, K = tpm.inputs(name, nt)
    family = tpm.CASES[name][0]
    b = gp_mod.BCM.split(X, y, K, kernel="se" if family == "ard" else family, ard=family == "ard", **kw)
    b.set_BCM_log_hyperparam(cov.hp)
    return b, Xt, cov


def ragged_bcm(gp_mod):
    """N = 194, K = 3: 64, 64 and 66 rows, one padded size of 128 -- 1, 1 and 2 training tiles of 64"""
    X, y = synth(194, 3, seed=194, scale=3.0)
    b = gp_mod.BCM.split(X, y, 3)
    assert b.rows == [64, 64, 66]
    b.set_BCM_log_hyperparam(tpm.HP)
    return b


def ard17_bcm(gp_mod):
    X, y = synth(390, 17, seed=17, scale=2.0)
    b = gp_mod.BCM.split(X, y, 3, kernel="matern32_ard")
    b.set_BCM_log_hyperparam(HP_ARD17)
    return b


def hold_all_modes(gp_mod, b, Xt, form=2):
    for combine in MODES:
        for with_noise in ((True,) if combine is None else (True, False)):
            got = b.predict_grad(Xt, combine=combine, with_noise=with_noise)
            assert b.predict_grad_form == form, (combine, b.predict_grad_form)
            assert all(np.all(np.isfinite(a)) for a in got)
            assert all_same(got, per_expert(gp_mod, b, Xt, combine, with_noise)), (combine, with_noise)


# ------------------------------------------------------------------ batched equals expert by expert
@pytest.mark.parametrize("nt", (1, 65, 200))
def test_ragged_experts(gp_mod, nt):
    b = ragged_bcm(gp_mod)
    try:
        Xt = synth(nt, 3, seed=7, scale=3.0)[0]
        assert b.predict_grad_form == 0
        hold_all_modes(gp_mod, b, Xt)
        first = b.predict_grad(Xt, combine="rbcm")
        assert all_same(b.predict_grad(Xt, combine="rbcm"), first)        # a second call: the same bits
        if nt == 200:                                                      # 4 passes of 64 rows against one
            try:
                capi.check(capi.lib().cugp_set_tuning(TUNE_PRED_CHUNK, 1))
                assert all_same(b.predict_grad(Xt, combine="rbcm"), first) and b.predict_grad_form == 2
                assert all_same(b.predict_grad(Xt), per_expert(gp_mod, b, Xt, None))
            finally:
                capi.check(capi.lib().cugp_set_tuning(TUNE_PRED_CHUNK, 0))
    finally:
        b.close()


@pytest.mark.parametrize("name", ("se_5x261p2", "matern52_3x300", "ard_3x300"))
def test_truth_models(gp_mod, name):
    b, Xt, _ = truth_bcm(gp_mod, name)
    try:
        hold_all_modes(gp_mod, b, Xt)
    finally:
        b.close()


def test_matern32_ard_second_feature_chunk(gp_mod):
    b = ard17_bcm(gp_mod)
    try:
        hold_all_modes(gp_mod, b, synth(65, 17, seed=9, scale=2.0)[0])
    finally:
        b.close()


# ------------------------------------------------------------------ fallback
def test_profiled_expert_goes_expert_by_expert(gp_mod):
    b = ragged_bcm(gp_mod)
    try:
        Xt = synth(65, 3, seed=7, scale=3.0)[0]
        grouped = b.predict_grad(Xt, combine="bcm")
        assert b.predict_grad_form == 2
        b.expert(1).set_profiling(3)
        hold_all_modes(gp_mod, b, Xt, form=1)
        assert all_same(b.predict_grad(Xt, combine="bcm"), grouped)       # the path does not show in the bits
        b.expert(1).set_profiling(0)
        assert all_same(b.predict_grad(Xt, combine="bcm"), grouped) and b.predict_grad_form == 2
    finally:
        b.close()


def test_unequal_padded_sizes_go_expert_by_expert(gp_mod):
    X, y = synth(1000, 3, seed=5, scale=3.0)
    b = gp_mod.BCM([300, 700], 3)
    try:
        b.set_expert_data(0, X[:300], y[:300])
        b.set_expert_data(1, X[300:], y[300:])
        b.set_BCM_log_hyperparam(tpm.HP)
        hold_all_modes(gp_mod, b, synth(65, 3, seed=7, scale=3.0)[0], form=1)
    finally:
        b.close()


def test_two_device_sets_give_the_bits_of_one(gp_mod):
    one, Xt, _ = truth_bcm(gp_mod, "se_5x261p2")
    two, _, _ = truth_bcm(gp_mod, "se_5x261p2", devices=[0, 0])
    try:
        for combine in (None, "gpoe", "rbcm"):
            assert all_same(two.predict_grad(Xt, combine=combine), one.predict_grad(Xt, combine=combine)), combine
    finally:
        one.close()
        two.close()


def test_two_device_sets_expert_by_expert(gp_mod):
    """Two device sets in the fallback: every set orders its own stream behind its experts' by its own events (one GPU
    listed twice is the nearest a single GPU comes to several; the events of a set belong to the set's device)."""
    one, Xt, _ = truth_bcm(gp_mod, "se_5x261p2")
    two, _, _ = truth_bcm(gp_mod, "se_5x261p2", devices=[0, 0])
    try:
        want = one.predict_grad(Xt, combine="rbcm")
        two.predict_grad(Xt, combine="rbcm")
        two.expert(3).set_profiling(3)                                      # set 1 goes expert by expert, set 0 as a group
        assert all_same(two.predict_grad(Xt, combine="rbcm"), want) and two.predict_grad_form == 1
        two.expert(0).set_profiling(3)                                      # both sets expert by expert
        assert all_same(two.predict_grad(Xt, combine="rbcm"), want) and two.predict_grad_form == 1
        assert all_same(two.predict_grad(Xt), one.predict_grad(Xt))
    finally:
        one.close()
        two.close()


def test_stale_experts_are_refreshed(gp_mod):
    b = ragged_bcm(gp_mod)
    try:
        Xt = synth(65, 3, seed=7, scale=3.0)[0]
        b.predict_grad(Xt)
        b.set_BCM_log_hyperparam(np.array(tpm.HP) + 0.1)
        stale = b.predict_grad(Xt, combine="rbcm")                         # right after: one evaluation of the model first
        assert b.predict_grad_form == 2
        assert all_same(b.predict_grad(Xt, combine="rbcm"), stale)        # on valid experts
        assert all_same(stale, per_expert(gp_mod, b, Xt, "rbcm"))
    finally:
        b.close()


# ------------------------------------------------------------------ a world of one through the communicator
def hold_communicator(gp_mod, oracle, comm, name, reports=True):
    """Every mode of the communicator form on a truth case: the bits of b.predict_grad where there is no transcendental,
    rbcm's mean / var against the host's at truth_poe_modes' yardstick, and every mode's gradients against the truth."""
    c = tpg.bcm_case(oracle, name)
    pc = tpm.case(oracle, name, tpg.BCM_NT)
    b, Xt, cov = truth_bcm(gp_mod, name)
    K, d, F = len(b.rows), Xt.shape[1], tpg.factor(cov)
    rep = Report("grad-bcm-comm/%s" % name, cov)
    try:
        for combine in MODES:
            mode = "reference" if combine is None else combine
            host = b.predict_grad(Xt, combine=combine, with_noise=False)
            got = comm.predict_grad_allgather(b, K, K, Xt, d, combine=combine, with_noise=False)
            assert b.predict_grad_form == 2
            t = c["modes"][mode]
            e = tpg.errors(got[2], got[3], t["tdm"], t["tdv"])
            for q in tpg.QUANTITIES:
                rep.add("%s_%s" % (mode, q), e[q], t["noise"][q], t["floor"][q], F)
            if combine in BITWISE:
                assert all_same(got, host), mode
            else:
                fl = tpm.floors(pc, mode)
                rep.add("rbcm_host_vs_device_mean", np.max(np.abs(got[0] - host[0])), pc["yard"][mode]["mean"], fl["mean"], F)
                rep.add("rbcm_host_vs_device_var", np.max(np.abs(got[1] - host[1])), pc["yard"][mode]["var"], fl["var"], F)
            if combine is not None:                                         # the noise term: sn2 added to the variance alone
                noisy = comm.predict_grad_allgather(b, K, K, Xt, d, combine=combine, with_noise=True)
                assert same_bits(noisy[0], got[0]) and same_bits(noisy[1], got[1] + b.prior_scalars()[1])
                assert same_bits(noisy[2], got[2]) and same_bits(noisy[3], got[3])
            nov = comm.predict_grad_allgather(b, K, K, Xt, d, combine=combine, with_noise=False, want_var_grad=False)
            assert nov[3] is None and all(same_bits(a, w) for a, w in zip(nov[:3], got[:3]))
    finally:
        b.close()
    rep.check()


@pytest.mark.parametrize("name", ("se_3x300", "ard_3x300"))
def test_communicator_world_of_one(gp_mod, oracle, comm1, name):
    hold_communicator(gp_mod, oracle, comm1, name)


def test_communicator_ragged_and_null_mean_var(gp_mod, comm1):
    """The ragged experts at a ragged test tile, and mean / var NULL: accepted, the gradients' bits unchanged."""
    b = ragged_bcm(gp_mod)
    try:
        Xt = synth(65, 3, seed=7, scale=3.0)[0]
        for combine in BITWISE:
            assert all_same(comm1.predict_grad_allgather(b, 3, 3, Xt, 3, combine=combine), b.predict_grad(Xt, combine=combine))
        want = b.predict_grad(Xt, combine="bcm")
        dm, dv = np.empty((65, 3)), np.empty((65, 3))
        sf2, sn2 = b.prior_scalars()
        capi.check(capi.lib().cugp_bcm_predict_grad_allgather(b._h, comm1._h, 3, 3, capi.ptr(Xt), 65, 3, capi.CUGP_COMBINE_BCM,
                                                              1, sf2, sn2, None, None, capi.ptr(dm), capi.ptr(dv)))
        assert same_bits(dm, want[2]) and same_bits(dv, want[3])
    finally:
        b.close()


def test_status_protocol_then_recovery(gp_mod, comm1):
    """Argument paths only: an expert count that is not the one nexperts implies, and a d that is not the BCM's."""
    L = capi.lib()
    b = ragged_bcm(gp_mod)
    try:
        nt, d = 65, 3
        Xt = synth(nt, d, seed=7, scale=3.0)[0]
        out = [np.zeros(nt), np.zeros(nt), np.zeros((nt, d)), np.zeros((nt, d))]
        sf2, sn2 = b.prior_scalars()

        def call(per, nexp, d_=d):
            for a in out:
                a[:] = 0.0
            return L.cugp_bcm_predict_grad_allgather(b._h, comm1._h, per, nexp, capi.ptr(Xt), nt, d_, 0, 1, sf2, sn2,
                                                     *[capi.ptr(a) for a in out])
        for per, nexp in ((4, 4), (2, 2)):                                  # the BCM holds 3
            assert call(per, nexp) == capi.CUGP_ERR_INVALID
            assert all(np.all(np.isnan(a)) for a in out), (per, nexp)
            err = L.cugp_last_error()
            assert b"cugp_bcm_predict_grad_allgather" in err and b"rank 0" in err
        assert call(3, 3, d_=2) == capi.CUGP_ERR_INVALID                    # refused before any collective: outputs untouched
        assert b"cugp_bcm_predict_grad_allgather" in L.cugp_last_error() and all(np.all(a == 0.0) for a in out)
        assert all_same(comm1.predict_grad_allgather(b, 3, 3, Xt, d, combine="poe"), b.predict_grad(Xt, combine="poe"))
    finally:
        b.close()


def test_one_rank_rccl_communicator(tmp_path):
    """The same through a one-rank RCCL communicator (ncclAllGather of the one block), in a child process: b.predict_grad's
    bits for the rules without a transcendental, and for rbcm the bits of the world of one without a communicator."""
    script = tmp_path / "rank0.py"
    script.write_text(textwrap.dedent('''
        import os, sys
        import numpy as np
        import torch                                   # (its RCCL is the copy the library's dlopen then finds)
        sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tests"))
        import cugp_amd.gp as gp
        import test_gpu_bcm_predict_grad_batched as T
        comm = gp.Comm(gp.Comm.unique_id(), 0, 1, 0)
        b = T.ragged_bcm(gp)
        Xt = T.synth(65, 3, seed=7, scale=3.0)[0]
        for combine in T.BITWISE:
            got = comm.predict_grad_allgather(b, 3, 3, Xt, 3, combine=combine)
            assert T.all_same(got, b.predict_grad(Xt, combine=combine)), combine
        plain = gp.Comm(None, 0, 1, 0)                 # rbcm: the device's own log on both sides -- bit for bit
        got = comm.predict_grad_allgather(b, 3, 3, Xt, 3, combine="rbcm")
        assert T.all_same(got, plain.predict_grad_allgather(b, 3, 3, Xt, 3, combine="rbcm"))
        plain.close()
        nov = comm.predict_grad_allgather(b, 3, 3, Xt, 3, combine="rbcm", want_var_grad=False)
        assert nov[3] is None and T.same_bits(nov[2], got[2])
        b.close(); comm.close()
        print("GRAD_SINGLE_RANK_OK")
        ''' % (ROOT, ROOT)))
    out = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=300, env=dict(os.environ))
    errs = [ln for ln in out.stderr.splitlines() if "Error" in ln or "assert" in ln or "File " in ln]
    assert out.returncode == 0 and "GRAD_SINGLE_RANK_OK" in out.stdout, (out.stdout[-2000:], errs[-20:])


# ------------------------------------------------------------------ existing results untouched
def test_existing_results_untouched(gp_mod, comm1):
    """cugp_bcm_predict, cugp_bcm_predict_mode and cugp_bcm_loglik_grad before and after the new calls on the same BCM, and
    on a plain isotropic BCM in the same process: the same bits."""
    b, Xt, _ = truth_bcm(gp_mod, "ard_3x300")
    other = ragged_bcm(gp_mod)
    Xo = synth(65, 3, seed=7, scale=3.0)[0]
    try:
        def snapshot():
            ll, g, per = b.loglik_grad()
            lo, go, _ = other.loglik_grad()
            return [np.array([ll, lo]), g, per, go, *b.predict(Xt), *b.predict(Xt, combine="rbcm"), *other.predict(Xo),
                    *other.predict(Xo, combine="gpoe")]
        before = snapshot()
        for combine in (None, "rbcm"):
            b.predict_grad(Xt, combine=combine)
            comm1.predict_grad_allgather(b, 3, 3, Xt, 3, combine=combine)
        after = snapshot()
        assert all(same_bits(x, y) for x, y in zip(before, after))
    finally:
        b.close()
        other.close()
