"""The combination rules on latent expert distributions (include/cugp.h: CUGP_COMBINE_*) on the GPU, held to fp64
rounding against the longdouble truth of tests/truth_poe_modes.py:

    err <= F_family max(yardstick, floor)

yardstick: the family's fp64 evaluator per expert, combined in fp64, over the data as given and 7 permutations; floor: 4
ulp of the quantity's scale; F: truth.F / F_MATERN / F_ARD -- tests/test_truth_poe_modes_cpu.py shows on the CPU that the
stand-in stays below half of them on this very case list and that three mutated formulations exceed the bound.

Shapes: truth.WIDE_BCM's 3 x 300 rows and the uneven 5-expert split of 5 * 261 + 2 rows (experts padded to a common
size), d = 3; one expert of 257 rows; 1, 255, 256 and 257 test points (the 256-thread boundary of k_poe_reduce_mode and the
second 128-row test tile), 257 once more in passes of 64 (tuning key 19); one Matern-5/2 and one ARD BCM at 200 points.
Every figure is printed before it is asserted ("ACC <case> <quantity> err noise floor ratio"; run with -s).  One process,
one device; nothing outside the tree is read.
"""
import ctypes as C

import numpy as np
import pytest

import truth
import truth_poe_modes as tp
from accuracy import Report
from cugp_amd import capi
from cugp_amd.capi import ptr

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not truth.EXTENDED, reason="numpy.longdouble is not an extended-precision type here")]

LD = truth.LD
TUNE_PRED_CHUNK = 19                                                # kernels.h TUNE_*
BITWISE = ("poe", "gpoe", "bcm")                                    # no transcendental: host and device agree bit for bit


@pytest.fixture(scope="module")
def gp_mod():
    import cugp_amd.gp as gp
    return gp


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def make_bcm(gp_mod, c, name):
    family = tp.CASES[name][0]
    b = gp_mod.BCM.split(c["X"], c["y"], c["K"], kernel="se" if family == "ard" else family, ard=family == "ard")
    assert b.rows == [r for _, r in truth.bcm_rows(len(c["y"]), c["K"])]
    b.set_BCM_log_hyperparam(c["cov"].hp)
    return b


def has_inverse(b):
    fn = capi.lib().cugp_has_inverse                                # csrc/group.h: the handle holds L^-1, K^-1, alpha
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p]
    return [fn(b.expert(k)._h) for k in range(len(b.rows))]


def existing_results(b, comm, Xt):
    K = len(b.rows)
    return (b.compute_BCM_test_means_and_var(Xt) + comm.predict_allgather(b, K, K, Xt)
            + b.expert(K - 1).compute_test_means_and_variances(None, None, Xt))


def host_rows(b, Xt):
    """The experts' latent rows fetched through cugp_predict_latent, formed as the device forms them."""
    rows = np.empty((len(b.rows), 2, len(Xt)))
    for k in range(len(b.rows)):
        m, v = b.expert(k).predict_latent(Xt)
        rows[k, 0] = 1.0 / v
        rows[k, 1] = (1.0 / v) * m
    return rows


def hold_modes(rep, c, tag, results):
    """results: {mode: (mean, var_f)} against the truth of the case at the bound."""
    for mode in tp.MODES:
        e = truth.errors_pred(*results[mode], *c["modes"][mode])
        fl = tp.floors(c, mode)
        for q in ("mean", "var"):
            rep.add("%s%s_%s" % (tag, mode, q), e[q], c["yard"][mode][q], fl[q], tp.factor(c["cov"]))


@pytest.mark.parametrize("name,nt", tp.CASE_LIST)
def test_modes_case(gp_mod, oracle, name, nt):
    """One case of the list: cugp_predict_latent of every expert, cugp_bcm_predict_mode and
    cugp_bcm_predict_allgather_mode (a world of one, a communicator without id) in all four modes against the truth; the
    two device reductions agree bit for bit; the host's cugp_poe_combine on the fetched rows agrees bit for bit for poe,
    gpoe and bcm and within the bound for rbcm; with_noise adds exactly sn2; and cugp_bcm_predict,
    cugp_bcm_predict_allgather and cugp_predict return the same bits before and after all of it, the experts' inverse
    state unchanged."""
    c = tp.case(oracle, name, nt)
    Xt, K, cov = c["Xt"], c["K"], c["cov"]
    F = tp.factor(cov)
    rep = Report("%s/nt%d" % (name, nt), cov)
    b = make_bcm(gp_mod, c, name)
    comm = gp_mod.Comm(None, 0, 1, 0)
    try:
        sf2, sn2 = b.prior_scalars()
        before = existing_results(b, comm, Xt)
        inv_before = has_inverse(b)
        assert inv_before == [1] * K
        # ---- every expert's latent prediction
        for k in range(K):
            e = b.expert(k)
            mn, vn = e.compute_test_means_and_variances(None, None, Xt)
            ml, vl = e.predict_latent(Xt)
            assert same_bits(ml, mn), k                             # cugp_predict's mean, bit for bit
            err = truth.errors_pred(ml, vl, *c["experts"][k])
            fl = tp.expert_floors(c, k)
            for q in ("mean", "var"):
                rep.add("latent%d_%s" % (k, q), err[q], c["yard"]["experts"][k][q], fl[q], F)
            assert np.all(vl <= vn)
        # ---- the two device paths, the host twin
        rows = host_rows(b, Xt)
        dev, gat = {}, {}
        for mode in tp.MODES:
            dev[mode] = b.predict(Xt, combine=mode, with_noise=False)
            gat[mode] = comm.predict_allgather(b, K, K, Xt, combine=mode, with_noise=False, sf2=sf2, sn2=sn2)
            assert same_bits(dev[mode][0], gat[mode][0]) and same_bits(dev[mode][1], gat[mode][1]), mode
            mn, vn = b.predict(Xt, combine=mode, with_noise=True)
            assert same_bits(mn, dev[mode][0]) and same_bits(vn, dev[mode][1] + sn2), mode
            hm, hv = gp_mod.poe_combine(rows, mode, sf2, sn2, with_noise=False)
            if mode in BITWISE:
                assert same_bits(hm, dev[mode][0]) and same_bits(hv, dev[mode][1]), mode
            else:
                fl = tp.floors(c, mode)
                rep.add("rbcm_host_vs_device_mean", np.max(np.abs(hm - dev[mode][0])), c["yard"][mode]["mean"], fl["mean"], F)
                rep.add("rbcm_host_vs_device_var", np.max(np.abs(hv - dev[mode][1])), c["yard"][mode]["var"], fl["var"], F)
        hold_modes(rep, c, "", dev)
        if K == 1:                                                  # poe, gpoe, bcm of one expert: the expert itself
            ml, vl = b.expert(0).predict_latent(Xt)
            for mode in BITWISE:
                fl = tp.floors(c, mode)
                rep.add("k1_%s_mean" % mode, np.max(np.abs(dev[mode][0] - ml)), c["yard"][mode]["mean"], fl["mean"], F)
                rep.add("k1_%s_var" % mode, np.max(np.abs(dev[mode][1] - vl)), c["yard"][mode]["var"], fl["var"], F)
        # ---- the existing calls: the same bits as before, the experts' state untouched
        after = existing_results(b, comm, Xt)
        assert all(same_bits(x, y) for x, y in zip(before, after))
        assert has_inverse(b) == inv_before
    finally:
        comm.close()
        b.close()
    rep.check()


@pytest.mark.parametrize("name", ["se_3x300", "se_5x261p2"])
def test_passes_and_repeats(gp_mod, oracle, name):
    """257 test points in passes of 64 (tuning key 19 = 1: more than one pass, t0 > 0) give the bits of the default single
    pass in every mode, through both calls; ten repeated calls give identical bits."""
    nt = 257
    c = tp.case(oracle, name, nt)
    Xt, K = c["Xt"], c["K"]
    b = make_bcm(gp_mod, c, name)
    comm = gp_mod.Comm(None, 0, 1, 0)
    rep = Report("%s/nt%d/chunk64" % (name, nt), c["cov"])
    try:
        sf2, sn2 = b.prior_scalars()
        whole = {mode: b.predict(Xt, combine=mode, with_noise=False) for mode in tp.MODES}
        try:
            capi.check(capi.lib().cugp_set_tuning(TUNE_PRED_CHUNK, 1))
            dev = {mode: b.predict(Xt, combine=mode, with_noise=False) for mode in tp.MODES}
            gat = {mode: comm.predict_allgather(b, K, K, Xt, combine=mode, with_noise=False, sf2=sf2, sn2=sn2)
                   for mode in tp.MODES}
        finally:
            capi.check(capi.lib().cugp_set_tuning(TUNE_PRED_CHUNK, 0))     # the built-in default
        for mode in tp.MODES:
            for r in (dev, gat):
                assert same_bits(r[mode][0], whole[mode][0]) and same_bits(r[mode][1], whole[mode][1]), mode
        hold_modes(rep, c, "", dev)
        for mode in tp.MODES:
            for _ in range(10):
                m, v = b.predict(Xt, combine=mode, with_noise=False)
                assert same_bits(m, whole[mode][0]) and same_bits(v, whole[mode][1]), mode
    finally:
        comm.close()
        b.close()
    rep.check()


@pytest.mark.parametrize("name", ["se_3x300", "se_5x261p2", "matern52_3x300", "ard_3x300"])
def test_far_from_the_data(gp_mod, name):
    """A test point 1e3 x the input scale away: every expert returns its prior there (the cross-covariances underflow to
    exact zeros in fp64 and are below 1e-2000 in any precision, so the true latent variance of every expert is sf2 and the
    true combinations are sf2 for bcm, rbcm and gpoe and sf2 / K for poe -- the defect of the plain product).  Held to F x the floor, 4 ulp of
    sf2 + sn2: no yardstick can be larger than the bound's own."""
    X, y, _, cov, K = tp.inputs(name, 1)
    c = dict(X=X, y=y, K=K, cov=cov)
    Xt = np.full((1, tp.D), 1e3 * tp.SCALE)
    b = make_bcm(gp_mod, c, name)
    try:
        sf2, sn2 = b.prior_scalars()
        bound = tp.factor(cov) * truth.U4 * (sf2 + sn2)
        for mode, want in (("bcm", sf2), ("rbcm", sf2), ("gpoe", sf2), ("poe", sf2 / K)):
            m, v = b.predict(Xt, combine=mode, with_noise=False)
            print("FAR %-16s %-4s var_f %.17g  want %.17g  err %.2e  bound %.2e" % (name, mode, v[0], want, abs(v[0] - want), bound))
            assert abs(v[0] - want) <= bound, (mode, v[0], want)
            assert m[0] == 0.0
        _, v = b.compute_BCM_test_means_and_var(Xt)                 # today's noisy product: (sf2 + sn2) / K
        assert abs(v[0] - (sf2 + sn2) / K) <= bound
    finally:
        b.close()


def test_sharded_library_against_torch_form(gp_mod, oracle, monkeypatch):
    """ShardedBCM at one rank: the library form (cugp_bcm_predict_allgather_mode, the rule on the device) against the
    torch form (predict_latent per expert, cugp_poe_combine on the host): bit for bit for poe, gpoe and bcm, within the
    bound for rbcm; combine=None keeps today's bits in both."""
    import torch
    from cugp_amd.bcm import ShardedBCM
    monkeypatch.delenv("CUGP_BCM_EXCHANGE", raising=False)
    name, nt = "se_3x300", 257
    c = tp.case(oracle, name, nt)
    Xt, K = c["Xt"], c["K"]
    experts = [(c["X"][o: o + r], c["y"][o: o + r]) for o, r in truth.bcm_rows(len(c["y"]), K)]
    lib = ShardedBCM(experts, rank=0, world=1, device=0, comm_device=torch.device("cuda", 0))
    tor = ShardedBCM(experts)
    rep = Report("%s/nt%d/sharded" % (name, nt), c["cov"])
    try:
        assert lib.exchange_form == "library" and tor.exchange_form != "library"
        res = {}
        for sb, form in ((lib, "library"), (tor, "torch")):
            sb.set_loghyper(c["cov"].hp)
            sb.loglik_grad()                    # (the torch form predicts expert by expert: bring all up to date as a group)
            res[form] = {mode: sb.predict(Xt, combine=mode, with_noise=False) for mode in tp.MODES}
            assert sb.predict_form == form
            res[form][None] = sb.predict(Xt)
            assert sb.predict_form == form
        assert same_bits(res["library"][None][0], res["torch"][None][0])
        assert same_bits(res["library"][None][1], res["torch"][None][1])
        for mode in BITWISE:
            assert same_bits(res["library"][mode][0], res["torch"][mode][0]), mode
            assert same_bits(res["library"][mode][1], res["torch"][mode][1]), mode
        fl = tp.floors(c, "rbcm")
        F = tp.factor(c["cov"])
        for i, q in enumerate(("mean", "var")):
            rep.add("rbcm_library_vs_torch_" + q, np.max(np.abs(res["library"]["rbcm"][i] - res["torch"]["rbcm"][i])),
                    c["yard"]["rbcm"][q], fl[q], F)
        hold_modes(rep, c, "library_", res["library"])
        hold_modes(rep, c, "torch_", res["torch"])
    finally:
        lib.close()
        tor.close()
    rep.check()


def test_refusals_leave_the_model_usable(gp_mod, oracle):
    """An unknown mode, nt <= 0 and null pointers are CUGP_ERR_INVALID before any device call, on null handles and on a
    live BCM, which predicts the same bits afterwards; unknown names raise ValueError."""
    lib = capi.lib()
    c = tp.case(oracle, "se_3x300", 1)
    Xt, K = c["Xt"], c["K"]
    m, v = np.empty(1), np.empty(1)
    null = C.c_void_p()
    assert lib.cugp_bcm_predict_mode(null, ptr(Xt), 1, 0, 1, ptr(m), ptr(v)) == capi.CUGP_ERR_INVALID
    assert lib.cugp_predict_latent(null, ptr(Xt), 1, ptr(m), ptr(v)) == capi.CUGP_ERR_INVALID
    b = make_bcm(gp_mod, c, "se_3x300")
    comm = gp_mod.Comm(None, 0, 1, 0)
    try:
        sf2, sn2 = b.prior_scalars()
        want = b.predict(Xt, combine="rbcm")
        for mode in (-1, 4):
            assert lib.cugp_bcm_predict_mode(b._h, ptr(Xt), 1, mode, 1, ptr(m), ptr(v)) == capi.CUGP_ERR_INVALID
            assert lib.cugp_bcm_predict_allgather_mode(b._h, comm._h, K, K, ptr(Xt), 1, mode, 1, sf2, sn2, ptr(m),
                                                       ptr(v)) == capi.CUGP_ERR_INVALID
        assert lib.cugp_bcm_predict_mode(b._h, ptr(Xt), 0, 0, 1, ptr(m), ptr(v)) == capi.CUGP_ERR_INVALID
        assert lib.cugp_bcm_predict_mode(b._h, None, 1, 0, 1, ptr(m), ptr(v)) == capi.CUGP_ERR_INVALID
        assert lib.cugp_bcm_predict_mode(b._h, ptr(Xt), 1, 0, 1, None, ptr(v)) == capi.CUGP_ERR_INVALID
        assert lib.cugp_bcm_predict_allgather_mode(b._h, None, K, K, ptr(Xt), 1, 0, 1, sf2, sn2, ptr(m), ptr(v)) == \
            capi.CUGP_ERR_INVALID
        assert lib.cugp_predict_latent(b.expert(0)._h, ptr(Xt), 0, ptr(m), ptr(v)) == capi.CUGP_ERR_INVALID
        with pytest.raises(ValueError):
            b.predict(Xt, combine="robust")
        with pytest.raises(ValueError):
            comm.predict_allgather(b, K, K, Xt, combine="robust")
        got = b.predict(Xt, combine="rbcm")
        assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
    finally:
        comm.close()
        b.close()


def test_several_device_sets(gp_mod, oracle):
    """A BCM over two device sets of one process (the same GPU listed twice): the experts' latent predictions go to pinned
    host memory and cugp_poe_combine reduces them: all four modes against the truth at the bound, and poe, gpoe and bcm
    bit for bit against cugp_poe_combine on the rows fetched from the same experts."""
    name, nt = "se_5x261p2", 257
    c = tp.case(oracle, name, nt)
    Xt, K = c["Xt"], c["K"]
    two = gp_mod.BCM.split(c["X"], c["y"], K, devices=[0, 0])
    rep = Report("%s/nt%d/two-sets" % (name, nt), c["cov"])
    try:
        two.set_BCM_log_hyperparam(c["cov"].hp)
        res = {mode: two.predict(Xt, combine=mode, with_noise=False) for mode in tp.MODES}
        hold_modes(rep, c, "", res)
        rows = host_rows(two, Xt)
        sf2, sn2 = two.prior_scalars()
        for mode in BITWISE:
            hm, hv = gp_mod.poe_combine(rows, mode, sf2, sn2, with_noise=False)
            assert same_bits(hm, res[mode][0]) and same_bits(hv, res[mode][1]), mode
    finally:
        two.close()
    rep.check()
