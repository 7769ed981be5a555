"""GPU tests of the ARD product of experts: ARD handles as the experts of a group of shared launches (batched
k_build, k_cross, k_trace <true, KERNEL_SE>, k_finalize_ard), rows {LL, g[nh]} through cugp_bcm_*_ard, the optimiser, the
exchange.

Accuracy is held to fp64 rounding against the extended-precision truth, through tests/truth_ard_bcm.py and the Report of
tests/accuracy.py:

    err_gpu(q) <= F_ARD * max(noise(q), floor(q))

with the yardstick from the CPU oracle's product of experts on the scaled copy X / l and F_ARD = 32 as it stands
(tests/test_truth_ard_bcm_cpu.py: the stand-in asks for 8 at most) -- never from the GPU.  Everything else is bit
equality.  Every figure is printed before it is asserted (run with -s).  One process, one device; two tests start one
fresh child process each (a process group and "no ARD BCM has lived here yet" are process-global state).
"""
import ctypes as C
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import truth
import truth_ard_bcm as tab
from accuracy import Report
from conftest import ROOT, synth
from cugp_amd import capi

pytestmark = pytest.mark.gpu
extended = pytest.mark.skipif(not truth.EXTENDED, reason="numpy.longdouble is not an extended-precision type here")

LD = truth.LD
INV = capi.CUGP_ERR_INVALID


@pytest.fixture(scope="module")
def gp_mod():
    import cugp_amd.gp as gp
    return gp


@pytest.fixture(scope="module")
def comm1(gp_mod):
    c = gp_mod.Comm(None, 0, 1, 0)            # a world of one without an id: no RCCL
    yield c
    c.close()


def same(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


def bcm_of(gp_mod, X, y, rows, hp, devices=None):
    b = gp_mod.BCM(rows, X.shape[1], 0, devices, ard=True)
    off = 0
    for k, n in enumerate(rows):
        b.set_expert_data(k, X[off: off + n], y[off: off + n])
        off += n
    b.set_BCM_log_hyperparam(hp)
    return b


def hold(rep, tag, c, b):
    """One evaluation and one prediction of the ARD BCM b against the case's truth."""
    ll, g, per = b.loglik_grad()
    m, v = b.compute_BCM_test_means_and_var(c["Xt"])
    assert g.shape == (b.nh,) and per.shape == (len(c["parts"]),)
    rep.add_all(tag, tab.bcm_errors(c, ll, g, m, v), c["noise"], c["floor"])
    return ll, g, m, v


# ------------------------------------------------------------------ 1. accuracy
@extended
@pytest.mark.parametrize("name", list(tab.CASES))
def test_accuracy(gp_mod, oracle, name):
    """LL, the worst g_c, gf, gn, means and variances of BCM.split(X, y, K, ard=True); again after theta moved away and
    back (the second and third evaluation replay the group's captured graph: the new length scales travel by the copy
    node at its head)."""
    c = tab.case(oracle, name)
    X, y, cov, K = c["X"], c["y"], c["cov"], len(c["parts"])
    b = gp_mod.BCM.split(X, y, K, ard=True)
    assert b.ard and b.nh == X.shape[1] + 2 and b.kernel == "se"
    b.set_BCM_log_hyperparam(cov.hp)
    assert np.array_equal(b.get_loghyperparam(), cov.hp)
    rep = Report(name, cov)
    first = hold(rep, "", c, b)
    moved = np.array(cov.hp)
    moved[0] += 0.25                                              # ONE length scale
    b.set_BCM_log_hyperparam(moved)
    away = b.loglik_grad()
    assert away[0] != first[0] and not np.array_equal(away[1], first[1])
    b.set_BCM_log_hyperparam(cov.hp)
    again = hold(rep, "replay_", c, b)
    b.close()
    assert all(same(p, q) for p, q in zip(first, again))
    rep.check()


# ------------------------------------------------------------------ 2. the batched kernels run
def test_group_of_ard_handles(gp_mod):
    """cugp_group_create takes three ARD handles (300 rows, d = 17) and cugp_group_eval with the gradient returns
    CUGP_OK -- the shared launches ran, not the CUGP_ERR_INVALID that sends a BCM to one stream per expert.  The rows
    are then the single handles' to 1e-11 (a group takes its inverse in other blocks: not the same bits).  A list of
    ARD and isotropic handles is CUGP_ERR_INVALID."""
    L = capi.lib()
    L.cugp_group_create.restype = C.c_int
    L.cugp_group_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_void_p)]
    L.cugp_group_eval.restype = C.c_int
    L.cugp_group_eval.argtypes = [C.c_void_p, C.c_int, capi._dp, capi._dp]
    L.cugp_group_destroy.restype = None
    L.cugp_group_destroy.argtypes = [C.c_void_p]
    n, d, k = 300, 17, 3
    hp = np.linspace(0.7, 1.9, d).tolist() + [0.3, -0.8]
    hs, alone = [], []
    for i in range(k):
        X, y = synth(n, d=d, seed=40 + i, scale=1.8)
        g = gp_mod.Covsum(n, d, ard=True)
        g.set_overlap(False)                                      # as the experts of a BCM
        g.set_data(X, y)
        g.set_loghyperparam(hp)
        alone.append(g.loglik_grad())
        g.set_data(X, y)                                          # (nothing valid: the group evaluates)
        hs.append(g)
    arr = (C.c_void_p * k)(*[g.handle.value for g in hs])
    gr = C.c_void_p()
    assert L.cugp_group_create(arr, k, C.byref(gr)) == capi.CUGP_OK, L.cugp_last_error()
    ll, gv = np.zeros(k), np.zeros(k * (d + 2))
    assert L.cugp_group_eval(gr, 1, capi.ptr(ll), capi.ptr(gv)) == capi.CUGP_OK, L.cugp_last_error()
    for i in range(k):
        gi = gv[(d + 2) * i: (d + 2) * (i + 1)]
        assert abs(ll[i] - alone[i][0]) <= 1e-11 * abs(alone[i][0]), (i, ll[i], alone[i][0])
        assert np.max(np.abs(gi - alone[i][1])) <= 1e-11 * np.max(np.abs(alone[i][1])), (i, gi, alone[i][1])
    assert L.cugp_group_eval(gr, 0, capi.ptr(ll), None) == capi.CUGP_OK, L.cugp_last_error()      # LL only
    for i in range(k):
        assert abs(ll[i] - alone[i][0]) <= 1e-11 * abs(alone[i][0]), (i, ll[i], alone[i][0])
    L.cugp_group_destroy(gr)
    iso = gp_mod.Covsum(n, d)
    mixed = (C.c_void_p * 2)(hs[0].handle.value, iso.handle.value)
    gr2 = C.c_void_p()
    assert L.cugp_group_create(mixed, 2, C.byref(gr2)) == INV
    assert b"ARD and isotropic" in L.cugp_last_error()
    mixed = (C.c_void_p * 2)(iso.handle.value, hs[0].handle.value)
    assert L.cugp_group_create(mixed, 2, C.byref(gr2)) == INV
    iso.close()
    for g in hs:
        g.close()


# ------------------------------------------------------------------ 3. indexing
def test_rows_follow_their_experts(gp_mod):
    """Three experts with the same data: three rows of identical bits.  Two experts' data swapped: their rows swap, the
    third stays.  Ten evaluations: identical bits.  loglik_grad is the expert-order sum of loglik_grad_rows."""
    n, d = 150, 5
    hp = [0.9, 0.5, 1.3, 0.7, 1.1, 0.2, -1.0]
    data = [synth(n, d=d, seed=60 + i, scale=3.0) for i in range(3)]

    def rows_of(order):
        b = gp_mod.BCM([n] * 3, d, 0, ard=True)
        for k, i in enumerate(order):
            b.set_expert_data(k, *data[i])
        b.set_BCM_log_hyperparam(hp)
        r = b.loglik_grad_rows()
        return b, r
    b, r = rows_of([0, 0, 0])
    assert r.shape == (3, 1 + d + 2) and np.all(np.isfinite(r))
    assert same(r[0], r[1]) and same(r[0], r[2])
    b.close()
    b, r012 = rows_of([0, 1, 2])
    assert not same(r012[0], r012[1]) and same(r012[0], r[0])
    b2, r210 = rows_of([2, 1, 0])
    assert same(r210[0], r012[2]) and same(r210[2], r012[0]) and same(r210[1], r012[1])
    b2.close()
    ll0, g0, per0 = b.loglik_grad()
    for _ in range(9):
        for k in range(3):
            b.set_expert_data(k, *data[k])                        # invalidates what the experts hold: a full evaluation
        ll, g, per = b.loglik_grad()
        assert ll == ll0 and same(g, g0) and same(per, per0)
        assert same(b.loglik_grad_rows(), r012)
    sll, sg = 0.0, None
    for k in range(3):
        sll = sll + r012[k, 0]
        sg = r012[k, 1:].copy() if k == 0 else sg + r012[k, 1:]
    assert ll0 == sll and same(g0, sg) and same(per0, r012[:, 0])
    b.close()


# ------------------------------------------------------------------ 4. d across the feature-chunk boundary
CHUNK_TOL = 1e-11      # tests/test_gpu_ard.py::test_feature_chunks_against_the_standin: stand-in and GPU are each within ~5e-13
                       # of the truth on inputs this small, so 1e-11 leaves a factor of ten


@pytest.mark.parametrize("d", [1, 16, 17, 33])
def test_feature_chunks_against_the_standin(gp_mod, d):
    """A wiring test of the batched trace and build: 2 x 130 rows, LL and every gradient component against the CPU
    stand-in at 1e-11 relative (gradient: to max|g|)."""
    X, y = synth(260, d=d, seed=100 + d, scale=2.0)
    hp = np.linspace(0.8, 1.6, d).tolist() + [0.3, -0.8]
    cov = truth.ARD(hp)
    sll, sg, _, _ = truth.standin_bcm(cov, X, y, 2, X[:1])
    b = gp_mod.BCM.split(X, y, 2, ard=True)
    b.set_BCM_log_hyperparam(hp)
    ll, gr, _ = b.loglik_grad()
    b.close()
    el, eg = abs(ll - sll) / abs(sll), np.max(np.abs(gr - sg)) / np.max(np.abs(sg))
    print("d=%d: LL %.3e, gradient %.3e (of max|g|)" % (d, el, eg))
    assert el <= CHUNK_TOL and eg <= CHUNK_TOL, (d, el, eg)


# ------------------------------------------------------------------ 5. equal length scales meet the isotropic BCM
@extended
def test_equal_length_scales_meet_the_isotropic_bcm(gp_mod, oracle):
    """5x261p2_d3's data with all theta_c = 0.9: the ARD BCM and the isotropic BCM are each within their bound (F_ARD, F)
    of the same truth, so they differ by at most (F + F_ARD) yardsticks -- the isotropic BCM's own yardstick
    (truth.bcm_yardstick), as tests/test_gpu_ard.py holds the single handle.  The first gradient entry compared is
    sum_c g_c against g0."""
    X, y, Xt, _, K = tab.inputs("5x261p2_d3")
    d = X.shape[1]
    hp = [0.9, 0.2, -1.0]
    cov = truth.SE(hp)
    tb = truth.bcm_truth(X, y, cov, K, Xt)
    noise = truth.bcm_yardstick(oracle, cov, X, y, K, Xt, tb)[0]
    fl = truth.floors(cov, truth.scales(cov, tb["ll"], tb["grad"], tb["mean"]))
    bi = gp_mod.BCM.split(X, y, K)
    bi.set_BCM_log_hyperparam(hp)
    lli, gi, _ = bi.loglik_grad()
    mi, vi = bi.compute_BCM_test_means_and_var(Xt)
    bi.close()
    ba = gp_mod.BCM.split(X, y, K, ard=True)
    ba.set_BCM_log_hyperparam([hp[0]] * d + hp[1:])
    lla, ga, _ = ba.loglik_grad()
    ma, va = ba.compute_BCM_test_means_and_var(Xt)
    ba.close()
    e = truth.errors(cov, lla, [ga[:d].sum(), ga[d], ga[d + 1]], ma, va, LD(lli), gi.astype(LD), mi.astype(LD), vi.astype(LD))
    rep = Report("5x261p2_d3_iso", cov)
    rep.add_all("", e, noise, fl, truth.F + truth.F_ARD)
    rep.check()


# ------------------------------------------------------------------ 6. ungrouped and several sets
@extended
def test_ungrouped_experts_accuracy(gp_mod, oracle):
    """rows = [100, 400]: no common padded size, so no group -- every expert on its own stream through the single-handle
    kernels and the nh-wide fetch.  Held to the accuracy bound; rows, sums and the device rows agree bit for bit."""
    import torch
    d, hp = 3, [0.9, 0.3, 1.6, 0.2, -1.0]
    X, y = synth(500, d=d, seed=502, scale=4.0)
    cov = truth.ARD(hp)
    c = tab.case_at(oracle, cov, X, y, [(0, 100), (100, 400)], np.ascontiguousarray(truth.points(X, d, 4.0)))
    b = bcm_of(gp_mod, X, y, [100, 400], hp)
    rep = Report("100+400_d3", cov)
    ll, g, _, _ = hold(rep, "", c, b)
    r = b.loglik_grad_rows()
    assert ll == r[0, 0] + r[1, 0] and same(g, r[0, 1:] + r[1, 1:])
    t = torch.zeros((4, 1 + b.nh), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    b.loglik_grad_rows_device(t.data_ptr(), [3, 1])
    out = t.cpu().numpy()
    assert same(out[3], r[0]) and same(out[1], r[1]) and not out[0].any() and not out[2].any()
    b.close()
    rep.check()


@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0]])
def test_several_sets_equal_one(gp_mod, devices):
    """5 experts over a device list naming the same GPU two or three times (2 or 3 groups in flight at once, one of them
    possibly a group of one) are bit-equal to the single set: LL, gradient, rows, prediction, a 12-probe cg_solve."""
    X, y = synth(5 * 300 + 17, 6, seed=21, scale=2.5)
    hp = np.array([0.6, 0.8, 0.9, 1.0, 1.1, 1.3, 0.2, -1.0])
    ref = gp_mod.BCM.split(X, y, 5, ard=True)
    ref.set_BCM_log_hyperparam(hp)
    ll0, g0, per0 = ref.loglik_grad()
    rows0 = ref.loglik_grad_rows()
    Xt = X[:9] * 0.5 + 0.1
    m0, v0 = ref.compute_BCM_test_means_and_var(Xt)
    b = gp_mod.BCM.split(X, y, 5, devices=devices, ard=True)
    b.set_BCM_log_hyperparam(hp)
    for _ in range(2):                                            # the second pass replays the captured group graphs
        ll, g, per = b.loglik_grad()
        assert ll == ll0 and same(g, g0) and same(per, per0)
    assert same(b.loglik_grad_rows(), rows0)
    m, v = b.compute_BCM_test_means_and_var(Xt)
    assert same(m, m0) and same(v, v0)
    tr0 = ref.cg_solve(budget=12)
    tr = b.cg_solve(budget=12)
    assert tr.shape[1] == 9 and len(tr) >= 12 and same(tr, tr0)
    b.close()
    ref.close()


# ------------------------------------------------------------------ 7. prediction
def test_prediction_is_the_experts_product(gp_mod):
    """compute_BCM_test_means_and_var at 1, 64, 65 and 200 points equals the expert(k) views' predictions combined by
    poe_finish bit for bit; right after set_BCM_log_hyperparam (stale experts: one nh-wide evaluation of the whole model
    first) the bits are those with valid experts."""
    n, d, K = 200, 4, 3
    X, y = synth(K * n, d=d, seed=77, scale=3.0)
    hp = np.array([0.9, 0.5, 1.3, 0.7, 0.2, -1.0])
    b = gp_mod.BCM.split(X, y, K, ard=True)
    rng = np.random.default_rng(3)
    for i, nt in enumerate([1, 64, 65, 200]):
        Xt = rng.uniform(-3, 3, (nt, d))
        b.set_BCM_log_hyperparam(hp + 0.05 * i)
        m1, v1 = b.compute_BCM_test_means_and_var(Xt)             # stale
        assert np.all(np.isfinite(m1)) and np.all(v1 > 0)
        m2, v2 = b.compute_BCM_test_means_and_var(Xt)             # valid
        assert same(m1, m2) and same(v1, v2), nt
        sp, spm = np.zeros(nt), np.zeros(nt)
        for k in range(K):
            e = b.expert(k)
            assert e.ard and e.nh == d + 2 and np.array_equal(e.get_loghyperparam(), hp + 0.05 * i)
            mk, vk = e.compute_test_means_and_variances(None, None, Xt)
            inv = 1.0 / vk
            sp += inv
            spm += inv * mk
        m3, v3 = gp_mod.poe_finish(sp, spm)
        assert same(m3, m2) and same(v3, v2), nt
    b.close()


# ------------------------------------------------------------------ 8. the optimiser
def test_cg_solve_equals_the_python_driven_loop(gp_mod):
    """3 x 150 rows, d = 3, y a function of x_0 only.  b.cg_solve(budget=15) equals cugp_cg_minimize_n driven from Python
    on another BCM's loglik_grad probe for probe and bit for bit; the objective at the end point is below the start's (and
    is the lowest the run saw); theta_0 ends below theta_1 and theta_2 (the irrelevant dimensions' length scales grow)."""
    X, y = synth(450, d=3, seed=31, scale=3.0)
    start = [0.5, 0.5, 0.5, 0.5, 0.5]
    b = gp_mod.BCM.split(X, y, 3, ard=True)
    b.set_BCM_log_hyperparam(start)
    tr = b.cg_solve(budget=15)
    end = b.get_loghyperparam()
    f_end = -1.0 * b.loglik_grad()[0]                             # (the trace's last row is a probe, not the end point)
    b.close()
    b2 = gp_mod.BCM.split(X, y, 3, ard=True)

    def fn(th):
        b2.set_BCM_log_hyperparam(th)
        ll, g, _ = b2.loglik_grad()
        return -1.0 * ll, g
    th, tr2 = gp_mod.cg_minimize_n(fn, start, 15)
    b2.close()
    print("ARD BCM cg_solve: %d probes, f %.10g -> %.10g, end %s" % (len(tr), tr[0, -1], f_end, end))
    assert tr.shape[1] == 6 and len(tr) >= 15
    assert same(tr, tr2) and same(end, th)
    assert f_end < tr[0, -1] - 1.0 and f_end == np.min(tr[:, -1]), (tr[0, -1], f_end)
    assert end[0] < end[1] and end[0] < end[2], end


# ------------------------------------------------------------------ 9. the exchange
@pytest.mark.parametrize("rows", [[300], [300] * 3, [100, 400]], ids=["K1", "K3", "ungrouped"])
def test_world_of_one_exchange(gp_mod, comm1, rows):
    """loglik_grad_allgather(b, K, nh) equals loglik_grad_rows() bit for bit (rows packed on the device behind the
    evaluation: two strided copies per group, one per lone expert); predict_allgather (the batched k_cross<true, KERNEL_SE>) equals
    compute_BCM_test_means_and_var.  An isotropic BCM then uses the same communicator at its own width."""
    K, d = len(rows), 4
    X, y = synth(sum(rows), d=d, seed=11 + K, scale=3.0)
    hp = [0.9, 0.5, 1.3, 0.7, 0.2, -1.0]
    b = bcm_of(gp_mod, X, y, rows, hp)
    r0 = b.loglik_grad_rows()
    for _ in range(2):
        for k in range(K):
            b.set_expert_data(k, X[sum(rows[:k]): sum(rows[:k + 1])], y[sum(rows[:k]): sum(rows[:k + 1])])
        r = comm1.loglik_grad_allgather(b, K, b.nh)
        assert r.shape == (K, 1 + b.nh) and same(r, r0)
    r = comm1.loglik_grad_allgather(b, K + 2, b.nh)               # spare slots stay zero
    assert same(r[:K], r0) and not r[K:].any()
    Xt = np.random.default_rng(5).uniform(-3, 3, (130, d))
    b.set_BCM_log_hyperparam(np.array(hp) + 0.05)                 # stale experts
    m, v = comm1.predict_allgather(b, K, K, Xt)
    m0, v0 = b.compute_BCM_test_means_and_var(Xt)
    assert same(m, m0) and same(v, v0)
    b.close()
    bi = gp_mod.BCM(rows, d, 0)
    off = 0
    for k, n in enumerate(rows):
        bi.set_expert_data(k, X[off: off + n], y[off: off + n])
        off += n
    bi.set_BCM_log_hyperparam([0.9, 0.2, -1.0])
    ri = comm1.loglik_grad_allgather(bi, K + 2)
    assert ri.shape == (K + 2, 4) and same(ri[:K], bi.loglik_grad_rows()) and not ri[K:].any()
    bi.close()


@pytest.mark.parametrize("form", ["library", "allreduce"])
def test_sharded_ard_bcm_rccl_single_rank(tmp_path, form):
    """ShardedBCM(ard=True) under a one-rank NCCL (= RCCL) process group, as
    tests/test_gpu_bcm_predict_exchange.py::test_sharded_bcm_predict_rccl_single_rank: objective and prediction equal the
    single-process gp.BCM(ard=True) bit for bit, before and after a short cg_solve.  Child process: a process group is
    process-global state."""
    script = tmp_path / "rank0.py"
    script.write_text(textwrap.dedent('''
        import os, sys
        import numpy as np, torch, torch.distributed as dist
        sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tests"))
        from conftest import synth
        from cugp_amd.bcm import ShardedBCM
        import cugp_amd.gp as gp
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29543")
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
        X, y = synth(3 * 300, 5, seed=4, scale=3.0)
        experts = [(X[300 * k:300 * (k + 1)], y[300 * k:300 * (k + 1)]) for k in range(3)]
        b = ShardedBCM(experts, rank=0, world=1, device=0, comm_device=torch.device("cuda", 0), ard=True)
        assert b.exchange_form == %r, b.exchange_form
        assert b.ard and b.nh == 7
        b._allreduce = lambda t: (dist.all_reduce(t, op=dist.ReduceOp.SUM), t)[1]     # force the collective at 1 rank
        want = "library" if b.exchange_form == "library" else "torch"
        ref = gp.BCM([300, 300, 300], 5, 0, ard=True)
        for k, (Xk, yk) in enumerate(experts):
            ref.set_expert_data(k, Xk, yk)
        Xt = np.random.default_rng(1).uniform(-3, 3, (130, 5))
        b.set_loghyper([0.9, 0.5, 1.3, 0.7, 1.1, 0.2, -1.0])
        bits = lambda a: np.asarray(a, dtype=np.float64).view(np.uint64)
        for step in range(2):
            ll, g, per = b.loglik_grad()
            ref.set_BCM_log_hyperparam(b.hp)
            ll0, g0, per0 = ref.loglik_grad()
            assert ll == ll0 and np.array_equal(bits(g), bits(g0)) and np.array_equal(bits(per), bits(per0)), (step, ll, ll0)
            assert g.shape == (7,)
            m, v = b.predict(Xt)
            assert b.predict_form == want, (b.predict_form, want)
            m0, v0 = ref.compute_BCM_test_means_and_var(Xt)
            assert np.array_equal(bits(m), bits(m0)), (step, np.max(np.abs(m - m0)))
            assert np.array_equal(bits(v), bits(v0)), (step, np.max(np.abs(v - v0)))
            if step == 0:
                tr = b.cg_solve(budget=6)
                assert tr.shape[1] == 8
        b.close(); ref.close()
        dist.destroy_process_group()
        print("ARD_SINGLE_RANK_OK")
        ''' % (ROOT, ROOT, form)))
    env = dict(os.environ)
    env.pop("CUGP_BCM_EXCHANGE", None)
    if form != "library":
        env["CUGP_BCM_EXCHANGE"] = form
    out = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=300, env=env)
    errs = [ln for ln in out.stderr.splitlines() if "Error" in ln or "assert" in ln or "File " in ln]
    assert out.returncode == 0 and "ARD_SINGLE_RANK_OK" in out.stdout, (out.stdout[-2000:], errs[-20:])


# ------------------------------------------------------------------ 10. refusals and recovery
def test_refusals_leave_the_bcm_usable(gp_mod, comm1):
    """The 3-entry BCM calls on an ARD BCM, the _ard calls on an isotropic BCM and nh != d + 2: CUGP_ERR_INVALID with the
    call to use in cugp_last_error, and the evaluation after every one of them reproduces the bits from before."""
    L = capi.lib()
    d, K = 3, 2
    X, y = synth(K * 150, d=d, seed=8, scale=3.0)
    hp = [0.9, 0.5, 1.2, 0.2, -1.0]
    b = gp_mod.BCM.split(X, y, K, ard=True)
    b.set_BCM_log_hyperparam(hp)
    want = b.loglik_grad_rows()
    h, ch = b._h, comm1._h
    v, ll, ne, nh = np.zeros(64), C.c_double(), C.c_int(), C.c_int()
    slot = np.zeros(K, dtype=np.int32)
    p, sp = capi.ptr(v), slot.ctypes.data_as(capi._ip)

    def usable():
        for k in range(K):
            b.set_expert_data(k, X[150 * k: 150 * (k + 1)], y[150 * k: 150 * (k + 1)])     # a full evaluation
        assert same(b.loglik_grad_rows(), want) and np.array_equal(b.get_loghyperparam(), hp)
    assert L.cugp_bcm_num_hyper(h, C.byref(nh)) == 0 and nh.value == 5
    for name, call, use in [
            ("cugp_bcm_set_loghyper", lambda: L.cugp_bcm_set_loghyper(h, p), b"cugp_bcm_set_loghyper_ard"),
            ("cugp_bcm_get_loghyper", lambda: L.cugp_bcm_get_loghyper(h, p), b"cugp_bcm_get_loghyper_ard"),
            ("cugp_bcm_loglik_grad", lambda: L.cugp_bcm_loglik_grad(h, C.byref(ll), p, None), b"cugp_bcm_loglik_grad_ard"),
            ("cugp_bcm_loglik_grad_rows", lambda: L.cugp_bcm_loglik_grad_rows(h, p), b"cugp_bcm_loglik_grad_rows_ard"),
            ("cugp_bcm_loglik_grad_rows_device", lambda: L.cugp_bcm_loglik_grad_rows_device(h, C.c_void_p(v.ctypes.data), sp),
             b"cugp_bcm_loglik_grad_rows_device_ard"),
            ("cugp_bcm_loglik_grad_allgather", lambda: L.cugp_bcm_loglik_grad_allgather(h, ch, K, p),
             b"cugp_bcm_loglik_grad_allgather_ard"),
            ("cugp_bcm_cg_solve", lambda: L.cugp_bcm_cg_solve(h, 5, None, 0, C.byref(ne)), b"cugp_bcm_cg_solve_ard")]:
        assert call() == INV, name
        msg = L.cugp_last_error()
        assert name.encode() in msg and use in msg, (name, msg)
        usable()
    for bad in (3, 4, 6):
        for name, call in [
                ("set", lambda: L.cugp_bcm_set_loghyper_ard(h, p, bad)), ("get", lambda: L.cugp_bcm_get_loghyper_ard(h, p, bad)),
                ("grad", lambda: L.cugp_bcm_loglik_grad_ard(h, C.byref(ll), p, bad, None)),
                ("rows", lambda: L.cugp_bcm_loglik_grad_rows_ard(h, p, bad)),
                ("rows_device", lambda: L.cugp_bcm_loglik_grad_rows_device_ard(h, C.c_void_p(v.ctypes.data), sp, bad)),
                ("allgather", lambda: L.cugp_bcm_loglik_grad_allgather_ard(h, ch, K, bad, p))]:
            assert call() == INV, (name, bad)
            assert b"d + 2 = 5" in L.cugp_last_error(), (name, bad, L.cugp_last_error())
        usable()
    b.close()

    bi = gp_mod.BCM.split(X, y, K)
    bi.set_BCM_log_hyperparam([0.9, 0.2, -1.0])
    wi = bi.loglik_grad_rows()
    hi = bi._h
    assert L.cugp_bcm_num_hyper(hi, C.byref(nh)) == 0 and nh.value == 3
    for name, call, use in [
            ("cugp_bcm_set_loghyper_ard", lambda n: L.cugp_bcm_set_loghyper_ard(hi, p, n), b"cugp_bcm_set_loghyper"),
            ("cugp_bcm_get_loghyper_ard", lambda n: L.cugp_bcm_get_loghyper_ard(hi, p, n), b"cugp_bcm_get_loghyper"),
            ("cugp_bcm_loglik_grad_ard", lambda n: L.cugp_bcm_loglik_grad_ard(hi, C.byref(ll), p, n, None), b"cugp_bcm_loglik_grad"),
            ("cugp_bcm_loglik_grad_rows_ard", lambda n: L.cugp_bcm_loglik_grad_rows_ard(hi, p, n), b"cugp_bcm_loglik_grad_rows"),
            ("cugp_bcm_loglik_grad_rows_device_ard",
             lambda n: L.cugp_bcm_loglik_grad_rows_device_ard(hi, C.c_void_p(v.ctypes.data), sp, n), b"cugp_bcm_loglik_grad_rows_device"),
            ("cugp_bcm_loglik_grad_allgather_ard", lambda n: L.cugp_bcm_loglik_grad_allgather_ard(hi, ch, K, n, p),
             b"cugp_bcm_loglik_grad_allgather"),
            ("cugp_bcm_cg_solve_ard", lambda n: L.cugp_bcm_cg_solve_ard(hi, 5, None, 0, C.byref(ne)), b"cugp_bcm_cg_solve")]:
        for n in (5, 3):
            assert call(n) == INV, (name, n)
            msg = L.cugp_last_error()
            assert name.encode() in msg and b"isotropic" in msg and use in msg, (name, msg)
        for k in range(K):
            bi.set_expert_data(k, X[150 * k: 150 * (k + 1)], y[150 * k: 150 * (k + 1)])
        assert same(bi.loglik_grad_rows(), wi)
    bi.close()


_ISOLATION = r"""
import json, sys
import numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import cugp_amd.gp as gp
from conftest import synth

def iso(K, n):
    X, y = synth(K * n, d=5, seed=n + K, scale=3.0)
    b = gp.BCM.split(X, y, K)
    b.set_BCM_log_hyperparam([0.9, 0.2, -1.0])
    ll, gr, per = b.loglik_grad()
    rows = b.loglik_grad_rows()
    m, v = b.compute_BCM_test_means_and_var(X[:7] * 0.5)
    tr = b.cg_solve(budget=4)
    b.close()
    return [float(x).hex() for x in np.concatenate([[ll], gr, per, rows.ravel(), m, v, tr.ravel()])]

def run_ard(K, n, d):
    X, y = synth(K * n, d=d, seed=n + d, scale=3.0)
    b = gp.BCM.split(X, y, K, ard=True)
    b.set_BCM_log_hyperparam(np.linspace(0.6, 1.2, d).tolist() + [0.2, -1.0])
    b.loglik_grad()
    b.compute_BCM_test_means_and_var(X[:7] * 0.5)
    b.cg_solve(budget=3)
    b.close()

shapes = ((3, 300), (2, 700))
before = {"%%dx%%d" %% s: iso(*s) for s in shapes}          # no ARD BCM has existed in this process yet
for K, n, d in ((3, 300, 5), (2, 700, 5), (4, 200, 17), (1, 300, 3)):
    run_ard(K, n, d)
after = {"%%dx%%d" %% s: iso(*s) for s in shapes}
print("ISOLATION " + json.dumps(dict(before=before, after=after)))
"""


def test_isotropic_bcm_bits_do_not_depend_on_ard_bcms():
    """An isotropic BCM evaluated before any ARD BCM exists in the process (a fresh child process) and a new one on the
    same data after ARD BCMs of the same and of other shapes have lived and gone: identical bits (LL, gradient, rows,
    prediction, a 4-probe cg_solve) at 3 x 300 and 2 x 700 rows."""
    script = _ISOLATION % dict(root=ROOT, tests=os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [s for s in r.stdout.splitlines() if s.startswith("ISOLATION ")][-1]
    out = json.loads(line[len("ISOLATION "):])
    assert out["before"] == out["after"]
    assert all(len(v) > 40 for v in out["before"].values())
