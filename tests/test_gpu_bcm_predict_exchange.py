"""Product-of-experts prediction across ranks inside the library (cugp_bcm_predict_allgather, csrc/comm.cpp): batched
prediction kernels per group of experts, one all-gather of every rank's rows, the product of experts on the device.
On one GPU: a world of one without a communicator, and a one-rank RCCL communicator in a child process.  Every result
must be bit-identical to cugp_bcm_predict over the same experts in one process (BCM.cpp:45-83)."""
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from conftest import GOLDEN, HP_BCM, HP_DENSE, ROOT, synth

pytestmark = pytest.mark.gpu

TUNE_PRED_CHUNK = 19


@pytest.fixture(scope="module")
def gp():
    import cugp_amd.gp as gp
    return gp


@pytest.fixture(scope="module")
def comm1(gp):
    c = gp.Comm(None, 0, 1, 0)            # a world of one without an id: no RCCL
    yield c
    c.close()


def _bcm(gp, rows, d=5, seed=11):
    X, y = synth(sum(rows), d, seed=seed)
    b = gp.BCM(rows, d, 0)
    off = 0
    for k, n in enumerate(rows):
        b.set_expert_data(k, X[off:off + n], y[off:off + n])
        off += n
    return b


def _same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


@pytest.mark.parametrize("rows", [[300], [300] * 3, [300] * 16, [300, 700, 1500]],
                         ids=["K1", "K3", "K16", "ungrouped"])
def test_world_of_one_bits(gp, comm1, rows):
    """K in {1, 3, 16} equal experts (batched launches for K > 1) and 300/700/1500 rows (no group: each expert on its
    own stream): mean and variance bit-equal to cugp_bcm_predict, right after set_BCM_log_hyperparam (stale experts)
    and with the experts valid; a second call gives the same bits."""
    K = len(rows)
    b = _bcm(gp, rows)
    rng = np.random.default_rng(3)
    for i, nt in enumerate([1, 63, 64, 65, 1000]):
        Xt = rng.uniform(-10, 10, (nt, 5))
        b.set_BCM_log_hyperparam(np.array(HP_BCM) + 0.05 * i)
        m1, v1 = comm1.predict_allgather(b, K, K, Xt)              # stale: one evaluation first
        m0, v0 = b.compute_BCM_test_means_and_var(Xt)
        assert np.all(np.isfinite(m0)) and np.all(v0 > 0)
        assert _same(m1, m0) and _same(v1, v0), (nt, np.max(np.abs(m1 - m0)), np.max(np.abs(v1 - v0)))
        m2, v2 = comm1.predict_allgather(b, K, K, Xt)              # valid
        m3, v3 = comm1.predict_allgather(b, K, K, Xt)
        assert _same(m2, m0) and _same(v2, v0) and _same(m3, m0) and _same(v3, v0), nt
    b.close()


@pytest.mark.parametrize("rows", [[300] * 3, [300, 700, 1500]], ids=["grouped", "ungrouped"])
def test_chunked_passes_same_bits(gp, comm1, rows):
    """Tuning key 19 = 1 (64 test points per pass) forces 4 passes for 200 test points: the same bits as one pass."""
    from cugp_amd import capi
    K = len(rows)
    b = _bcm(gp, rows, seed=5)
    b.set_BCM_log_hyperparam(HP_DENSE)
    Xt = np.random.default_rng(8).uniform(-10, 10, (200, 5))
    m0, v0 = comm1.predict_allgather(b, K, K, Xt)
    try:
        capi.check(capi.lib().cugp_set_tuning(TUNE_PRED_CHUNK, 1))
        m1, v1 = comm1.predict_allgather(b, K, K, Xt)
        capi.check(capi.lib().cugp_set_tuning(TUNE_PRED_CHUNK, 3))     # 192 + 8 rows
        m2, v2 = comm1.predict_allgather(b, K, K, Xt)
    finally:
        capi.check(capi.lib().cugp_set_tuning(TUNE_PRED_CHUNK, 0))
    assert _same(m1, m0) and _same(v1, v0) and _same(m2, m0) and _same(v2, v0)
    mr, vr = b.compute_BCM_test_means_and_var(Xt)
    assert _same(m0, mr) and _same(v0, vr)
    b.close()


def _job(name):
    with open(os.path.join(GOLDEN, "golden_r2", name + ".json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def si24000():
    d = np.load(os.path.join(GOLDEN, "data_si24000.npz"))
    return np.ascontiguousarray(d["X"]), np.ascontiguousarray(d["y"])


def _pred_close(a, b):
    b = np.asarray(b)
    return np.all(np.abs(np.asarray(a) - b) <= 1e-8 + 1e-8 * np.abs(b))


@pytest.mark.parametrize("name,K,case", [("si24000_bcm16", 16, 0), ("si24000_bcm16", 16, 1), ("si6000_poe", 4, None)])
def test_goldens_through_the_exchange(gp, comm1, si24000, name, K, case):
    """Configs 5 (16 x 1500 rows, both cases) and 4 (4 x 6000 rows) predicted through the new path: the reference's
    numbers to the suite's tolerances, and the bits of cugp_bcm_predict."""
    X, y = si24000
    c = _job(name)
    if case is not None:
        c = c["cases"][case]
    b = gp.BCM.split(X, y, K)
    b.set_BCM_log_hyperparam(c["hp"])
    Xt = np.array(c["Xt"])
    m, v = comm1.predict_allgather(b, K, K, Xt)
    assert _pred_close(m, c["pred_mean"]), np.max(np.abs(m - np.array(c["pred_mean"])))
    assert _pred_close(v, c["pred_var"]), np.max(np.abs(v - np.array(c["pred_var"])))
    nlpp = b.get_BCM_negative_log_predprob(np.array(c["yt"]), m, v)
    assert abs(nlpp - c["nlpp"]) <= 1e-8 * max(1.0, abs(c["nlpp"]))
    m0, v0 = b.compute_BCM_test_means_and_var(Xt)
    assert _same(m, m0) and _same(v, v0)
    b.close()


def test_errors_then_recovery(gp, comm1):
    """Argument errors return CUGP_ERR_INVALID; a local failure (an expert whose data was never set) returns an error
    with NaN outputs, no hang; the same communicator then serves a correct call."""
    from cugp_amd import capi
    L = capi.lib()
    Xt = np.random.default_rng(2).uniform(-10, 10, (70, 5))
    m, v = np.empty(70), np.empty(70)
    b = _bcm(gp, [300] * 3)
    b.set_BCM_log_hyperparam(HP_BCM)

    def call(bcm, per, nexp, nt=70, mp=m, vp=v):
        m[:] = 0.0
        v[:] = 0.0
        return L.cugp_bcm_predict_allgather(bcm._h if bcm is not None else None, comm1._h, per, nexp, capi.ptr(Xt), nt,
                                            capi.ptr(mp) if mp is not None else None,
                                            capi.ptr(vp) if vp is not None else None)

    assert call(b, 3, 3, nt=0) == capi.CUGP_ERR_INVALID
    assert call(b, 3, 3, mp=None) == capi.CUGP_ERR_INVALID
    assert call(b, 3, 3, vp=None) == capi.CUGP_ERR_INVALID
    assert call(b, 2, 2) == capi.CUGP_ERR_INVALID                  # per smaller than the local expert count
    assert np.all(np.isnan(m)) and np.all(np.isnan(v))
    assert call(b, 4, 4) == capi.CUGP_ERR_INVALID                  # nexperts does not match the BCM
    assert np.all(np.isnan(m)) and np.all(np.isnan(v))
    assert b"rank 0" in L.cugp_last_error()
    bad = gp.BCM([300], 5, 0)                                      # data never set
    bad.set_BCM_log_hyperparam(HP_BCM)
    rc = call(bad, 1, 1)
    assert rc != capi.CUGP_OK
    assert np.all(np.isnan(m)) and np.all(np.isnan(v))
    assert b"rank 0" in L.cugp_last_error()
    bad.close()
    mg, vg = comm1.predict_allgather(b, 3, 3, Xt)
    m0, v0 = b.compute_BCM_test_means_and_var(Xt)
    assert _same(mg, m0) and _same(vg, v0)
    b.close()


@pytest.mark.parametrize("form", ["library", "allreduce"])
def test_sharded_bcm_predict_rccl_single_rank(tmp_path, form):
    """ShardedBCM under a one-rank NCCL (= RCCL) process group: the library form predicts through
    cugp_bcm_predict_allgather (predict_form == "library"), the allreduce form through torch (predict_form == "torch");
    both give the bits of the single-process gp.BCM, before and after a short cg_solve.  Child process: a process group
    is process-global state."""
    script = tmp_path / "rank0.py"
    script.write_text(textwrap.dedent('''
        import os, sys
        import numpy as np, torch, torch.distributed as dist
        sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tests"))
        from conftest import synth, HP_DENSE
        from cugp_amd.bcm import ShardedBCM
        import cugp_amd.gp as gp
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29541")
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
        X, y = synth(3 * 300, 5, seed=4)
        experts = [(X[300 * k:300 * (k + 1)], y[300 * k:300 * (k + 1)]) for k in range(3)]
        b = ShardedBCM(experts, rank=0, world=1, device=0, comm_device=torch.device("cuda", 0))
        assert b.exchange_form == %r, b.exchange_form
        b._allreduce = lambda t: (dist.all_reduce(t, op=dist.ReduceOp.SUM), t)[1]     # force the collective at 1 rank
        want = "library" if b.exchange_form == "library" else "torch"
        ref = gp.BCM([300, 300, 300], 5, 0)
        for k, (Xk, yk) in enumerate(experts):
            ref.set_expert_data(k, Xk, yk)
        Xt = np.random.default_rng(1).uniform(-10, 10, (130, 5))
        b.set_loghyper(HP_DENSE)
        for step in range(2):
            if want == "torch":
                # (the torch path predicts expert by expert: stale experts would each be evaluated alone, and a lone
                #  evaluation's K^-1 is not bit-identical to a group's -- today's behaviour of that path)
                b.loglik_grad()
            m, v = b.predict(Xt)
            assert b.predict_form == want, (b.predict_form, want)
            ref.set_BCM_log_hyperparam(b.hp)
            m0, v0 = ref.compute_BCM_test_means_and_var(Xt)
            assert np.array_equal(m.view(np.uint64), m0.view(np.uint64)), (step, np.max(np.abs(m - m0)))
            assert np.array_equal(v.view(np.uint64), v0.view(np.uint64)), (step, np.max(np.abs(v - v0)))
            if step == 0:
                b.cg_solve(budget=6)
        b.close(); ref.close()
        dist.destroy_process_group()
        print("PREDICT_SINGLE_RANK_OK")
        ''' % (ROOT, ROOT, form)))
    env = dict(os.environ)
    env.pop("CUGP_BCM_EXCHANGE", None)
    if form != "library":
        env["CUGP_BCM_EXCHANGE"] = form
    out = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=300, env=env)
    errs = [ln for ln in out.stderr.splitlines() if "Error" in ln or "assert" in ln or "File " in ln]
    assert out.returncode == 0 and "PREDICT_SINGLE_RANK_OK" in out.stdout, (out.stdout[-2000:], errs[-20:])


def test_train_test_rows_nlpp(tmp_path, oracle):
    """`python -m cugp_amd.train --test-rows` on one rank (the torch path of ShardedBCM.predict): the printed NLPP is the
    oracle BCM's prediction NLPP at the final hyper-parameters, to 1e-8."""
    from cugp_amd import dataset
    from cugp_amd.bcm import ShardedBCM
    K, rows, nt, budget = 3, 200, 40, 5
    X, y = synth(K * rows + nt, 4, seed=21)
    pre_x, pre_y = str(tmp_path / "in_"), str(tmp_path / "lab_")
    dataset.write_chunk(pre_x + "0.txt", pre_y + "0.txt", np.vstack([X[:rows], X[K * rows:]]),
                        np.concatenate([y[:rows], y[K * rows:]]))
    for k in range(1, K):
        dataset.write_chunk("%s%d.txt" % (pre_x, k), "%s%d.txt" % (pre_y, k), X[k * rows:(k + 1) * rows],
                            y[k * rows:(k + 1) * rows])
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "CUGP_BCM_EXCHANGE"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, "-m", "cugp_amd.train", "--numchunks", str(K), "--rows", str(rows),
                          "--inputs", pre_x, "--labels", pre_y, "--test-rows", str(nt), "--budget", str(budget),
                          "--hp", "1.5", "1.5", "1.5"],
                         capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-3000:])
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("NLPP = ")]
    assert len(line) == 1, out.stdout[-2000:]
    nlpp = float(line[0].split("=")[1])
    # the same data as the run read it (5 significant digits), the same deterministic optimisation -> its end point
    shards = dataset.load_shards(pre_x, pre_y, K)
    experts = [(s[0][:rows], s[1][:rows]) for s in shards]
    sb = ShardedBCM(experts)
    sb.set_loghyper([1.5, 1.5, 1.5])
    sb.cg_solve(budget)
    hp = sb.hp.copy()
    sb.close()
    Xt, yt = shards[0][0][rows:rows + nt], shards[0][1][rows:rows + nt]
    ob = oracle.bcm(np.vstack([e[0] for e in experts]), np.concatenate([e[1] for e in experts]), K, hp)
    mo, vo = ob.predict(Xt)
    ob.close()
    nlpp_o = oracle.nlpp(yt, mo, vo)
    assert abs(nlpp - nlpp_o) <= 1e-8 * max(1.0, abs(nlpp_o)), (nlpp, nlpp_o)
