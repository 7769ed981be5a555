"""GPU tests of the sparse variational model with its rows sharded over ranks (cugp_sparse_create_shard,
cugp_sparse_sharded_bound_grad, cugp_sparse_sharded_cg_solve; cugp_amd.sparse_sharded.ShardedSparseGP).

  K = 1      F, g, gZ and the predictions are SparseGP's on the same data bit for bit -- in a world of one without an id and
             through a one-rank RCCL communicator (child process: a process group is process-global state)
  accuracy   every case of truth_sparse_shard.SHARD_CASES, in a world of one that owns all K shards, against the
             extended-precision truth of the truth_sparse case it is built over:
                 err_gpu(q) <= F_SPARSE_SHARD[family] * max(yardstick, 4 ulp)      (gZ: F_SPARSE_SHARD_Z)
             the factors fixed on the CPU (tests/test_truth_sparse_shard_cpu.py), never from the GPU; every figure is
             printed before it is asserted ("ACC ..."; run with -s)
  bits       depend on (data, K) only: per = K against per = K + 2, repeated calls, what = 0 / 1 / 2
  state      staleness and refusals, not positive definite, the optimiser, other handles untouched
  two ranks  K = 3 over W = 2 and K = 2 over W = 2 in two child processes on two devices against the world of one's bits;
             skips on a machine with one device.  The children run under tests/rank_children.py: each under its own
             timeout in a session of its own, all ended by process group on the first failure
"""
import ctypes as C
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import rank_children
import truth
import truth_sparse as ts
import truth_sparse_shard as tsh
from accuracy import Report
from cugp_amd import capi

pytestmark = pytest.mark.gpu
extended = pytest.mark.skipif(not truth.EXTENDED, reason="numpy.longdouble is not an extended-precision type here")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def mods():
    import cugp_amd.gp as gp
    import cugp_amd.sparse_sharded as ss
    return gp, ss


def kernel_args(name):
    family = ts.CASES[name][0]
    if family.endswith("_ard"):
        return dict(kernel=family)
    return dict(kernel=family if family.startswith("matern") else "se", ard=family == "ard")


def sharded(ss, name, counts, hp=None, **kw):
    """A ShardedSparseGP of the case in a world of one that owns every shard -> (model, shards, Z, Xt, cov)."""
    shards, Z, Xt, cov, chunk = tsh.shards_of(name, counts)
    m = ss.ShardedSparseGP(shards, Z, jitter=ts.JITTER, chunk_rows=chunk, **dict(kernel_args(name), **kw))
    m.set_loghyper(cov.hp if hp is None else hp)
    return m, shards, Z, Xt, cov


def plain(gp, name, hp=None):
    X, y, Z, Xt, cov, chunk = ts.inputs(name)
    s = gp.SparseGP(len(y), Z.shape[0], Z.shape[1], jitter=ts.JITTER, chunk_rows=chunk, **kernel_args(name))
    s.set_data(X, y)
    s.set_inducing(Z)
    s.set_loghyperparam(cov.hp if hp is None else hp)
    return s


def bits(*arrays):
    return [np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).copy() for a in arrays]


def same_bits(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(bits(*a), bits(*b)))


def everything(m, Xt):
    """F, g, gZ and the predictions the lead answers, as one list of arrays."""
    F, g, gZ = m.bound_grad_z()
    mean, var = m.predict(Xt)
    jm, jc = m.predict_joint(Xt)
    gm, gv, dm, dv = m.predict_grad(Xt)
    return [np.float64(F), g, gZ, mean, var, jm, jc, gm, gv, dm, dv]


# ------------------------------------------------------------------ 1. K = 1 is SparseGP
K1_NAMES = ["se_n300_m65", "se_n1300_m200", "ard_n300_m130_d17", "matern32_ard_n1000_m130"]


@pytest.mark.parametrize("name", K1_NAMES)
def test_one_shard_is_sparsegp_bit_for_bit(mods, name):
    gp, ss = mods
    N = ts.CASES[name][1]
    m, _, Z, Xt, cov = sharded(ss, name, (N,))
    ref = plain(gp, name)
    got, want = everything(m, Xt), everything(ref, Xt)
    assert np.all(np.isfinite(got[0])) and np.all(np.isfinite(got[2]))
    assert same_bits(got, want), [np.max(np.abs(a - b)) for a, b in zip(got, want)]
    assert same_bits([m.bound()], [ref.bound()]) and same_bits(m.bound_grad(), ref.bound_grad())
    assert m.lead.info() == (0, 1, N)
    k, K, rows = C.c_int(7), C.c_int(7), C.c_longlong(7)              # an ordinary handle is no member of anything
    capi.check(capi.lib().cugp_sparse_shard_info(ref.handle, C.byref(k), C.byref(K), C.byref(rows)))
    assert (k.value, K.value, rows.value) == (-1, 0, 0)
    m.close()
    ref.close()


def test_one_shard_through_a_one_rank_rccl_communicator(tmp_path):
    script = tmp_path / "rank0.py"
    script.write_text(textwrap.dedent('''
        import os, sys
        import numpy as np, torch, torch.distributed as dist
        sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tests"))
        import test_gpu_sparse_shard as T
        import truth_sparse as ts
        import cugp_amd.gp as gp, cugp_amd.sparse_sharded as ss
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29547")
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
        for name in ("se_n300_m65", "se_n1300_m200"):
            m, _, Z, Xt, cov = T.sharded(ss, name, (ts.CASES[name][1],))
            assert m._comm is not None and m.world == 1
            ref = T.plain(gp, name)
            got, want = T.everything(m, Xt), T.everything(ref, Xt)
            assert T.same_bits(got, want), name
            m.close(); ref.close()
        # three shards through the communicator: the bits of the world of one without an id
        m, _, Z, Xt, cov = T.sharded(ss, "se_n300_m65", (171, 128, 1))
        got = T.everything(m, Xt)
        m.close()
        dist.destroy_process_group()
        np.savez(sys.argv[1], *got)
        print("SHARD_SINGLE_RANK_OK")
        ''' % (ROOT, ROOT)))
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, str(script), str(tmp_path / "got.npz")], capture_output=True, text=True, timeout=300,
                         env=env)
    errs = [ln for ln in out.stderr.splitlines() if "Error" in ln or "assert" in ln or "File " in ln]
    assert out.returncode == 0 and "SHARD_SINGLE_RANK_OK" in out.stdout, (out.stdout[-2000:], errs[-20:])
    import cugp_amd.sparse_sharded as ss
    m, _, Z, Xt, cov = sharded(ss, "se_n300_m65", (171, 128, 1))
    want = everything(m, Xt)
    m.close()
    with np.load(tmp_path / "got.npz") as f:
        got = [f["arr_%d" % i] for i in range(len(want))]
    assert same_bits(got, want)


# ------------------------------------------------------------------ 2. accuracy
@extended
@pytest.mark.parametrize("sc", tsh.SHARD_CASES, ids=tsh.case_id)
def test_accuracy(mods, sc):
    gp, ss = mods
    name, counts = sc
    c, cz = ts.case(name), tsh.gz_case(name)
    m, shards, Z, Xt, cov = sharded(ss, name, counts)
    assert m.K == len(counts) and [s.n for s in m.local_shards] == list(counts)
    F, g, gZ = m.bound_grad_z()
    mean, var = m.predict(Xt)
    assert np.isfinite(F) and np.all(np.isfinite(g)) and np.all(np.isfinite(gZ)) and gZ.shape == Z.shape
    rep = Report("sparse-shard/" + tsh.case_id(sc), cov)
    tsh.hold(rep, c, F, g, mean, var)
    tsh.hold_gz(rep, cz, gZ)
    assert m.lead.info() == (0, len(counts), sum(counts))
    m.close()
    rep.check()


# ------------------------------------------------------------------ 3. the bits depend on (data, K) only
@pytest.mark.parametrize("sc", [("se_n300_m65", (171, 128, 1)), ("se_n1300_m200", (700, 600)),
                                ("se_n128_m128", (26, 26, 26, 26, 24))], ids=tsh.case_id)
def test_bits_depend_on_data_and_shard_count_only(mods, sc):
    gp, ss = mods
    name, counts = sc
    m, _, Z, Xt, cov = sharded(ss, name, counts)
    first = everything(m, Xt)
    for s in m.local_shards:                                          # launched again: the same bits
        s.set_loghyperparam(np.asarray(cov.hp) + 0.125)
    m.bound_grad_z()
    m.set_loghyper(cov.hp)
    assert same_bits(everything(m, Xt), first)
    F0 = m.bound()                                                    # what = 0, 1, 2 on fresh state each
    m.set_inducing(Z)
    F1, g1 = m.bound_grad()
    m.set_inducing(Z)
    assert same_bits([F0, F1, g1], [first[0], first[0], first[1]])
    wide, _, _, _, _ = sharded(ss, name, counts)
    wide.per = len(counts) + 2                                        # two empty slots behind the shards
    assert same_bits(everything(wide, Xt), first)
    wide.close()
    m.close()


# ------------------------------------------------------------------ 4. staleness and refusals
def raises_invalid(fn, *words):
    with pytest.raises(capi.CugpError) as ei:
        fn()
    assert ei.value.code == capi.CUGP_ERR_INVALID, ei.value
    for w in words:
        assert w in str(ei.value), (w, str(ei.value))


def test_staleness_and_refusals(mods):
    gp, ss = mods
    name, counts = "se_n300_m65", (171, 128, 1)
    m, shards, Z, Xt, cov = sharded(ss, name, counts)
    first = everything(m, Xt)
    lead, mid, last = m.local_shards

    def fresh_again():
        assert same_bits(everything(m, Xt), first)

    hp2 = np.asarray(cov.hp) + 0.25
    for change, undo in ((lambda: last.set_loghyperparam(hp2), lambda: m.set_loghyper(cov.hp)),
                         (lambda: mid.set_inducing(Z + 0.5), lambda: m.set_inducing(Z)),
                         (lambda: last.set_data(*shards[2]), lambda: None),
                         (lambda: lead.set_loghyperparam(hp2), lambda: m.set_loghyper(cov.hp))):
        change()
        for call in (lambda: m.predict(Xt), lambda: m.predict_joint(Xt), lambda: m.predict_grad(Xt),
                     lambda: m.sample_posterior(Xt, 2, rng=0)):
            raises_invalid(call, "cugp_sparse_sharded_bound_grad")
        undo()
        fresh_again()
    # the plain evaluating calls on a shard handle, a prediction from a shard that is not the lead
    for call in (lead.bound, lead.bound_grad, lead.bound_grad_z, lambda: lead.cg_solve(3), lambda: lead.cg_solve(3, inducing=True),
                 lambda: lead.set_targets(np.zeros((lead.n, 2))), lead.bound_targets, lambda: mid.predict(Xt)):
        raises_invalid(call, "cugp_sparse_sharded_bound_grad")
    fresh_again()
    # an ordinary handle in the list
    odd = gp.SparseGP(128, Z.shape[0], Z.shape[1], jitter=ts.JITTER, chunk_rows=128)
    odd.set_data(*shards[1])
    odd.set_inducing(Z)
    odd.set_loghyperparam(cov.hp)
    raises_invalid(lambda: m._comm.sparse_sharded_bound_grad([lead._h, odd._h, last._h], m.per, m.K, 2, m.nh, m.m, m.d),
                   "ordinary handle", "rank 0")
    raises_invalid(lambda: m._comm.sparse_sharded_bound_grad([odd._h], 1, 1, 0, m.nh, m.m, m.d), "ordinary")
    odd.close()
    fresh_again()
    # Z differing in one bit between local shards
    Z1 = Z.copy()
    Z1.view(np.uint64)[3, 1] ^= np.uint64(1)
    mid.set_inducing(Z1)
    raises_invalid(m.bound_grad_z, "bits of Z", "rank 0")
    raises_invalid(lambda: m.predict(Xt))
    mid.set_inducing(Z)
    fresh_again()
    # hyper-parameters differing between local shards; a wrong count
    last.set_loghyperparam(hp2)
    raises_invalid(m.bound, "hyper-parameters")
    # the optimiser refuses them too, and brings nothing into line in passing
    raises_invalid(lambda: m.cg_solve(3), "cugp_sparse_sharded_cg_solve", "hyper-parameters", "rank 0")
    raises_invalid(lambda: m.cg_solve(3, inducing=True), "hyper-parameters")
    assert np.array_equal(last.get_loghyperparam(), hp2) and np.array_equal(lead.get_loghyperparam(), np.asarray(cov.hp, dtype=np.float64))
    m.set_loghyper(cov.hp)
    raises_invalid(lambda: m._comm.sparse_sharded_bound_grad([lead._h, mid._h], m.per, m.K, 0, m.nh, m.m, m.d), "holds 2 shards")
    fresh_again()
    m.close()


# ------------------------------------------------------------------ 5. not positive definite
def test_not_positive_definite_gives_nan_everywhere(mods):
    gp, ss = mods
    name, counts = "se_n300_m65", (171, 128, 1)
    m, shards, Z, Xt, cov = sharded(ss, name, counts)
    first = everything(m, Xt)
    Xbad = shards[1][0].copy()
    Xbad[40, 0] = np.nan                                              # a NaN row in the middle shard
    m.local_shards[1].set_data(Xbad, shards[1][1])
    got = everything(m, Xt)                                           # CUGP_OK throughout: no raise
    assert all(np.all(np.isnan(a)) for a in got)
    m.local_shards[1].set_data(*shards[1])
    fresh, _, _, _, _ = sharded(ss, name, counts)                     # a model that never failed
    want = everything(fresh, Xt)
    fresh.close()
    assert same_bits(everything(m, Xt), want) and same_bits(first, want)
    hp = np.asarray(cov.hp, dtype=np.float64).copy()
    hp[0] = -800.0                                                    # a length scale of exp(-800)
    m.set_loghyper(hp)
    got = everything(m, Xt)
    assert all(np.all(np.isnan(a)) for a in got)
    m.set_loghyper(cov.hp)
    assert same_bits(everything(m, Xt), want)
    m.close()


# ------------------------------------------------------------------ 6. the optimiser
def test_optimiser(mods):
    gp, ss = mods
    name = "se_n300_m65"
    m, shards, Z, Xt, cov = sharded(ss, name, (171, 128, 1))
    for budget, inducing in ((10, False), (6, True)):
        m.set_loghyper(cov.hp)
        m.set_inducing(Z)
        tr = m.cg_solve(budget, inducing=inducing)
        assert tr.shape[1] == m.nh + 1 and tr.shape[0] >= 2 and np.all(np.isfinite(tr))
        assert tr[-1, -1] < tr[0, -1], tr[:, -1]
        assert all(np.array_equal(s.get_loghyperparam(), m.get_loghyper()) for s in m.local_shards)
        assert all(np.array_equal(s.get_inducing(), m.get_inducing()) for s in m.local_shards)
        assert np.array_equal(m.get_inducing(), Z) != inducing
        assert -m.bound() < tr[0, -1]                                 # the end point that stays set lies below the start
    m.close()
    # one shard: SparseGP.cg_solve's trajectory
    one, _, Z, Xt, cov = sharded(ss, name, (300,))
    ref = plain(gp, name)
    for budget, inducing in ((10, False), (6, True)):
        a, b = one.cg_solve(budget, inducing=inducing), ref.cg_solve(budget, inducing=inducing)
        assert same_bits([a, one.get_loghyper(), one.get_inducing()], [b, ref.get_loghyperparam(), ref.get_inducing()])
    one.close()
    ref.close()


# ------------------------------------------------------------------ 7. other handles untouched
def test_other_handles_keep_their_bits(mods):
    gp, ss = mods
    from conftest import HP_DEFAULT, synth
    ref = plain(gp, "se_n300_m65")
    X, y = synth(200, d=3, seed=5)
    dense = gp.Covsum(200, 3)
    dense.set_loghyperparam(HP_DEFAULT)
    before = [*ref.bound_grad_z(), *ref.predict(ts.inputs("se_n300_m65")[3]), *dense.loglik_grad(X, y)]
    m, _, Z, Xt, cov = sharded(ss, "se_n300_m65", (171, 128, 1))
    everything(m, Xt)
    ref.set_inducing(Z)                                               # launched again beside the live sharded model
    dense.set_data(X, y)
    after = [*ref.bound_grad_z(), *ref.predict(Xt), *dense.loglik_grad(X, y)]
    assert same_bits(before, after)
    m.close()
    after = [*ref.bound_grad_z(), *ref.predict(Xt), *dense.loglik_grad(X, y)]
    assert same_bits(before, after)
    ref.close()
    dense.close()


# ------------------------------------------------------------------ 8. two ranks on two devices
TWO_RANK_CASES = (("se_n300_m65", (171, 128, 1)), ("se_n1300_m200", (700, 600)))


def test_two_ranks_give_the_world_of_ones_bits(mods, tmp_path):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    gp, ss = mods
    script = tmp_path / "rank.py"
    script.write_text(textwrap.dedent('''
        import os, sys
        import numpy as np, torch, torch.distributed as dist
        sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tests"))
        import test_gpu_sparse_shard as T
        import truth_sparse_shard as tsh
        import cugp_amd.sparse_sharded as ss
        rank = int(sys.argv[1])
        torch.cuda.set_device(rank)
        dist.init_process_group("nccl", rank=rank, world_size=2, device_id=torch.device("cuda", rank))
        out = []
        for name, counts in T.TWO_RANK_CASES:
            shards, Z, Xt, cov, chunk = tsh.shards_of(name, counts)
            mine = [s if k %% 2 == rank else None for k, s in enumerate(shards)]
            m = ss.ShardedSparseGP(mine, Z, rank=rank, world=2, device=rank, jitter=T.ts.JITTER, chunk_rows=chunk,
                                   **T.kernel_args(name))
            m.set_loghyper(cov.hp)
            out += T.everything(m, Xt)
            m.close()
        dist.barrier()
        dist.destroy_process_group()
        np.savez(sys.argv[2], *out)
        print("SHARD_RANK_OK")
        ''' % (ROOT, ROOT)))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29548")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    cmds = [[sys.executable, script, r, tmp_path / ("r%d.npz" % r)] for r in range(2)]
    failed, texts = rank_children.run_ranks(cmds, env, tmp_path, 240)  # (ends both on the first failure, by process group)
    assert failed is None, (failed, texts[failed[0]][-3000:])
    assert all("SHARD_RANK_OK" in t for t in texts), [t[-1500:] for t in texts]
    want = []
    for name, counts in TWO_RANK_CASES:
        m, _, Z, Xt, cov = sharded(ss, name, counts)
        want += everything(m, Xt)
        m.close()
    for r in range(2):
        with np.load(tmp_path / ("r%d.npz" % r)) as f:
            got = [f["arr_%d" % i] for i in range(len(want))]
        assert same_bits(got, want), r
