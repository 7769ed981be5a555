"""The sharded sparse model's interface without a GPU: the four entry points are exported and bound with the header's
signatures, the header states the protocol, every refusal that needs no device is CUGP_ERR_INVALID with the call's name and
writes nothing, the plumbing of ShardedSparseGP (handles in slot order, per, K, what, the keywords) and of train.py is in
place, the slot map is bcm.py's, and a world above one without an nccl group raises."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cugp_amd.gp as gp
import cugp_amd.sparse_sharded as ss
from conftest import ROOT
from cugp_amd import capi, train
from cugp_amd.bcm import gather_row_index, gather_rows_per_rank
from cugp_amd.bcm import split_rows as bcm_split_rows

_dp, _ip, _vp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_void_p
_vpp = C.POINTER(C.c_void_p)
NEW = {
    "cugp_sparse_create_shard": [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, _vpp],
    "cugp_sparse_shard_info": [_vp, _ip, _ip, C.POINTER(C.c_longlong)],
    "cugp_sparse_sharded_bound_grad": [_vpp, C.c_int, _vp, C.c_int, C.c_int, C.c_int, _dp, _dp, C.c_int, _dp],
    "cugp_sparse_sharded_cg_solve": [_vpp, C.c_int, _vp, C.c_int, C.c_int, C.c_int, C.c_int, _dp, C.c_int, _ip],
}
DECLS = {
    "cugp_sparse_create_shard": "int n_local, int m, int d, int device, int kernel, int ard, double jitter, int chunk_rows, "
                                "int shard, int nshards, cugp_sparse **out",
    "cugp_sparse_shard_info": "const cugp_sparse *sp, int *shard, int *nshards, long long *rows_total",
    "cugp_sparse_sharded_bound_grad": "cugp_sparse *const *shards, int nlocal, cugp_comm *comm, int per, int nshards, int what, "
                                      "double *F, double *g, int nh, double *gZ",
    "cugp_sparse_sharded_cg_solve": "cugp_sparse *const *shards, int nlocal, cugp_comm *comm, int per, int nshards, int budget, "
                                    "int inducing, double *trace, int trace_cap, int *nevals",
}
INV = capi.CUGP_ERR_INVALID


def header():
    with open(os.path.join(ROOT, "include", "cugp.h")) as f:
        return f.read()


@pytest.mark.parametrize("name", sorted(NEW))
def test_exported_and_bound(name):
    res, args = capi.SIGNATURES[name]
    assert res is C.c_int and args == NEW[name] and len(args) == len(DECLS[name].split(","))
    fn = getattr(capi.lib(), name)
    assert fn.restype is C.c_int and list(fn.argtypes) == NEW[name]


@pytest.mark.parametrize("name", sorted(NEW))
def test_header_declares_the_signature(name):
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, text)
    assert decl, name
    assert " ".join(decl.group(1).split()).replace(" ,", ",") == DECLS[name]


def test_header_states_the_protocol():
    text = " ".join(re.sub(r"\n\s*\*(?!/)", " ", header()).split())
    for words in ("Shard k lives on rank k mod W in slot k / W", "K >= W: every rank owns a shard",
                  "ONE ncclAllGather of [header | per slots] on the evaluation's stream", "GLOBAL SHARD ORDER",
                  "first term copied, then a = a + b; no atomics, never ncclAllReduce", "depend on (data, K), not on W or per",
                  "With K = 1 every sum hands the one shard's numbers on", "No host wait beyond those two",
                  "a fingerprint of the bits of the hyper-parameters and of Z",
                  "still joins exchange 1 (nonzero status, all-ones slots)", "none enters exchange 2",
                  "they never evaluate", "nshards = 0 (shard = -1, rows_total = 0) on an ordinary handle",
                  "on every rank alike, before any collective", "identical trajectories by construction", "no targets"):
        assert words in text, words


def refused(rc, call, *words):
    err = capi.lib().cugp_last_error()
    return rc == INV and call.encode() in err and all(w.encode() in err for w in words)


def test_refusals_that_need_no_device():
    L = capi.lib()
    h, F, ne, out = _vp(), C.c_double(7.0), C.c_int(7), np.zeros(8)
    for shard, nshards in ((0, 0), (-1, 2), (2, 2)):
        assert refused(L.cugp_sparse_create_shard(10, 4, 2, 0, 0, 0, 1e-6, 0, shard, nshards, C.byref(h)), "cugp_sparse_create_shard")
    assert refused(L.cugp_sparse_create_shard(10, 4, 2, 0, 0, 0, 1e-6, 0, 0, 1, None), "cugp_sparse_create_shard")
    assert refused(L.cugp_sparse_create_shard(0, 4, 2, 0, 0, 0, 1e-6, 0, 0, 1, C.byref(h)), "cugp_sparse_create")   # n_local >= 1
    assert not h.value
    assert refused(L.cugp_sparse_shard_info(None, None, None, None), "cugp_sparse_shard_info")
    comm = gp.Comm(None, 0, 1, 0)                                    # a world of one without an id: no device is touched
    lst = (C.c_void_p * 2)(None, None)
    call, solve = "cugp_sparse_sharded_bound_grad", "cugp_sparse_sharded_cg_solve"
    g, gZ = capi.ptr(out), capi.ptr(out)
    assert refused(L.cugp_sparse_sharded_bound_grad(lst, 1, None, 1, 1, 0, C.byref(F), g, 3, gZ), call)
    assert refused(L.cugp_sparse_sharded_bound_grad(None, 1, comm._h, 1, 1, 0, C.byref(F), g, 3, gZ), call)
    assert refused(L.cugp_sparse_sharded_bound_grad(lst, 1, comm._h, 1, 1, 0, None, g, 3, gZ), call)
    assert refused(L.cugp_sparse_sharded_bound_grad(lst, 0, comm._h, 1, 1, 0, C.byref(F), g, 3, gZ), call)
    assert refused(L.cugp_sparse_sharded_bound_grad(lst, 1, comm._h, 0, 1, 0, C.byref(F), g, 3, gZ), call)
    assert refused(L.cugp_sparse_sharded_bound_grad(lst, 1, comm._h, 1, 1, 3, C.byref(F), g, 3, gZ), call, "what")
    assert refused(L.cugp_sparse_sharded_bound_grad(lst, 1, comm._h, 1, 1, 1, C.byref(F), None, 3, gZ), call)
    assert refused(L.cugp_sparse_sharded_bound_grad(lst, 1, comm._h, 1, 1, 2, C.byref(F), g, 3, None), call)
    assert refused(L.cugp_sparse_sharded_bound_grad(lst, 1, comm._h, 1, 0, 0, C.byref(F), g, 3, gZ), call, "a rank without a shard")
    assert refused(L.cugp_sparse_sharded_bound_grad(lst, 2, comm._h, 1, 2, 0, C.byref(F), g, 3, gZ), call, "per * world < nshards")
    assert refused(L.cugp_sparse_sharded_bound_grad(lst, 1, comm._h, 1, 1, 2, C.byref(F), g, 3, gZ), call, "first shard handle is NULL")
    assert refused(L.cugp_sparse_sharded_cg_solve(lst, 1, None, 1, 1, 5, 0, None, 0, C.byref(ne)), solve)
    assert refused(L.cugp_sparse_sharded_cg_solve(lst, 1, comm._h, 1, 1, 0, 0, None, 0, C.byref(ne)), solve, "budget")
    assert refused(L.cugp_sparse_sharded_cg_solve(lst, 1, comm._h, 1, 0, 5, 0, None, 0, C.byref(ne)), solve)
    assert refused(L.cugp_sparse_sharded_cg_solve(lst, 1, comm._h, 1, 1, 5, 1, None, 0, C.byref(ne)), solve, "first shard handle is NULL")
    comm.close()
    assert (F.value, ne.value) == (7.0, 7) and not out.any()


@pytest.mark.parametrize("K, W", [(1, 1), (3, 1), (4, 2), (5, 2), (8, 8), (9, 8)])
def test_slot_map_is_bcms(K, W):
    per = ss.slots_per_rank(K, W)
    assert per == gather_rows_per_rank(K, W) == -(-K // W)
    seen = set()
    for k in range(K):
        assert ss.shard_owner(k, W) == k % W
        assert ss.slot_index(k, W, per) == gather_row_index(k, W, per) == (k % W) * per + k // W
        seen.add(ss.slot_index(k, W, per))
    assert len(seen) == K and max(seen) < W * per
    assert ss.split_rows(1003, K) == bcm_split_rows(1003, K)


class _Lib:
    """Records the calls in place of the library (no device): what ShardedSparseGP hands over."""

    def __init__(self):
        self.calls, self.next = [], 0x100

    def cugp_sparse_create_shard(self, n, m, d, device, kind, ard, jitter, chunk, shard, nshards, out):
        self.next += 0x10
        out._obj.value = self.next
        self.calls.append(("create_shard", n, m, d, device, kind, ard, jitter, chunk, shard, nshards))
        return 0

    def cugp_sparse_destroy(self, h):
        self.calls.append(("destroy", h.value))
        return 0

    def cugp_sparse_set_data(self, h, X, y):
        self.calls.append(("set_data", h.value))
        return 0

    def cugp_sparse_set_inducing(self, h, Z):
        self.calls.append(("set_inducing", h.value, Z[0]))
        return 0

    def cugp_sparse_set_loghyper(self, h, hp, nh):
        self.calls.append(("set_loghyper", h.value, nh, hp[0]))
        return 0

    def cugp_comm_create(self, idbuf, nbytes, rank, world, device, out):
        out._obj.value = 0x7
        self.calls.append(("comm_create", idbuf is None, nbytes, rank, world, device))
        return 0

    def cugp_comm_destroy(self, h):
        self.calls.append(("comm_destroy",))
        return 0

    def cugp_sparse_sharded_bound_grad(self, lst, nlocal, comm, per, nshards, what, F, g, nh, gZ):
        self.calls.append(("bound_grad", [lst[i] for i in range(nlocal)], comm.value, per, nshards, what, nh, g is None, gZ is None))
        F._obj.value = -2.5
        return 0

    def cugp_sparse_sharded_cg_solve(self, lst, nlocal, comm, per, nshards, budget, inducing, tr, cap, ne):
        self.calls.append(("cg_solve", [lst[i] for i in range(nlocal)], per, nshards, budget, inducing, cap))
        ne._obj.value = 5
        for k in range(2 * 4):
            tr[k] = float(k)
        return 0

    def cugp_sparse_predict(self, h, Xt, nt, noise, m, v):
        self.calls.append(("predict", h.value, nt, noise))
        return 0


def test_python_plumbing(monkeypatch):
    fake = _Lib()
    monkeypatch.setattr(capi, "lib", lambda: fake)
    rng = np.random.default_rng(0)
    X, y, Z = rng.standard_normal((50, 2)), rng.standard_normal(50), rng.standard_normal((4, 2))
    m = ss.ShardedSparseGP.split(X, y, 3, Z, kernel="matern52", jitter=1e-5, chunk_rows=256, device=0)
    created = [c for c in fake.calls if c[0] == "create_shard"]
    assert [(c[1], c[9], c[10]) for c in created] == [(16, 0, 3), (16, 1, 3), (18, 2, 3)]                 # split_rows' blocks
    assert all(c[2:9] == (4, 2, 0, capi.CUGP_KERNEL_MATERN52, 0, 1e-5, 256) for c in created)
    assert ("comm_create", True, 0, 0, 1, 0) in fake.calls                                                   # no id: a world of one
    assert (m.K, m.world, m.per, m.mine, m.nh) == (3, 1, 3, [0, 1, 2], 3)
    handles = [s._h.value for s in m.local_shards]
    assert m.lead is m.local_shards[0]
    m.set_loghyper([0.5, 1.0, -1.0])
    assert [c[1] for c in fake.calls[-3:]] == handles and all(c[0] == "set_loghyper" and c[3] == 0.5 for c in fake.calls[-3:])
    m.set_inducing(Z + 1.0)
    assert [c[1] for c in fake.calls[-3:]] == handles and all(c[0] == "set_inducing" for c in fake.calls[-3:])
    assert m.bound() == -2.5 and fake.calls[-1] == ("bound_grad", handles, 0x7, 3, 3, 0, 3, True, True)
    F, g = m.bound_grad()
    assert g.shape == (3,) and fake.calls[-1] == ("bound_grad", handles, 0x7, 3, 3, 1, 3, False, True)
    F, g, gZ = m.bound_grad_z()
    assert gZ.shape == (4, 2) and fake.calls[-1] == ("bound_grad", handles, 0x7, 3, 3, 2, 3, False, False)
    assert m.cg_solve(7).shape == (2, 4) and fake.calls[-1] == ("cg_solve", handles, 3, 3, 7, 0, 36)
    assert m.cg_solve(7, inducing=True).shape == (2, 4) and fake.calls[-1] == ("cg_solve", handles, 3, 3, 7, 1, 36)
    m.predict(rng.standard_normal((5, 2)), with_noise=False)
    assert fake.calls[-1] == ("predict", handles[0], 5, 0)                                                   # the lead answers
    m.close()
    assert [c for c in fake.calls[-4:]] == [("destroy", h) for h in handles] + [("comm_destroy",)]
    # a rank of a larger world owns every W-th shard; shards it does not own may be None
    with pytest.raises(ValueError, match="without a shard"):
        ss.ShardedSparseGP([(X, y)], Z, rank=0, world=2)
    with pytest.raises(ValueError, match="rational quadratic"):
        ss.ShardedSparseGP([(X, y)], Z, kernel="rq")
    with pytest.raises(ValueError, match="no data"):
        ss.ShardedSparseGP([None], Z)


def test_a_world_above_one_needs_nccl():
    rng = np.random.default_rng(0)
    X, y, Z = rng.standard_normal((20, 2)), rng.standard_normal(20), rng.standard_normal((4, 2))
    with pytest.raises(RuntimeError) as ei:
        ss.ShardedSparseGP([(X[:10], y[:10]), None], Z, rank=0, world=2)
    assert "needs an nccl process group" in str(ei.value) and "no torch / gloo fall-back" in str(ei.value)


BASE = ["--rows", "100", "--inputs", "x", "--labels", "y"]


def test_train_inducing_over_ranks(monkeypatch, capsys):
    parse = lambda argv: train.main(argv, parse_only=True)     # noqa: E731
    monkeypatch.setenv("WORLD_SIZE", "2")
    a = parse(["--numchunks", "2"] + BASE + ["--inducing", "8", "--learn-inducing"])
    assert (a.inducing, a.numchunks, a.learn_inducing) == (8, 2, True)
    for bad in (["--numchunks", "1"] + BASE + ["--inducing", "8"], ["--numchunks", "4"] + BASE + ["--inducing", "8"],
                ["--numchunks", "2"] + BASE + ["--inducing", "8", "--objective", "loo"]):
        with pytest.raises(SystemExit):
            parse(bad)
    assert "one chunk per process" in capsys.readouterr().err
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    assert parse(["--numchunks", "1"] + BASE + ["--inducing", "8"]).inducing == 8
    with pytest.raises(SystemExit):
        parse(["--numchunks", "2"] + BASE + ["--inducing", "8"])
