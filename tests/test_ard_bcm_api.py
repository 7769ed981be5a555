"""The ARD product-of-experts interface without a GPU: the new entry points are exported and bound with their argument
counts, the Python layer has its keywords, every argument error comes back as CUGP_ERR_INVALID before any device call
(a null or a dummy handle is never dereferenced), ARD x Matern raises, and two gloo ranks run ShardedBCM(ard=True) --
the real sharding, both torch.distributed exchange forms, rows of 1 + nh doubles -- on a CPU expert and reproduce the
in-process sum in expert order bit for bit."""
import ctypes as C
import inspect
import os
import socket
import sys

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

import cugp_amd.gp as gp
from cugp_amd import capi
from cugp_amd.bcm import ShardedBCM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = [("cugp_bcm_create_ard", 6), ("cugp_bcm_create_split_ard", 8), ("cugp_bcm_num_hyper", 2),
       ("cugp_bcm_set_loghyper_ard", 3), ("cugp_bcm_get_loghyper_ard", 3), ("cugp_bcm_loglik_grad_ard", 5),
       ("cugp_bcm_loglik_grad_rows_ard", 3), ("cugp_bcm_loglik_grad_rows_device_ard", 4),
       ("cugp_bcm_loglik_grad_allgather_ard", 5), ("cugp_bcm_cg_solve_ard", 5)]


@pytest.mark.parametrize("name, nargs", NEW)
def test_exported_and_bound(name, nargs):
    assert name in capi.SIGNATURES
    assert len(capi.SIGNATURES[name][1]) == nargs
    fn = getattr(capi.lib(), name)
    assert fn.restype is C.c_int and len(fn.argtypes) == nargs
    with open(os.path.join(ROOT, "include", "cugp.h")) as f:
        assert "int %s(" % name in f.read()


def test_python_keywords():
    for fn in (gp.BCM.__init__, gp.BCM.split, ShardedBCM.__init__):
        p = inspect.signature(fn).parameters
        assert "ard" in p and p["ard"].default is False, fn
    p = inspect.signature(gp.Comm.loglik_grad_allgather).parameters
    assert "nh" in p and p["nh"].default == 3
    for m in ("set_BCM_log_hyperparam", "get_loghyperparam", "loglik_grad", "loglik_grad_rows", "loglik_grad_rows_device",
              "expert", "cg_solve"):
        assert callable(getattr(gp.BCM, m))
    import cugp_amd.train as train
    assert "--ard" in inspect.getsource(train.main)


@pytest.mark.parametrize("kernel", ["matern32", "matern52"])
def test_ard_with_matern_raises_before_any_call(kernel):
    """The same ValueError as Covsum's, before the library is asked for anything."""
    with pytest.raises(ValueError, match="squared-exponential only"):
        gp.BCM([10, 10], 3, ard=True, kernel=kernel)
    X, y = np.zeros((20, 3)), np.zeros(20)
    with pytest.raises(ValueError, match="squared-exponential only"):
        gp.BCM.split(X, y, 2, ard=True, kernel=kernel)
    with pytest.raises(ValueError, match="squared-exponential only"):
        ShardedBCM([(X, y)], ard=True, kernel=kernel, expert_factory=lambda *a, **k: None)
    with pytest.raises(ValueError, match="squared-exponential only"):
        gp.Covsum(10, 3, ard=True, kernel=kernel)


DUMMY = C.c_void_p(0x1000)     # never dereferenced: the checks come first


@pytest.mark.parametrize("handle", [None, DUMMY], ids=["null", "dummy"])
def test_argument_errors(handle):
    L = capi.lib()
    v, ll, nh, ne = np.zeros(8), C.c_double(), C.c_int(), C.c_int()
    p = capi.ptr(v)
    INV = capi.CUGP_ERR_INVALID
    out = C.c_void_p()
    dev, rows = (C.c_int * 1)(0), (C.c_int * 2)(10, 10)
    assert L.cugp_bcm_create_ard(1, dev, 2, rows, 3, None) == INV and L.cugp_bcm_create_ard(0, dev, 2, rows, 3, C.byref(out)) == INV
    assert L.cugp_bcm_create_ard(1, None, 2, rows, 3, C.byref(out)) == INV and L.cugp_bcm_create_ard(1, dev, 0, rows, 3, C.byref(out)) == INV
    assert L.cugp_bcm_create_ard(1, dev, 2, None, 3, C.byref(out)) == INV and L.cugp_bcm_create_ard(1, dev, 2, rows, 0, C.byref(out)) == INV
    bad_rows = (C.c_int * 2)(10, 0)
    assert L.cugp_bcm_create_ard(1, dev, 2, bad_rows, 3, C.byref(out)) == INV
    assert L.cugp_bcm_create_split_ard(None, p, 8, 1, 2, 1, dev, C.byref(out)) == INV
    assert L.cugp_bcm_create_split_ard(p, None, 8, 1, 2, 1, dev, C.byref(out)) == INV
    assert L.cugp_bcm_create_split_ard(p, p, 0, 1, 2, 1, dev, C.byref(out)) == INV
    assert L.cugp_bcm_create_split_ard(p, p, 8, 0, 2, 1, dev, C.byref(out)) == INV
    assert L.cugp_bcm_create_split_ard(p, p, 8, 1, 9, 1, dev, C.byref(out)) == INV
    assert L.cugp_bcm_num_hyper(None, C.byref(nh)) == INV and L.cugp_bcm_num_hyper(handle, None) == INV
    assert L.cugp_bcm_set_loghyper_ard(None, p, 5) == INV and L.cugp_bcm_set_loghyper_ard(handle, None, 5) == INV
    assert L.cugp_bcm_set_loghyper_ard(handle, p, 2) == INV and L.cugp_bcm_set_loghyper_ard(handle, p, -1) == INV
    assert b"cugp_bcm_set_loghyper_ard" in L.cugp_last_error()
    assert L.cugp_bcm_get_loghyper_ard(None, p, 5) == INV and L.cugp_bcm_get_loghyper_ard(handle, None, 5) == INV
    assert L.cugp_bcm_get_loghyper_ard(handle, p, 0) == INV
    assert L.cugp_bcm_loglik_grad_ard(None, C.byref(ll), p, 5, None) == INV
    assert L.cugp_bcm_loglik_grad_ard(handle, C.byref(ll), p, 1, None) == INV
    assert b"cugp_bcm_loglik_grad_ard" in L.cugp_last_error()
    assert L.cugp_bcm_loglik_grad_rows_ard(None, p, 5) == INV and L.cugp_bcm_loglik_grad_rows_ard(handle, None, 5) == INV
    assert L.cugp_bcm_loglik_grad_rows_ard(handle, p, 2) == INV
    slot = (C.c_int * 1)(0)
    assert L.cugp_bcm_loglik_grad_rows_device_ard(None, DUMMY, slot, 5) == INV
    assert L.cugp_bcm_loglik_grad_rows_device_ard(handle, None, slot, 5) == INV
    assert L.cugp_bcm_loglik_grad_rows_device_ard(handle, DUMMY, None, 5) == INV
    assert L.cugp_bcm_loglik_grad_rows_device_ard(handle, DUMMY, slot, 2) == INV
    assert L.cugp_bcm_loglik_grad_allgather_ard(handle, None, 1, 5, p) == INV
    assert L.cugp_bcm_loglik_grad_allgather_ard(handle, DUMMY, 0, 5, p) == INV
    assert L.cugp_bcm_loglik_grad_allgather_ard(handle, DUMMY, 1, 5, None) == INV
    assert L.cugp_bcm_loglik_grad_allgather_ard(handle, DUMMY, 1, 2, p) == INV
    assert b"cugp_bcm_loglik_grad_allgather_ard" in L.cugp_last_error()
    assert L.cugp_bcm_cg_solve_ard(None, 10, None, 0, C.byref(ne)) == INV
    # the 3-entry calls keep their null checks
    assert L.cugp_bcm_set_loghyper(None, p) == INV and L.cugp_bcm_set_loghyper(handle, None) == INV
    assert L.cugp_bcm_get_loghyper(handle, None) == INV and L.cugp_bcm_loglik_grad_rows(handle, None) == INV
    assert L.cugp_bcm_loglik_grad(None, C.byref(ll), p, None) == INV and L.cugp_bcm_cg_solve(None, 5, None, 0, C.byref(ne)) == INV


# ---------------------------------------------------------------------------------------------- two gloo ranks
class StandinExpert:
    """Stand-in for gp.Covsum(ard=True) with the same enqueue / fetch / predict surface: tests/truth.py's fp64 stand-in."""

    def __init__(self, n, d, device, ard=False):
        assert ard is True                       # ShardedBCM(ard=True) tells an injected factory
        self.d = d
        self.hp = np.zeros(d + 2)

    def set_data(self, X, y):
        self.X, self.y = X, y

    def set_loghyperparam(self, hp):
        self.hp = np.array(hp, dtype=np.float64)
        assert self.hp.shape == (self.d + 2,)

    def enqueue(self, want_grad=True):
        pass

    def _eval(self, Xt):
        import truth
        return truth.standin(truth.ARD(self.hp), self.X, self.y, Xt)

    def fetch(self):
        ll, g, _, _ = self._eval(self.X[:1])
        return float(ll), g

    def compute_test_means_and_variances(self, X, y, Xt):
        return self._eval(Xt)[2:]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from conftest import synth
    from cugp_amd.bcm import ShardedBCM, split_rows
    d, hp = 3, [0.9, 0.3, 1.6, 0.2, -1.0]               # nh = 5
    X, y = synth(130, d=d, seed=17, scale=4.0)
    Xt = np.vstack([X[:3], X[:5] * 0.7 - 0.1])
    out = {}
    for K in (4, 5):                                     # even, and uneven: rank 1 leaves a zero slot in the all-gather
        experts = [(X[o:o + n], y[o:o + n]) for o, n in split_rows(130, K)]
        single = ShardedBCM(experts, rank=0, world=1, expert_factory=StandinExpert, ard=True)
        single.set_loghyper(hp)
        sl, sg, sper = single.loglik_grad()
        sm, sv = single.predict(Xt)
        # ... and by hand: every expert alone, summed in expert order
        ll, g = 0.0, None
        for k, (Xk, yk) in enumerate(experts):
            e = StandinExpert(len(yk), d, 0, ard=True)
            e.set_data(Xk, yk)
            e.set_loghyperparam(hp)
            lk, gk = e.fetch()
            ll, g = ll + lk, (gk.copy() if k == 0 else g + gk)
        assert sl == ll and np.array_equal(sg, g) and sg.shape == (5,)
        for form in ("allgather", "allreduce"):          # both torch.distributed forms
            os.environ["CUGP_BCM_EXCHANGE"] = form
            mine = [experts[k] if k % world == rank else None for k in range(K)]
            b = ShardedBCM(mine, rank=rank, world=world, expert_factory=StandinExpert, ard=True, d=d)
            os.environ.pop("CUGP_BCM_EXCHANGE")
            assert b.exchange_form == form and b.ard and b.nh == 5
            assert b.mine == [k for k in range(K) if k % world == rank]
            b.set_loghyper(hp)
            bl, bg, bper = b.loglik_grad()
            assert bl == sl and np.array_equal(bg, sg) and np.array_equal(bper, sper), (rank, K, form, bl, sl)
            m, v = b.predict(Xt)
            assert np.array_equal(m, sm) and np.array_equal(v, sv), (rank, K, form)
            if form == "allgather":
                tr = b.cg_solve(4)
                assert tr.shape[1] == 6 and b.hp.shape == (5,)
                out[K] = (b.hp.copy(), tr)
    q.put((rank, out))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_sharded_ard_bcm():
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=240) for _ in range(world)], key=lambda t: t[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    (_, r0), (_, r1) = res
    for K in (4, 5):                                     # both ranks ran the same optimisation on identical sums
        assert np.array_equal(r0[K][0], r1[K][0]) and np.array_equal(r0[K][1], r1[K][1])
