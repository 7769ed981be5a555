"""Sparse variational GP regression with its DATA ROWS sharded over ranks, one process per GPU (cugp_sparse_sharded_*;
DESIGN.md section 32).

K shards hold disjoint row blocks (X_k, y_k) of ONE data set; shard k lives on rank k mod W in slot k // W of that rank
(bcm.gather_row_index's convention), Z and the hyper-parameters are the same everywhere.  An evaluation is SparseGP's cut at
the two points where the shards meet: one all-gather of the shards' P_k, q_k, y_k'y_k, n_k and one of their gradient rows,
both inside the library on the evaluation's stream, each followed by a sum in global shard order -- so every rank holds the
same bits, they depend on (data, K) only, and with K = 1 they are SparseGP's.  The result is one model: the bound, its
gradients and the predictive distribution of all N rows, not a product of experts.

There is no torch / gloo fall-back: the exchange is the library's RCCL all-gather or, in a world of one, nothing at all.
"""
import ctypes as C

import numpy as np

from . import capi
from . import gp as _gp
from .capi import check, f64

NO_NCCL = ("ShardedSparseGP: a world above one needs an nccl process group -- the exchange runs inside the library over "
           "RCCL, there is no torch / gloo fall-back")


def shard_owner(k, world):
    """Shard k lives on rank k mod W."""
    return k % world


def slots_per_rank(K, world):
    """per = ceil(K / W): the slots every rank's block of an exchange has."""
    return -(-int(K) // int(world))


def slot_index(k, world, per):
    """Where shard k lies among the world * per gathered slots: rank k mod W, slot k // W (bcm.gather_row_index)."""
    return shard_owner(k, world) * per + k // world


def split_rows(N, K):
    """bcm.split_rows: contiguous blocks of floor(N / K) rows, the remainder to the last."""
    part = N // K
    return [(k * part, part if k < K - 1 else N - part * (K - 1)) for k in range(K)]


class _Shard(_gp.SparseGP):
    """A SparseGP handle that is shard `shard` of `nshards` (cugp_sparse_create_shard): data, Z and hyper-parameters are
    set as on any SparseGP; the evaluating calls refuse, and predictions answer on the lead of a sharded evaluation only."""

    def __init__(self, n, m, d, shard, nshards, device=0, kernel="se", ard=False, jitter=1e-6, chunk_rows=0):
        self.n, self.m, self.d, self.device = int(n), int(m), int(d), int(device)
        self._kind, self.ard = _gp.kernel_spec(kernel, ard)
        if self._kind == capi.CUGP_KERNEL_RQ:
            raise ValueError("ShardedSparseGP: the rational quadratic kernel is not built for the sparse model")
        self.nh = self.d + 2 if self.ard else 3
        self.jitter, self.chunk_rows = float(jitter), int(chunk_rows)
        self.shard, self.nshards = int(shard), int(nshards)
        self._h = C.c_void_p()
        check(capi.lib().cugp_sparse_create_shard(self.n, self.m, self.d, self.device, self._kind, 1 if self.ard else 0,
                                                  self.jitter, self.chunk_rows, self.shard, self.nshards, C.byref(self._h)))

    def info(self):
        """(shard, nshards, N of the last sharded evaluation) as the library holds them (cugp_sparse_shard_info)."""
        k, K, N = C.c_int(), C.c_int(), C.c_longlong()
        check(capi.lib().cugp_sparse_shard_info(self._h, C.byref(k), C.byref(K), C.byref(N)))
        return k.value, K.value, N.value


class ShardedSparseGP:
    """K row shards of one sparse model over `world` ranks.  `shards` is a list of K (X_k, y_k) pairs, None where this rank
    does not own the shard; K >= world, every n_k >= 1, unequal where the caller likes.  Z [m, d], kernel, ard, jitter and
    chunk_rows are SparseGP's and the same on every rank (the library checks what it can: the first exchange of every
    evaluation carries m, d, kernel, ard, nh, K, the jitter's bits and a fingerprint of the hyper-parameters' and Z's bits).
    group: the torch.distributed group rank 0's RCCL id is broadcast through, as ShardedBCM's library form does; with
    world == 1 none is needed (under an initialised nccl group the one rank still goes through a real communicator)."""

    def __init__(self, shards, Z, rank=0, world=1, device=0, group=None, kernel="se", ard=False, jitter=1e-6, chunk_rows=0):
        self.K, self.rank, self.world, self.device = len(shards), int(rank), int(world), int(device)
        if self.K < self.world:
            raise ValueError("ShardedSparseGP: %d shards over %d ranks leave a rank without a shard" % (self.K, self.world))
        Z = f64(Z)
        self.m, self.d = Z.shape
        self.per = slots_per_rank(self.K, self.world)
        self.mine = [k for k in range(self.K) if shard_owner(k, self.world) == self.rank]
        missing = [k for k in self.mine if shards[k] is None]
        if missing:
            raise ValueError("ShardedSparseGP: rank %d owns shards %s but was given no data for them" % (self.rank, missing))
        uid = self._unique_id(group)
        self._shards, self._comm = [], None
        try:
            for k in self.mine:
                X, y = f64(shards[k][0]), f64(shards[k][1])
                s = _Shard(X.shape[0], self.m, self.d, k, self.K, device=self.device, kernel=kernel, ard=ard, jitter=jitter,
                           chunk_rows=chunk_rows)
                self._shards.append(s)
                s.set_data(X, y)
                s.set_inducing(Z)
            self._comm = _gp.Comm(uid, self.rank, self.world, self.device)
        except Exception:
            self.close()
            raise
        self._lead = self._shards[0]
        self.nh, self.ard = self._lead.nh, self._lead.ard

    def _unique_id(self, group):
        """Rank 0's RCCL id through the process group that already exists (None: a world of one without a communicator)."""
        if self.world == 1:
            try:
                import torch.distributed as dist
            except ImportError:
                return None
            if not (dist.is_available() and dist.is_initialized() and dist.get_backend(group) == "nccl"):
                return None
            return _gp.Comm.unique_id()                               # one rank, but through a real communicator
        import torch
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_backend(group) != "nccl":
            raise RuntimeError(NO_NCCL)
        idt = torch.zeros(_gp.Comm.ID_BYTES, dtype=torch.uint8)
        if self.rank == 0:
            idt = torch.frombuffer(bytearray(_gp.Comm.unique_id()), dtype=torch.uint8).clone()
        idt = idt.to(torch.device("cuda", self.device))
        dist.broadcast(idt, src=0, group=group)
        return bytes(idt.cpu().numpy().tobytes())

    @classmethod
    def split(cls, X, y, K, Z, rank=0, world=1, **kw):
        """A model over (X, y) cut into K contiguous row blocks (split_rows); only this rank's blocks are copied."""
        X, y = f64(X), f64(y)
        shards = [(X[r0:r0 + n], y[r0:r0 + n]) if shard_owner(k, world) == rank else None
                  for k, (r0, n) in enumerate(split_rows(X.shape[0], int(K)))]
        return cls(shards, Z, rank=rank, world=world, **kw)

    def close(self):
        for s in getattr(self, "_shards", []):
            s.close()
        self._shards = []
        if getattr(self, "_comm", None) is not None:
            self._comm.close()
            self._comm = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def lead(self):
        """The first local shard: after an evaluation it holds the global M side and answers the predictions."""
        return self._lead

    @property
    def local_shards(self):
        return list(self._shards)

    def _handles(self):
        return [s._h for s in self._shards]

    # -- state: every local shard gets the same bits
    def set_loghyper(self, hp):
        for s in self._shards:
            s.set_loghyperparam(hp)

    set_loghyperparam = set_loghyper

    def get_loghyper(self):
        return self._lead.get_loghyperparam()

    def set_inducing(self, Z):
        for s in self._shards:
            s.set_inducing(Z)

    def get_inducing(self):
        return self._lead.get_inducing()

    # -- the objective
    def _eval(self, what):
        return self._comm.sparse_sharded_bound_grad(self._handles(), self.per, self.K, what, self.nh, self.m, self.d)

    def bound(self):
        """F of all N rows."""
        return self._eval(0)[0]

    def bound_grad(self):
        """(F, g): the bound and the gradient of -F [nh]."""
        return self._eval(1)

    def bound_grad_z(self):
        """(F, g, gZ): bound_grad and the gradient of -F with respect to the inducing inputs [m, d]."""
        return self._eval(2)

    def cg_solve(self, budget=100, inducing=False):
        """SparseGP.cg_solve on the sharded objective: every rank runs the same loop on the same numbers; the end point
        (and moved inducing inputs) are written into every local shard.  -> the trace [n_iterates, nh + 1]."""
        return self._comm.sparse_sharded_cg_solve(self._handles(), self.per, self.K, budget, self.nh, inducing=inducing)

    # -- predictions: the lead's, from the state of the last evaluation; they raise when it is stale and never evaluate
    def predict(self, Xtest, with_noise=True):
        return self._lead.predict(Xtest, with_noise=with_noise)

    def predict_joint(self, Xtest, with_noise=True):
        return self._lead.predict_joint(Xtest, with_noise=with_noise)

    def sample_posterior(self, Xtest, nsamples, **kw):
        return self._lead.sample_posterior(Xtest, nsamples, **kw)

    def predict_grad(self, Xtest, with_noise=True, want_var_grad=True):
        return self._lead.predict_grad(Xtest, with_noise=with_noise, want_var_grad=want_var_grad)
