"""The combination rules through ShardedBCM on two gloo ranks, no GPU: the torch forms all-reduce the zero-padded
[K][2][nt] LATENT rows that every local expert's predict_latent fills and combine them with the host's cugp_poe_combine.
For every rule the two-rank result must equal the world-of-one result bit for bit -- for an even (4) and an uneven (5)
expert count and under both torch exchange forms -- and combine=None must stay poe_finish of today's noisy rows."""
import os
import socket
import sys

import numpy as np
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = ("poe", "gpoe", "bcm", "rbcm")
HP = [1.2, 0.7, -0.3]


class LatentOracleExpert:
    """A stand-in expert of this test's own: the CPU oracle's prediction, and predict_latent as its noisy variance
    minus sn2 (any deterministic latent prediction serves: the test is about the exchange and the combination)."""

    def __init__(self, n, d, device):
        from oracle.oracle_py import Oracle
        self.o = Oracle()
        self.hp = np.zeros(3)

    def set_data(self, X, y):
        self.X, self.y = X, y

    def set_loghyperparam(self, hp):
        self.hp = np.array(hp, dtype=np.float64)

    def compute_test_means_and_variances(self, X, y, Xt):
        return self.o.predict(self.X, self.y, self.hp, Xt)

    def predict_latent(self, Xt):
        m, v = self.o.predict(self.X, self.y, self.hp, Xt)
        return m, v - np.exp(2 * self.hp[2])


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _worker(rank, world, port, q):
    try:
        _body(rank, world, port, q)
    except BaseException as exc:                      # the parent reads the failure instead of waiting for a result
        q.put((rank, repr(exc)))
        raise


def _body(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import cugp_amd.gp as gp
    from cugp_amd.bcm import ShardedBCM, split_rows
    d = np.load(os.path.join(ROOT, "tests", "golden", "data_si128.npz"))
    X, y = d["X"], d["y"]
    Xt = np.vstack([X[:3], X[:5] * 0.7 - 0.1, X[:1] * 1e3])        # the last one far outside the data
    checked = 0
    for form in ("allgather", "allreduce"):
        os.environ["CUGP_BCM_EXCHANGE"] = form
        for K in (4, 5):
            ex = [(X[o:o + n], y[o:o + n]) for o, n in split_rows(128, K)]
            b = ShardedBCM(ex, rank=rank, world=world, expert_factory=LatentOracleExpert)
            one = ShardedBCM(ex, rank=0, world=1, expert_factory=LatentOracleExpert)
            assert b.exchange_form == form
            b.set_loghyper(HP)
            one.set_loghyper(HP)
            for mode in MODES:
                for with_noise in (True, False):
                    m2, v2 = b.predict(Xt, combine=mode, with_noise=with_noise)
                    assert b.predict_form == "torch"
                    m1, v1 = one.predict(Xt, combine=mode, with_noise=with_noise)
                    assert same_bits(m2, m1) and same_bits(v2, v1), (form, K, mode, with_noise)
                    assert np.all(np.isfinite(m2)) and np.all(v2 > 0)
                    checked += 1
            # combine=None: poe_finish of today's noisy rows, expert order
            m, v = b.predict(Xt)
            sp, spm = np.zeros(len(Xt)), np.zeros(len(Xt))
            for k in range(K):
                e = LatentOracleExpert(0, 0, 0)
                e.set_data(*ex[k])
                e.set_loghyperparam(HP)
                mk, vk = e.compute_test_means_and_variances(None, None, Xt)
                sp += 1.0 / vk
                spm += (1.0 / vk) * mk
            mf, vf = gp.poe_finish(sp, spm)
            assert same_bits(m, mf) and same_bits(v, vf), (form, K)
            try:
                b.predict(Xt, combine="product")
            except ValueError:
                pass
            else:
                raise AssertionError("an unknown combine= name must raise ValueError")
    os.environ.pop("CUGP_BCM_EXCHANGE")
    q.put((rank, checked))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_combination_rules_match_world_of_one():
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=240) for _ in range(world)], key=lambda t: t[0])
    for p in procs:
        p.join(60)
    assert all(p.exitcode == 0 for p in procs), res
    assert [r[1] for r in res] == [2 * 2 * 4 * 2] * 2
