"""ShardedBCM.predict_grad on two gloo ranks, no GPU: the torch forms move the zero-padded [K][2 + 2 d][nt] rows (m, v,
dmean^T, dvar^T) that every local expert's predict_grad fills -- by the all-gather or the all-reduce of the objective's
rows -- and combine them on the host (poe_combine / poe_finish, poe_combine_grad).  For every rule, the reference's
product (combine=None) included, with and without the noise term, the two-rank result must equal the world-of-one result
bit for bit in all four outputs -- for an even (4) and an uneven (5) expert count and under both torch exchange forms."""
import os
import socket
import sys

import numpy as np
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = (None, "poe", "gpoe", "bcm", "rbcm")
HP = [0.3, 0.2, -1.1]


class ClosedFormExpert:
    """A stand-in expert of this test's own: a deterministic closed form of its data and the hyper-parameters with exact
    gradients -- m = sum_c sin(x_c + a_c), var_f = sf2 (1 - 0.9 exp(-|x - b|^2)) in (0, sf2], noisy var = var_f + sn2
    (the test is about the exchange and the combination, not about the expert)."""

    def __init__(self, n, d, device):
        self.hp = np.zeros(3)

    def set_data(self, X, y):
        self.a = X.mean(0) + y.mean()
        self.b = X[0] * 0.5

    def set_loghyperparam(self, hp):
        self.hp = np.array(hp, dtype=np.float64)

    def predict_grad(self, Xt, with_noise=True):
        sf2, sn2 = np.exp(2 * self.hp[1]), np.exp(2 * self.hp[2])
        m = np.sin(Xt + self.a).sum(1)
        dm = np.cos(Xt + self.a)
        e = 0.9 * np.exp(-((Xt - self.b) ** 2).sum(1))
        v = sf2 * (1.0 - e) + (sn2 if with_noise else 0.0)
        dv = sf2 * (2.0 * (Xt - self.b)) * e[:, None]
        return m, v, dm, dv


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
    Xt = np.vstack([X[:3], X[:5] * 0.7 - 0.1, X[:1] * 3.0])
    nt, dim = Xt.shape
    checked = 0
    for form in ("allgather", "allreduce"):
        os.environ["CUGP_BCM_EXCHANGE"] = form
        for K in (4, 5):
            ex = [(X[o:o + n], y[o:o + n]) for o, n in split_rows(128, K)]
            b = ShardedBCM(ex, rank=rank, world=world, expert_factory=ClosedFormExpert)
            one = ShardedBCM(ex, rank=0, world=1, expert_factory=ClosedFormExpert)
            assert b.exchange_form == form
            b.set_loghyper(HP)
            one.set_loghyper(HP)
            for mode in MODES:
                for with_noise in (True, False):
                    r2 = b.predict_grad(Xt, combine=mode, with_noise=with_noise)
                    assert b.predict_form == "torch"
                    r1 = one.predict_grad(Xt, combine=mode, with_noise=with_noise)
                    assert [a.shape for a in r2] == [(nt,), (nt,), (nt, dim), (nt, dim)]
                    for a2, a1 in zip(r2, r1):
                        assert same_bits(a2, a1), (form, K, mode, with_noise)
                        assert np.all(np.isfinite(a2))
                    assert np.all(r2[1] > 0)
                    checked += 1
            # what the world of one computes: the host rule on the experts' own predict_grad, expert order
            es = []
            for k in range(K):
                e = ClosedFormExpert(0, 0, 0)
                e.set_data(*ex[k])
                e.set_loghyperparam(HP)
                es.append(e.predict_grad(Xt, with_noise=False))
            m, v, dm, dv = (np.stack([r[i] for r in es]) for i in range(4))
            sf2, sn2 = gp.prior_scalars(np.array(HP))
            wm, wv = gp.poe_combine(np.stack([1.0 / v, (1.0 / v) * m], axis=1), "rbcm", sf2, sn2, True)
            wdm, wdv = gp.poe_combine_grad(m, v, dm, dv, "rbcm", sf2)
            got = b.predict_grad(Xt, combine="rbcm")
            for a, w in zip(got, (wm, wv, wdm, wdv)):
                assert same_bits(a, w), (form, K)
            try:
                b.predict_grad(Xt, combine="product")
            except ValueError:
                pass
            else:
                raise AssertionError("an unknown combine= name must raise ValueError")
    os.environ.pop("CUGP_BCM_EXCHANGE")
    q.put((rank, checked))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_input_gradients_match_world_of_one():
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
    assert [r[1] for r in res] == [2 * 2 * 5 * 2] * 2
