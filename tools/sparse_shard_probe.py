"""What sharding the rows of the sparse model costs and buys (needs the built library):

    python tools/sparse_shard_probe.py --json profiles/sparse_shard_probe.json     # one GPU: N = 1e5; M = 512, 1024, 2048; D = 10
    torchrun --nproc-per-node W tools/sparse_shard_probe.py --sizes 1000000 --json out.json   # W ranks of N / W rows each

One GPU: per (N, M) the world-of-one sharded evaluation with ONE shard (K = 1: no RCCL, both reduces are copies of
M^2 + M + 2 and nh - 1 (+ m d) doubles) beside SparseGP on the same data in the same process, ALTERNATING call by call at
fresh hyper-parameter vectors; host clock around the synchronous call, in ms: the median and the spread (min .. max) of
--reps calls of each, for bound_grad and bound_grad_z, and whether the two gave the same bits at the last vector.
Under torchrun: every rank times the W-rank evaluation of its N / W rows (one shard per rank, both all-gathers inside);
rank 0 also times SparseGP over all N rows on its card and writes the file.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

CHUNK = 16384


def hyper(d, i):
    return [float(np.log(3.0)) + 1e-3 * i, 0.0, float(np.log(0.1))]


def stats(ts):
    return dict(median_ms=float(np.median(ts)), min_ms=float(np.min(ts)), max_ms=float(np.max(ts)))


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return 1e3 * (time.perf_counter() - t0), out


def same(a, b):
    return all(np.array_equal(np.asarray(x, dtype=np.float64).view(np.uint64), np.asarray(y, dtype=np.float64).view(np.uint64))
               for x, y in zip(a, b))


def one_gpu(n, m, d, reps):
    import cugp_amd.gp as gp
    from conftest import synth
    from cugp_amd.sparse_sharded import ShardedSparseGP
    X, y = synth(n, d, seed=15618)
    rows = np.sort(np.random.default_rng(0).choice(n, m, replace=False))
    Z = np.ascontiguousarray(X[rows])
    ref = gp.SparseGP(n, m, d, chunk_rows=CHUNK)
    ref.set_data(X, y)
    ref.set_inducing(Z)
    sh = ShardedSparseGP([(X, y)], Z, chunk_rows=CHUNK)
    out = dict(n=n, m=m, d=d, shards=1, world=1, chunks=len(ref.plan()),
               reduce_doubles=[(-(-m // 128) * 128) ** 2 + -(-m // 128) * 128 + 2, 2 + m * d])
    for name, a, b in (("bound_grad", ref.bound_grad, sh.bound_grad), ("bound_grad_z", ref.bound_grad_z, sh.bound_grad_z)):
        ta, tb, last = [], [], None
        for i in range(1 + reps):                                     # (one warm-up pair), alternating
            hp = hyper(d, (100 if name == "bound_grad" else 200) + i)
            ref.set_loghyperparam(hp)
            sh.set_loghyper(hp)
            ms_a, ra = timed(a)
            ms_b, rb = timed(b)
            if i:
                ta.append(ms_a)
                tb.append(ms_b)
            last = same(ra, rb)
        out[name] = dict(sparsegp=stats(ta), sharded=stats(tb), same_bits=bool(last),
                         sharded_over_sparsegp=float(np.median(tb) / np.median(ta)),
                         inside_spread=bool(np.min(ta) <= np.median(tb) <= np.max(ta)))
    ref.close()
    sh.close()
    return out


def ranks(n, m, d, reps, rank, world):
    import torch
    import torch.distributed as dist
    import cugp_amd.gp as gp
    from conftest import synth
    from cugp_amd.sparse_sharded import ShardedSparseGP, split_rows
    X, y = synth(n, d, seed=15618)
    rows = np.sort(np.random.default_rng(0).choice(n, m, replace=False))
    Z = np.ascontiguousarray(X[rows])
    r0, cnt = split_rows(n, world)[rank]
    shards = [(X[r0:r0 + cnt], y[r0:r0 + cnt]) if k == rank else None for k in range(world)]
    sh = ShardedSparseGP(shards, Z, rank=rank, world=world, device=rank, chunk_rows=CHUNK)
    out = dict(n=n, m=m, d=d, shards=world, world=world)
    for name, fn in (("bound_grad", sh.bound_grad), ("bound_grad_z", sh.bound_grad_z)):
        ts = []
        for i in range(1 + reps):
            sh.set_loghyper(hyper(d, 300 + i))
            dist.barrier()
            torch.cuda.synchronize()
            ms, _ = timed(fn)
            if i:
                ts.append(ms)
        out[name] = dict(sharded=stats(ts))
    sh.close()
    if rank == 0:
        ref = gp.SparseGP(n, m, d, device=0, chunk_rows=CHUNK)
        ref.set_data(X, y)
        ref.set_inducing(Z)
        for name, fn in (("bound_grad", ref.bound_grad), ("bound_grad_z", ref.bound_grad_z)):
            ts = []
            for i in range(1 + reps):
                ref.set_loghyperparam(hyper(d, 300 + i))
                ms, _ = timed(fn)
                if i:
                    ts.append(ms)
            out[name]["sparsegp_one_card"] = stats(ts)
            out[name]["speedup"] = float(np.median(ts) / out[name]["sharded"]["median_ms"])
        ref.close()
    dist.barrier()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[100000])
    ap.add_argument("--inducing", type=int, nargs="+", default=[512, 1024, 2048])
    ap.add_argument("--dims", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    if world > 1:
        import torch
        import torch.distributed as dist
        torch.cuda.set_device(rank)
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", rank))
    rows = []
    for n in args.sizes:
        for m in args.inducing:
            r = ranks(n, m, args.dims, args.reps, rank, world) if world > 1 else one_gpu(n, m, args.dims, args.reps)
            rows.append(r)
            if rank == 0:
                print(json.dumps(r), flush=True)
    if world > 1:
        import torch.distributed as dist
        dist.destroy_process_group()
    if args.json and rank == 0:
        from cugp_amd import capi
        doc = dict(build_id=(capi.lib().cugp_build_id() or b"unknown").decode(), reps=args.reps, chunk_rows=CHUNK, world=world,
                   rows=rows)
        with open(args.json, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
