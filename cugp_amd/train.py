"""Distributed BCM training driver -- the MI355X counterpart of cuda_scalingdist/main.cpp.

Reference CLI (harness.sh:53-59):  ./gp $HOSTNAME $MASTER $W numchunks N D inprefix labprefix
Here, one process per GPU on one node:

    python -m torch.distributed.run --nnodes=1 --nproc-per-node W --master-addr 127.0.0.1 \
        -m cugp_amd.train --numchunks 16 --rows 1500 --inputs <prefix> --labels <prefix> [--test-rows T]

Chunk i is <prefix>i.txt and goes to rank i mod W (cg_solver.cpp:93); hyper-parameters start at
{2,2,2} (main.cpp:298-301); cg_solve with the reference's 100-evaluation budget; rank 0 prints the
"PLEASE-SEE 3" line and the training time like the reference does (cg_solver.cpp:518, main.cpp:305).
"""
import argparse
import os
import time

import numpy as np


def start_vector(hp, nh, kernel, ard=False):
    """The start [log l, log sigma_f, log sigma_n] of --hp widened to a handle's nh entries: the length scale repeated,
    a rational quadratic kernel's log alpha = 0 behind the length scales, then the two variances."""
    from .gp import kernel_spec, num_hyper
    shape = num_hyper(kernel_spec(kernel, ard)[0], False, 1) - 3          # the family's shape parameters
    return [hp[0]] * (nh - 2 - shape) + [0.0] * shape + list(hp[1:])


def train_loo(args, local):
    """One expert, conjugate gradients on -L_LOO (Covsum.cg_solve_loo); prints what the default objective's run prints."""
    from . import dataset
    from .gp import Covsum
    X, y = dataset.load_chunk("%s0.txt" % args.inputs, "%s0.txt" % args.labels)
    Xt, yt = X[args.rows:args.rows + args.test_rows], y[args.rows:args.rows + args.test_rows]
    X, y = X[:args.rows], y[:args.rows]
    g = Covsum(X.shape[0], X.shape[1], local, ard=args.ard, kernel=args.kernel)
    g.set_loghyperparam(start_vector(args.hp, g.nh, args.kernel, args.ard))
    g.set_data(X, y)
    t0 = time.perf_counter()
    trace = g.cg_solve_loo(args.budget)
    dt = time.perf_counter() - t0
    hp = g.get_loghyperparam()
    print("\n\n PLEASE-SEE %d : %s\n" % (g.nh, ", ".join("%f" % v for v in hp)))
    print("TOTAL training time = %f  (%d iterates, final -L_LOO %.9g)" % (dt, trace.shape[0], trace[-1, -1]))
    if args.test_rows > 0:
        m, v = g.compute_test_means_and_variances(X, y, Xt)
        print("NLPP = %.12g" % Covsum.get_negative_log_predprob(yt, m, v))
    g.close()


def train_sparse(args, local):
    """One model over chunk 0's rows with --inducing M inducing inputs drawn from them (SparseGP.from_subset), conjugate
    gradients on the negative variational bound; prints what the default objective's run prints."""
    from . import dataset
    from .gp import Covsum, SparseGP, kernel_spec
    X, y = dataset.load_chunk("%s0.txt" % args.inputs, "%s0.txt" % args.labels)
    Xt, yt = X[args.rows:args.rows + args.test_rows], y[args.rows:args.rows + args.test_rows]
    X, y = X[:args.rows], y[:args.rows]
    ard = kernel_spec(args.kernel, args.ard)[1]
    g = SparseGP.from_subset(X, y, args.inducing, device=local, kernel=args.kernel, ard=args.ard)
    g.set_loghyperparam([args.hp[0]] * (g.nh - 2) + list(args.hp[1:]) if ard else args.hp)
    t0 = time.perf_counter()
    trace = g.cg_solve(args.budget, inducing=args.learn_inducing)
    dt = time.perf_counter() - t0
    hp = g.get_loghyperparam()
    print("\n\n PLEASE-SEE %d : %s\n" % (g.nh, ", ".join("%f" % v for v in hp)))
    print("TOTAL training time = %f  (%d iterates, final -F %.9g)" % (dt, trace.shape[0], trace[-1, -1]))
    if args.test_rows > 0:
        m, v = g.predict(Xt, with_noise=True)
        print("NLPP = %.12g" % Covsum.get_negative_log_predprob(yt, m, v))
    g.close()


def train_sparse_sharded(args, rank, local, world):
    """--inducing M under WORLD_SIZE > 1: ONE sparse model over the rows of all chunks, chunk r on rank r
    (ShardedSparseGP, one shard per rank; the process group is up).  The inducing inputs are M of chunk 0's rows, drawn as
    train_sparse draws them and broadcast from rank 0; every rank runs the same conjugate gradients; rank 0 prints."""
    import torch
    import torch.distributed as dist
    from . import dataset
    from .gp import Covsum, kernel_spec
    from .sparse_sharded import ShardedSparseGP
    X, y = dataset.load_chunk("%s%d.txt" % (args.inputs, rank), "%s%d.txt" % (args.labels, rank))
    Xt, yt = X[args.rows:args.rows + args.test_rows], y[args.rows:args.rows + args.test_rows]
    X, y = X[:args.rows], y[:args.rows]
    Zt = torch.zeros((args.inducing, X.shape[1]), dtype=torch.float64, device=torch.device("cuda", local))
    if rank == 0:
        rows = np.sort(np.random.default_rng(0).choice(X.shape[0], args.inducing, replace=False))
        Zt.copy_(torch.from_numpy(np.ascontiguousarray(X[rows])))
    dist.broadcast(Zt, src=0)
    shards = [(X, y) if k == rank else None for k in range(world)]
    g = ShardedSparseGP(shards, Zt.cpu().numpy(), rank=rank, world=world, device=local, kernel=args.kernel, ard=args.ard)
    ard = kernel_spec(args.kernel, args.ard)[1]
    g.set_loghyper([args.hp[0]] * (g.nh - 2) + list(args.hp[1:]) if ard else args.hp)
    t0 = time.perf_counter()
    trace = g.cg_solve(args.budget, inducing=args.learn_inducing)
    dt = time.perf_counter() - t0
    if rank == 0:
        print("\n\n PLEASE-SEE %d : %s\n" % (g.nh, ", ".join("%f" % v for v in g.get_loghyper())))
        print("TOTAL training time = %f  (%d iterates, final -F %.9g, %d ranks)" % (dt, trace.shape[0], trace[-1, -1], world))
    if args.test_rows > 0:
        g.bound()                                                     # the end point's state on every rank's lead
        if rank == 0:
            m, v = g.predict(Xt, with_noise=True)
            print("NLPP = %.12g" % Covsum.get_negative_log_predprob(yt, m, v))
    g.close()
    dist.barrier()
    dist.destroy_process_group()


def main(argv=None, parse_only=False):
    """parse_only: -> the parsed arguments (--objective loo and --inducing are refused there, before any device is
    touched, where they are not built)."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--numchunks", type=int, required=True)
    ap.add_argument("--rows", type=int, required=True, help="training rows per chunk (numtrain)")
    ap.add_argument("--inputs", required=True, help="input file prefix")
    ap.add_argument("--labels", required=True, help="label file prefix")
    ap.add_argument("--hp", type=float, nargs=3, default=[2.0, 2.0, 2.0])
    ap.add_argument("--budget", type=int, default=100)
    ap.add_argument("--test-rows", type=int, default=0, help="rows after --rows in chunk 0 used as a held-out set")
    ap.add_argument("--backend", default="nccl")
    ap.add_argument("--kernel", default="se", choices=["se", "matern32", "matern52", "matern32_ard", "matern52_ard", "rq", "rq_ard"],
                    help="covariance family of every expert (the same on every rank); the _ard names: one length scale "
                         "per input dimension with that kind, the start as --ard's; rq / rq_ard: rational quadratic, "
                         "log alpha starts at 0 (not with --sparse)")
    ap.add_argument("--ard", action="store_true",
                    help="one length scale per input dimension (squared exponential only): the start is "
                         "[hp0] * d + [hp1, hp2]")
    ap.add_argument("--combine", default=None, choices=["poe", "gpoe", "bcm", "rbcm"],
                    help="how the held-out prediction combines the experts' LATENT distributions (with the noise added "
                         "for the NLPP); absent: the reference's product of the noisy predictions")
    ap.add_argument("--objective", default="ll", choices=["ll", "loo"],
                    help="what cg_solve minimises: ll, the negative marginal log-likelihood (the reference's), or loo, the "
                         "negative sum of the leave-one-out log predictive densities (GPML 5.4.2) -- one expert in one "
                         "process only (--numchunks 1): there is no LOO for a product of experts")
    ap.add_argument("--inducing", type=int, default=0, metavar="M",
                    help="sparse variational GP regression on M inducing inputs, a random subset of the training rows, "
                         "instead of the exact model: cg_solve maximises the variational bound -- one model (--objective ll): "
                         "--numchunks 1 in one process, or under WORLD_SIZE > 1 one chunk per rank, the rows of all "
                         "chunks sharded over the ranks")
    ap.add_argument("--learn-inducing", action="store_true",
                    help="with --inducing: the inducing inputs are learned together with the hyper-parameters (conjugate "
                         "gradients over both) instead of staying on the rows they were drawn from")
    args = ap.parse_args(argv)
    if args.learn_inducing and not args.inducing:
        ap.error("--learn-inducing needs --inducing M")
    if args.inducing < 0 or args.inducing > args.rows:
        ap.error("--inducing must lie between 1 and --rows")
    nproc = int(os.environ.get("WORLD_SIZE", "1"))
    if args.inducing and (args.numchunks != nproc or args.objective != "ll"):
        ap.error("--inducing needs --objective ll and --numchunks 1 in one process, or one chunk per process under "
                 "WORLD_SIZE > 1 (the rows sharded over the ranks): the sparse model is built for a single model over all rows")
    if args.objective == "loo" and (args.numchunks != 1 or int(os.environ.get("WORLD_SIZE", "1")) != 1):
        ap.error("--objective loo needs --numchunks 1 and one process: leave-one-out is built for a single expert")
    if parse_only:
        return args

    import torch
    import torch.distributed as dist
    from . import dataset
    from .bcm import ShardedBCM, expert_owner
    from .gp import Covsum

    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    torch.cuda.set_device(local)
    if args.objective == "loo":
        return train_loo(args, local)
    if args.inducing and world == 1:
        return train_sparse(args, local)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(args.backend, rank=rank, world_size=world)

    if args.inducing:
        return train_sparse_sharded(args, rank, local, world)
    mine = {k for k in range(args.numchunks) if expert_owner(k, world) == rank}
    shards = dataset.load_shards(args.inputs, args.labels, args.numchunks, rows=None, only=mine)
    experts = [None if s is None else (s[0][:args.rows], s[1][:args.rows]) for s in shards]
    bcm = ShardedBCM(experts, rank=rank, world=world, device=local, kernel=args.kernel, ard=args.ard)
    bcm.set_loghyper(start_vector(args.hp, bcm.nh, args.kernel, bcm.ard))
    t0 = time.perf_counter()
    trace = bcm.cg_solve(args.budget)
    dt = time.perf_counter() - t0
    if rank == 0:
        print("\n\n PLEASE-SEE %d : %s\n" % (bcm.nh, ", ".join("%f" % v for v in bcm.hp)))
        print("TOTAL training time = %f  (%d evaluations, final -LL %.9g)" % (dt, trace.shape[0], trace[-1, -1]))
    if args.test_rows > 0:
        s0 = dataset.load_chunk("%s0.txt" % args.inputs, "%s0.txt" % args.labels)
        Xt, yt = s0[0][args.rows:args.rows + args.test_rows], s0[1][args.rows:args.rows + args.test_rows]
        m, v = bcm.predict(Xt, combine=args.combine, with_noise=True)
        if rank == 0:
            print("NLPP = %.12g" % Covsum.get_negative_log_predprob(yt, m, v))
    bcm.close()
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
