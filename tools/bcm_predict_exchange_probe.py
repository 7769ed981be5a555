"""Product-of-experts prediction through the library's exchange (cugp_bcm_predict_allgather) against the paths it
replaces, on one GPU, 1000 test points, experts already valid:

  A. world of one, no communicator: cugp_bcm_predict (expert by expert, host sums) vs the new path (batched launches
     per group, the product on the device);
  B. a one-rank NCCL process group: ShardedBCM.predict in the `allreduce` form (torch all_reduce of a [K, 2, nt] array)
     vs the `library` form (the same through a one-rank RCCL communicator inside libcugp).

The variants are interleaved call by call; medians of --reps calls; every result must carry the same bits.

    python tools/bcm_predict_exchange_probe.py [--reps 25] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

SHAPES = ((2, 1500), (16, 1500), (4, 6000))


def same(a, b):
    return bool(np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64)))


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--json", default="")
    ap.add_argument("--no-rccl", action="store_true", help="part A only")
    ap.add_argument("--only", type=int, default=0, help="only the shape with this many experts")
    args = ap.parse_args()
    shapes = [s for s in SHAPES if not args.only or s[0] == args.only]

    import torch
    import torch.distributed as dist
    import cugp_amd.gp as gp
    from cugp_amd.bcm import ShardedBCM
    from conftest import synth

    hp = np.array([np.log(3.0), 0.0, np.log(0.1)])
    Xt = synth(1000, seed=9)[0]
    results = []
    comm = gp.Comm(None, 0, 1, 0)
    for K, rows in shapes:
        X, y = synth(K * rows, seed=5)
        b = gp.BCM.split(X, y, K)
        b.set_BCM_log_hyperparam(hp)
        b.loglik_grad()
        m0, v0 = b.compute_BCM_test_means_and_var(Xt)
        ta, tb, ok = [], [], True
        for _ in range(args.reps):
            t, (m, v) = timed(lambda: b.compute_BCM_test_means_and_var(Xt))
            ta.append(t)
            ok = ok and same(m, m0) and same(v, v0)
            t, (m, v) = timed(lambda: comm.predict_allgather(b, K, K, Xt))
            tb.append(t)
            ok = ok and same(m, m0) and same(v, v0)
        r = {"part": "A", "K": K, "rows": rows, "nt": Xt.shape[0], "reps": args.reps,
             "cugp_bcm_predict_ms": float(np.median(ta)), "allgather_world1_ms": float(np.median(tb)),
             "identical_bits": ok}
        results.append(r)
        print("A  K=%2d x %5d rows: cugp_bcm_predict %.3f ms | predict_allgather (world of one) %.3f ms | bits %s"
              % (K, rows, r["cugp_bcm_predict_ms"], r["allgather_world1_ms"], "identical" if ok else "DIFFER"),
              flush=True)
        b.close()
    comm.close()

    if not args.no_rccl:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29547")
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
        for K, rows in shapes:
            X, y = synth(K * rows, seed=5)
            experts = [(X[rows * k:rows * (k + 1)], y[rows * k:rows * (k + 1)]) for k in range(K)]
            forms = {}
            for form in ("allreduce", "library"):
                os.environ["CUGP_BCM_EXCHANGE"] = form
                s = ShardedBCM(experts, rank=0, world=1, device=0, comm_device=torch.device("cuda", 0))
                s._allreduce = lambda t: (dist.all_reduce(t, op=dist.ReduceOp.SUM), t)[1]   # the collective at 1 rank
                s.set_loghyper(hp)
                s.loglik_grad()
                forms[form] = s
            os.environ.pop("CUGP_BCM_EXCHANGE", None)
            m0, v0 = forms["allreduce"].predict(Xt)
            ta, tb, ok = [], [], True
            for _ in range(args.reps):
                t, (m, v) = timed(lambda: forms["allreduce"].predict(Xt))
                ta.append(t)
                ok = ok and same(m, m0) and same(v, v0) and forms["allreduce"].predict_form == "torch"
                t, (m, v) = timed(lambda: forms["library"].predict(Xt))
                tb.append(t)
                ok = ok and same(m, m0) and same(v, v0) and forms["library"].predict_form == "library"
            r = {"part": "B", "K": K, "rows": rows, "nt": Xt.shape[0], "reps": args.reps,
                 "sharded_allreduce_ms": float(np.median(ta)), "sharded_library_ms": float(np.median(tb)),
                 "identical_bits": ok}
            results.append(r)
            print("B  K=%2d x %5d rows: ShardedBCM.predict allreduce %.3f ms | library %.3f ms | bits %s"
                  % (K, rows, r["sharded_allreduce_ms"], r["sharded_library_ms"], "identical" if ok else "DIFFER"),
                  flush=True)
            for s in forms.values():
                s.close()
        dist.destroy_process_group()

    if args.json:
        with open(args.json, "w") as f:
            json.dump({"results": results}, f, indent=1)
    if not all(r["identical_bits"] for r in results):
        sys.exit(1)


if __name__ == "__main__":
    main()
