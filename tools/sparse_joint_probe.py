"""What the sparse model's joint covariance, draws and input gradients cost beside its marginal prediction (one GPU; needs
the built library):

    python tools/sparse_joint_probe.py --json profiles/sparse_joint_probe.json   # N = 1e5; M = 512, 1024, 2048; D = 10; SE and SE-ARD
    python tools/sparse_joint_probe.py --inducing 1024 --points 4096 --once      # for a rocprofv3 --kernel-trace --stats run

Per (family, M, nt), medians of --reps calls on ONE evaluated handle in one process, host clock around the synchronous
call, in ms:
  predict_ms                  cugp_sparse_predict
  joint_ms                    cugp_sparse_predict_cov (mean and the nt x nt covariance, copied to the host)
  draws_ms                    cugp_sparse_predict_sample, 1000 latent draws from given normals
  grad_ms / grad_mean_ms      cugp_sparse_predict_grad with and without dvar
  fd_ms                       what the gradient cost before: 2 d calls of cugp_sparse_predict at shifted points
--once: one call each, nothing timed, and an exact model of n = mpad rows beside it, so that one kernel trace holds
k_sparse_predict_cov and k_predict_cov at the same (ntpad, k): the sparse launch does two products per tile, 2 x the flop.
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
DRAWS = 1000


def median_ms(fn, reps):
    ts = []
    for _ in range(1 + reps):                                # (one warm-up call)
        t0 = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts[1:]))


def model(n, m, d, ard, nts, reps, once=False):
    import cugp_amd.gp as gp
    from conftest import synth
    X, y = synth(n, d, seed=15618)
    s = gp.SparseGP.from_subset(X, y, m, seed=0, chunk_rows=CHUNK, ard=ard)
    hp = [float(np.log(3.0))] * (d if ard else 1) + [0.0, float(np.log(0.1))]
    s.set_loghyperparam(hp)
    s.bound()
    rows = []
    for nt in nts:
        Xt = synth(nt, d, seed=7)[0]
        z = np.random.default_rng(nt).standard_normal((DRAWS, nt))
        if once:
            s.predict_joint(Xt)
            s.sample_posterior(Xt, DRAWS, normals=z)
            s.predict_grad(Xt)
            mpad = (m + 127) // 128 * 128
            g = gp.Covsum(mpad, d, ard=ard)
            g.set_data(X[:mpad], y[:mpad])
            g.set_loghyperparam(hp)
            g.compute_test_joint(None, None, Xt)
            g.close()
            print("once", "ard" if ard else "se", m, nt, s.predict_cov_plan(nt), flush=True)
            continue

        def fd():
            for c in range(d):
                for sign in (1.0, -1.0):
                    Xs = Xt.copy()
                    Xs[:, c] += sign * 1e-5
                    s.predict(Xs)
        r = dict(family="ard" if ard else "se", n=n, m=m, d=d, nt=nt, cov_plan=list(s.predict_cov_plan(nt)),
                 predict_ms=median_ms(lambda: s.predict(Xt), reps), joint_ms=median_ms(lambda: s.predict_joint(Xt), reps),
                 draws_ms=median_ms(lambda: s.sample_posterior(Xt, DRAWS, normals=z), reps),
                 grad_ms=median_ms(lambda: s.predict_grad(Xt), reps),
                 grad_mean_ms=median_ms(lambda: s.predict_grad(Xt, want_var_grad=False), reps), fd_ms=median_ms(fd, reps))
        r["fd_over_grad"] = r["fd_ms"] / r["grad_ms"]
        rows.append(r)
        print(json.dumps(r), flush=True)
    s.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=100000)
    ap.add_argument("--inducing", type=int, nargs="+", default=[512, 1024, 2048])
    ap.add_argument("--points", type=int, nargs="+", default=[1000, 4096])
    ap.add_argument("--dims", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--once", action="store_true", help="one call each and an exact model of mpad rows beside it, nothing timed")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    rows = []
    for ard in (False,) if args.once else (False, True):
        for m in args.inducing:
            rows += model(args.size, m, args.dims, ard, args.points, args.reps, args.once)
    if args.json and rows:
        from cugp_amd import capi
        doc = dict(build_id=(capi.lib().cugp_build_id() or b"unknown").decode(), reps=args.reps, chunk_rows=CHUNK, draws=DRAWS,
                   rows=rows)
        with open(args.json, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
