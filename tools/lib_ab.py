"""Two builds of libcugp.so on the same board, alternating A, B, A, B in child processes (a process can load only one of
them):
    tools/lib_ab.py <lib A> <lib B> [n ...]            stand-alone LA timings (cugp_bench_la ops 0 = Cholesky, 3 =
                                                       factorisation + inverse as an evaluation runs them)
    tools/lib_ab.py --families <lib A> <lib B> [rounds]   per covariance family (SE, Matern 3/2, 5/2 x isotropic, ARD) at
        4096 rows, d = 10: one gradient evaluation, one 3-target gradient evaluation and one 256-point predict_grad, each
        the median of REPS calls in ms (host clock around the synchronous API call; every call dispatches the family's
        k_trace / k_trace_targets / k_predict_grad once).  After the rounds: per figure the spread of A's own medians
        (A against A) and the largest |B - A| -- a changed kernel passes where the second lies inside the first.
    tools/lib_ab.py --sparse <lib A> <lib B> [rounds]     the sparse model at N = 100000, M = 1024, d = 10 (SE): bound,
        bound_grad, bound_grad_z and a 1000-point predict for the handle's own y, and bound_grad_targets with p = 3, each
        the median of REPS calls in ms at a fresh hyper-parameter vector; the same table and criterion."""
import ctypes as C
import os
import subprocess
import sys
import time

FAMILIES = [("se", False), ("matern32", False), ("matern52", False), ("se", True), ("matern32", True), ("matern52", True)]
REPS = 9


def child_setup(lib):
    """The package bound to `lib` -> (numpy, cugp_amd.gp, conftest.synth, median_ms)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "tests")]
    import numpy as np
    from cugp_amd import capi
    capi.LIB_PATH = os.path.abspath(lib)                 # (as tools/ard_bcm_bits.py --lib)
    capi._share_torch_hip_runtime()
    other = C.CDLL(capi.LIB_PATH)
    capi.SIGNATURES = {k: v for k, v in capi.SIGNATURES.items() if hasattr(other, k)}
    import cugp_amd.gp as gp
    from conftest import synth

    def median_ms(fn):
        ts = []
        for i in range(2 + REPS):                        # (two warm-up calls)
            t0 = time.perf_counter()
            fn(i)
            ts.append(1e3 * (time.perf_counter() - t0))
        return sorted(ts[2:])[REPS // 2]
    return np, gp, synth, median_ms


def families_child(lib):
    np, gp, synth, median_ms = child_setup(lib)
    n, d, nt, m = 4096, 10, 256, 3
    X, y = synth(n, d, seed=15618)
    Xt = np.ascontiguousarray(X[:nt] * 0.5)
    Y = np.ascontiguousarray(np.column_stack([y, np.cos(X[:, 1]), 0.3 * X[:, 2]]))

    for kind, ard in FAMILIES:
        kw = dict(kernel=kind + "_ard") if ard and kind != "se" else dict(kernel=kind, ard=ard)
        g = gp.Covsum(n, d, 0, **kw)
        g.set_data(X, y)

        def hyper(i):
            g.set_loghyperparam([float(np.log(3.0)) + 1e-3 * i] * (d if ard else 1) + [0.0, float(np.log(0.1))])

        def grad(i):
            hyper(i)
            g.loglik_grad()

        def targets(i):
            hyper(i)
            g.loglik_grad_targets()

        t_grad = median_ms(grad)
        t_pg = median_ms(lambda i: g.predict_grad(Xt))
        g.set_targets(Y)
        t_tg = median_ms(targets)
        g.close()
        print("%s%s grad %.3f targets %.3f predict_grad %.3f" % (kind, "_ard" if ard else "", t_grad, t_tg, t_pg), flush=True)


def sparse_child(lib):
    np, gp, synth, median_ms = child_setup(lib)
    n, m, d, nt = 100000, 1024, 10, 1000
    X, y = synth(n, d, seed=15618)
    Xt = np.ascontiguousarray(X[:nt] * 0.5)
    Y = np.ascontiguousarray(np.column_stack([y, np.cos(X[:, 1]), 0.3 * X[:, 2]]))
    s = gp.SparseGP.from_subset(X, y, m, seed=1)

    def fresh(call):
        def fn(i):
            s.set_loghyperparam([float(np.log(3.0)) + 1e-3 * i, 0.0, float(np.log(0.1))])
            call()
        return fn
    row = [("bound", median_ms(fresh(s.bound))), ("bound_grad", median_ms(fresh(s.bound_grad))),
           ("bound_grad_z", median_ms(fresh(s.bound_grad_z)))]
    s.bound()
    row.append(("predict", median_ms(lambda i: s.predict(Xt))))
    s.set_targets(Y)
    row.append(("bound_grad_targets", median_ms(fresh(s.bound_grad_targets))))
    s.close()
    print("sparse " + " ".join("%s %.3f" % kv for kv in row), flush=True)


def rounds_table(mode, lib_a, lib_b, rounds):
    res = {"A": [], "B": []}                              # per round: {figure: ms}
    for rnd in range(rounds):
        for which, lib in (("A", lib_a), ("B", lib_b)):
            r = subprocess.run([sys.executable, __file__, mode + "-child", lib], capture_output=True, text=True,
                               timeout=300)
            if r.returncode != 0:                         # nothing more is started on the board behind a failed child
                print("%s round %d failed (%d): %s" % (which, rnd, r.returncode, r.stderr.strip()[-400:]), flush=True)
                return 1
            row = {}
            for ln in r.stdout.strip().split("\n"):
                w = ln.split()
                print("%s round %d  %s" % (which, rnd, ln), flush=True)
                row.update({"%s %s" % (w[0], w[i]): float(w[i + 1]) for i in range(1, len(w), 2)})
            res[which].append(row)
    print("# figure | A medians | B medians | A-against-A spread | max |B - A's mean| | inside")
    for k in res["A"][0]:
        a, b = [r[k] for r in res["A"]], [r[k] for r in res["B"]]
        spread, diff = max(a) - min(a), max(abs(v - sum(a) / len(a)) for v in b)
        print("%s | %s | %s | %.3f | %.3f | %s" % (k, " ".join("%.3f" % v for v in a), " ".join("%.3f" % v for v in b),
                                                 spread, diff, "yes" if diff <= spread else "NO"), flush=True)
    return 0


if sys.argv[1] == "--families-child":
    families_child(sys.argv[2])
elif sys.argv[1] == "--sparse-child":
    sparse_child(sys.argv[2])
elif sys.argv[1] in ("--families", "--sparse"):
    sys.exit(rounds_table(sys.argv[1], sys.argv[2], sys.argv[3], int(sys.argv[4]) if len(sys.argv) > 4 else 3))
elif sys.argv[1] == "--child":
    L = C.CDLL(sys.argv[2])
    L.cugp_bench_la.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]
    out = []
    for n in [int(v) for v in sys.argv[3:]]:
        for op in (0, 3):
            ms = C.c_double()
            rc = L.cugp_bench_la(op, n, 0, 5, C.byref(ms))
            out.append("n=%d op%d %.3f ms%s" % (n, op, ms.value, "" if rc == 0 else " rc=%d" % rc))
    print("  ".join(out), flush=True)
else:
    sizes = sys.argv[3:] or ["1536", "4096", "8192"]
    for rnd in range(2):
        for lib in sys.argv[1:3]:
            r = subprocess.run([sys.executable, __file__, "--child", lib] + sizes, capture_output=True, text=True)
            print("%-28s %s" % (lib.split("/")[-1], r.stdout.strip() or r.stderr.strip()[-300:]), flush=True)
