"""Builds of libcugp.so against each other on one board, alternating in child processes (a process loads one library):
each child runs with its library copied over cugp_amd/lib/libcugp.so, which is put back at the end.
    tools/lib_bench_ab.py [--rounds 5] name=path name=path ...            the metric: bench.py --gpus 1 --steps 20 --warmup 5
    tools/lib_bench_ab.py --guard [--rounds 5] name=path name=path ...    the regression guard's shapes (GUARD below)
name=path@3=4,15=4 runs that library under CUGP_TUNE="3=4,15=4" (process defaults of tuning keys: one build stands for
the libraries that differ only in a default).
The first library is the base.  Per figure: every library's per-round values and median, the base's own spread over the
rounds (max - min: A against A), and each other library's median against the base's -- "beyond" where |difference|
exceeds that spread.  Stops at the first child that fails: nothing more is started on the board behind it."""
import json
import os
import shutil
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "cugp_amd", "lib", "libcugp.so")
# (experts, rows per expert, log-likelihood only): single handles, expert groups on one GPU, cugp_loglik alone
GUARD = [(1, 4096, False), (1, 1500, False), (2, 1500, False), (16, 1500, False), (8, 3000, False), (4, 6000, False),
         (1, 8192, True)]
EVALS = 12


def tolerate_older_library():
    """A base library from before a call was added: bind only what it exports (as tools/lib_ab.py does)."""
    import ctypes
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    from cugp_amd import capi
    capi._share_torch_hip_runtime()
    have = ctypes.CDLL(capi.LIB_PATH)
    capi.SIGNATURES = {k: v for k, v in capi.SIGNATURES.items() if hasattr(have, k)}


def bench_child(args):
    import runpy
    tolerate_older_library()
    sys.argv = [os.path.join(ROOT, "bench.py")] + args
    runpy.run_path(sys.argv[0], run_name="__main__")


def guard_child():
    tolerate_older_library()
    import numpy as np
    import cugp_amd.gp as gp
    from conftest import synth
    hp = np.array([np.log(3.0), 0.0, np.log(0.1)])
    for K, rows, ll_only in GUARD:
        X, y = synth(K * rows)
        if K == 1:
            g = gp.Covsum(rows, 10)
            g.set_data(X, y)
            run = g.compute_loglikelihood if ll_only else g.loglik_grad
            setter = g.set_loghyperparam
        else:
            g = gp.BCM.split(X, y, K)
            run, setter = g.loglik_grad, g.set_BCM_log_hyperparam
        ts = []
        for it in range(3 + EVALS):
            setter(hp + 1e-4 * it)
            t0 = time.perf_counter()
            run()
            ts.append(1e3 * (time.perf_counter() - t0))
        print("GUARD %dx%d%s %.4f" % (K, rows, "_ll" if ll_only else "", statistics.median(ts[3:])), flush=True)
        g.close()


def run_child(guard, tune):
    if guard:
        cmd = [sys.executable, os.path.abspath(__file__), "--guard-child"]
    else:
        cmd = [sys.executable, os.path.abspath(__file__), "--bench-child", "--gpus", "1", "--steps", "20", "--warmup", "5"]
    env = dict(os.environ)
    env.pop("CUGP_TUNE", None)
    if tune:
        env["CUGP_TUNE"] = tune
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    if r.returncode != 0:
        return None, "exit %d: %s" % (r.returncode, r.stderr.strip()[-400:])
    if guard:
        return {ln.split()[1]: float(ln.split()[2]) for ln in r.stdout.split("\n") if ln.startswith("GUARD ")}, None
    line = json.loads(r.stdout.strip().split("\n")[-1])
    return {"ms_per_step": line["ms_per_step"]}, None


def main(argv):
    guard = "--guard" in argv
    rounds = int(argv[argv.index("--rounds") + 1]) if "--rounds" in argv else 5
    libs = [a.split("=", 1) for a in argv if "=" in a]
    keep = LIB + ".ab_keep"
    shutil.copy2(LIB, keep)
    res = {name: [] for name, _ in libs}
    try:
        for rnd in range(rounds):
            for name, path in libs:
                path, _, tune = path.partition("@")
                shutil.copy2(path, LIB)
                row, err = run_child(guard, tune)
                if row is None:
                    print("%s round %d failed: %s" % (name, rnd, err), flush=True)
                    return 1
                res[name].append(row)
                print("round %d %-10s %s" % (rnd, name, "  ".join("%s %.4f" % kv for kv in row.items())), flush=True)
    finally:
        shutil.move(keep, LIB)
    base = libs[0][0]
    print("# figure | library | per round | median | base's A-against-A spread | median - base's median | verdict")
    for fig in res[base][0]:
        b = [r[fig] for r in res[base]]
        bmed, spread = statistics.median(b), max(b) - min(b)
        for name, _ in libs:
            v = [r[fig] for r in res[name]]
            d = statistics.median(v) - bmed
            print("%s | %s | %s | %.4f | %.4f | %+.4f (%+.2f %%) | %s" % (
                fig, name, " ".join("%.4f" % x for x in v), statistics.median(v), spread, d, 100 * d / bmed,
                "base" if name == base else "beyond the spread" if abs(d) > spread else "inside the spread"), flush=True)
    return 0


if __name__ == "__main__":
    if "--guard-child" in sys.argv:
        guard_child()
    elif "--bench-child" in sys.argv:
        bench_child(sys.argv[sys.argv.index("--bench-child") + 1:])
    else:
        sys.exit(main(sys.argv[1:]))
