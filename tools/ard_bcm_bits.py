"""Results of the paths the ARD product of experts must not change, as hex, for a comparison of two library builds in
fresh processes:

    python tools/ard_bcm_bits.py [--lib other/libcugp.so] > bits.txt        (once per build)
    python tools/ard_bcm_bits.py --compare parent.txt build.txt             (label | parent | this build | equal)

  - a single ARD handle at N = 1500 (captured graph) and at N = 4096 (launch by launch), D = 10: LL, the gradient, a
    64-point prediction;
  - a squared-exponential and a Matern-5/2 BCM of 2 x 1500 rows: LL, the gradient, the prediction.
Doubles as C99 hex; arrays longer than 12 as the first 24 hex digits of sha256 over their bytes.
"""
import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402


def show(label, a):
    a = np.atleast_1d(np.asarray(a, dtype=np.float64))
    txt = " ".join(float(x).hex() for x in a) if a.size <= 12 else "sha %s n=%d" % (hashlib.sha256(a.tobytes()).hexdigest()[:24], a.size)
    print("%s | %s" % (label, txt))


def compare(pa, pb):
    A = [ln.rstrip("\n").split(" | ") for ln in open(pa) if " | " in ln]
    B = dict(ln.rstrip("\n").split(" | ") for ln in open(pb) if " | " in ln)
    print("# label | parent | this build | equal")
    bad = 0
    for label, va in A:
        vb = B.get(label, "(missing)")
        bad += va != vb
        print("%s | %s | %s | %s" % (label, va, vb, "yes" if va == vb else "NO"))
    print("# %d values, %d differ" % (len(A), bad))
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default="")
    ap.add_argument("--compare", nargs=2)
    args = ap.parse_args()
    if args.compare:
        return compare(*args.compare)
    from cugp_amd import capi
    if args.lib:
        import ctypes
        capi.LIB_PATH = os.path.abspath(args.lib)
        capi._share_torch_hip_runtime()
        other = ctypes.CDLL(capi.LIB_PATH)
        capi.SIGNATURES = {k: v for k, v in capi.SIGNATURES.items() if hasattr(other, k)}
    import cugp_amd.gp as gp
    from conftest import synth
    d = 10
    for n in (1500, 4096):
        X, y = synth(n, d, seed=15618)
        Xt = np.ascontiguousarray(X[:64] * 0.5)
        g = gp.Covsum(n, d, 0, ard=True)
        g.set_data(X, y)
        for i in range(2):                              # the second evaluation replays the captured graph at N = 1500
            g.set_loghyperparam((np.log(3.0) + np.linspace(-0.2, 0.2, d) + 0.01 * i).tolist() + [0.0, float(np.log(0.1))])
            ll, gr = g.loglik_grad()
            m, v = g.compute_test_means_and_variances(X, y, Xt)
            show("ard n=%d ll@%d" % (n, i), ll)
            show("ard n=%d grad@%d" % (n, i), gr)
            show("ard n=%d mean@%d" % (n, i), m)
            show("ard n=%d var@%d" % (n, i), v)
        g.close()
    X, y = synth(3000, d, seed=15618)
    Xt = np.ascontiguousarray(X[:64] * 0.5)
    for kernel in ("se", "matern52"):
        b = gp.BCM.split(X, y, 2, kernel=kernel)
        for i in range(2):
            b.set_BCM_log_hyperparam([float(np.log(3.0)) + 0.01 * i, 0.0, float(np.log(0.1))])
            ll, gr, per = b.loglik_grad()
            m, v = b.compute_BCM_test_means_and_var(Xt)
            show("%s bcm 2x1500 ll@%d" % (kernel, i), ll)
            show("%s bcm 2x1500 grad@%d" % (kernel, i), gr)
            show("%s bcm 2x1500 per-expert ll@%d" % (kernel, i), per)
            show("%s bcm 2x1500 rows@%d" % (kernel, i), b.loglik_grad_rows().ravel())
            show("%s bcm 2x1500 mean@%d" % (kernel, i), m)
            show("%s bcm 2x1500 var@%d" % (kernel, i), v)
        b.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
