"""Results of every covariance pass, as hex, for a comparison of two library builds in fresh processes (a change that
must not move a bit: the ARD product of experts first, then the merge of the per-family kernel bodies):

    python tools/ard_bcm_bits.py [--lib other/libcugp.so] > bits.txt        (once per build)
    python tools/ard_bcm_bits.py --compare parent.txt build.txt             (label | parent | this build | equal)

  - a single ARD handle at N = 1500 (captured graph) and at N = 4096 (launch by launch), D = 10: LL, the gradient, a
    64-point prediction;
  - a squared-exponential and a Matern-5/2 BCM of 2 x 1500 rows: LL, the gradient, the prediction;
  - every kind in {SE, Matern 3/2, Matern 5/2} x {isotropic, ARD} at n = 130 (three 64-row tiles: an off-diagonal one and
    a diagonal one holding two data rows), d = 17 (two feature chunks, the second of one feature) and 70 test points (two
    test tiles): a single handle's LL and gradient launch by launch and as a captured graph (key 5), isotropic with the
    fused and the separate final sums (key 12); a 3-target evaluation; a prediction with joint covariance; the
    test-input gradients of mean and variance; a 2-expert grouped model's LL, gradient and prediction.
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


def family_cases(gp, synth):
    """Every instantiation of the covariance passes (build, cross, joint-covariance epilogue, trace, trace-targets,
    predict-grad) at the smallest shapes that cross a tile and a feature-chunk boundary."""
    GRAPHS, FINALIZE_FUSE_MAX = 5, 12                    # kernels.h TUNE_*
    n, d, nt, m = 130, 17, 70, 3
    X2, y2 = synth(2 * n, d, seed=4711, scale=3.0)
    X, y = X2[:n], y2[:n]
    rng = np.random.default_rng(4712)
    Xt = np.ascontiguousarray(0.5 * X[:nt] + 0.3 * rng.standard_normal((nt, d)))
    Y = np.ascontiguousarray(np.column_stack([y, np.cos(X[:, 1]) + 0.1 * rng.standard_normal(n), X[:, 2] * 0.3]))
    assert Y.shape == (n, m)
    for kind in ("se", "matern32", "matern52"):
        for ard in (False, True):
            tag = "%s%s n=%d" % (kind, " ard" if ard else "", n)
            kw = dict(kernel=kind + "_ard") if ard and kind != "se" else dict(kernel=kind, ard=ard)

            def hyper(i):
                ell = np.log(4.0) + (np.linspace(-0.3, 0.3, d) if ard else np.zeros(1)) + 0.01 * i
                return ell.tolist() + [0.1, float(np.log(0.2))]

            g = gp.Covsum(n, d, 0, **kw)
            g.set_data(X, y)
            for graphs in (0, 1):
                for fuse in ((None,) if ard else (0, 1 << 30)):
                    g.set_tuning(GRAPHS, graphs)
                    if fuse is not None:
                        g.set_tuning(FINALIZE_FUSE_MAX, fuse)
                    for i in range(2):                   # (graphs = 1: the second evaluation replays the captured graph)
                        g.set_loghyperparam(hyper(i))
                        ll, gr = g.loglik_grad()
                        cfg = "graphs=%d fuse=%s @%d" % (graphs, "-" if fuse is None else min(fuse, 1), i)
                        show("%s ll %s" % (tag, cfg), ll)
                        show("%s grad %s" % (tag, cfg), gr)
            g.set_targets(Y)
            ll, gr, each = g.loglik_grad_targets()
            show("%s targets ll" % tag, ll)
            show("%s targets grad" % tag, gr)
            show("%s targets each" % tag, each)
            tm, tv = g.predict_targets(Xt)
            show("%s targets mean" % tag, tm.ravel())
            mean, cov = g.compute_test_joint(X, y, Xt)
            show("%s joint mean" % tag, mean)
            show("%s joint cov" % tag, cov.ravel())
            for with_var in (True, False):
                pm, pv, dm, dv = g.predict_grad(Xt, want_var_grad=with_var)
                show("%s predict_grad mean var=%d" % (tag, with_var), pm)
                show("%s predict_grad variance var=%d" % (tag, with_var), pv)
                show("%s predict_grad dmean var=%d" % (tag, with_var), dm.ravel())
                if with_var:
                    show("%s predict_grad dvar" % tag, dv.ravel())
            g.close()
            b = gp.BCM.split(X2, y2, 2, **kw)
            for i in range(2):
                b.set_BCM_log_hyperparam(hyper(i))
                ll, gr, per = b.loglik_grad()
                bm, bv = b.compute_BCM_test_means_and_var(Xt)
                show("%s bcm 2x%d ll@%d" % (tag, n, i), ll)
                show("%s bcm 2x%d grad@%d" % (tag, n, i), gr)
                show("%s bcm 2x%d per-expert ll@%d" % (tag, n, i), per)
                show("%s bcm 2x%d mean@%d" % (tag, n, i), bm)
                show("%s bcm 2x%d var@%d" % (tag, n, i), bv)
            b.close()


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
    family_cases(gp, synth)
    return 0


if __name__ == "__main__":
    sys.exit(main())
