"""GPU tests of the ARD kernel (one length scale per input dimension; cugp_create_ard and the _ard calls).

Accuracy is held to fp64 rounding against the extended-precision truth of tests/truth.py (the truth.ARD descriptor),
through the harness of tests/accuracy.py:

    err_gpu(q) <= F_ARD * max(noise(q), floor(q))

with every gradient component relative to the largest of the d + 2 true ones, the yardstick from the CPU oracle on
the scaled copy X / l (every per-dimension component uses the yardstick of their sum) and F_ARD = 32 set from the
CPU stand-in (tests/test_truth_ard_cpu.py, docs/ACCURACY.md) -- never from the GPU.
Every figure is printed before it is asserted ("ACC <case> <quantity> err noise floor ratio"; run with -s).
One process, one device (test 9 starts one fresh child process); nothing outside the tree is read.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import accuracy
import golden_jobs
import truth
from accuracy import Report
from conftest import GOLDEN, ROOT, synth
from cugp_amd import capi

sys.path.insert(0, GOLDEN)
import make_truth  # noqa: E402

pytestmark = pytest.mark.gpu
extended = pytest.mark.skipif(not truth.EXTENDED, reason="numpy.longdouble is not an extended-precision type here")

LD = truth.LD


@pytest.fixture(scope="module")
def gp_mod():
    import cugp_amd.gp as gp
    return gp


def ard(gp_mod, X, y, hp, overlap=None):
    g = gp_mod.Covsum(X.shape[0], X.shape[1], ard=True)
    if overlap is not None:
        g.set_overlap(overlap)
    g.set_data(X, y)
    g.set_loghyperparam(hp)
    return g


# ------------------------------------------------------------------ 1. accuracy
@extended
@pytest.mark.parametrize("name", list(truth.ARD_CASES))
def test_accuracy_live(gp_mod, oracle, name):
    """loglik_grad, the LL-only path, prediction at 64 points, alpha and 64 rows of K^-1 (F_SOLVE), the joint covariance
    with and without noise on the two smallest and two largest cases; n1025_dense also with the inverse streams off."""
    c = accuracy.live(oracle, "ard", name)
    X, y, cov = c["X"], c["y"], c["cov"]

    def fresh(g):
        assert g.get_param_dim() == X.shape[1] + 2
    accuracy.hold_live_case(Report(name, cov), c, lambda overlap=None: ard(gp_mod, X, y, cov.hp, overlap),
                            overlaps=(False, True) if name == "n1025_dense" else (True,),
                            joint=name in truth.JOINT_CASES_ARD, fresh=fresh)


@extended
def test_accuracy_fixture_n2049_d10(gp_mod):
    """17 tiles, ten unequal length scales, against the committed truth (tests/golden/make_truth.py)."""
    X, y, Xt, cov, _ = make_truth.inputs("n2049_d10")
    accuracy.hold_fixture_case(Report("n2049_d10", cov), make_truth.load("n2049_d10"),       # a missing fixture fails, it does not skip
                               X, y, Xt, cov, lambda: ard(gp_mod, X, y, cov.hp))


# ------------------------------------------------------------------ 2. a dropped dimension drops out exactly
def test_dropped_dimension_is_exact(gp_mod):
    """theta_2 = 800: w_2 = exp(-800) = 0.0, and adding 0.0 * 0.0 in index order changes no bit -- K, LL and the other
    components equal those of an ARD handle on the data without column 2 bit for bit, and g_2 == 0.0."""
    X, y = synth(200, d=4, seed=11, scale=3.0)
    keep = [0, 1, 3]
    hp = np.array([0.5, 0.7, 800.0, 0.9, 0.3, -1.0])
    hp3 = hp[[0, 1, 3, 4, 5]]
    g4 = ard(gp_mod, X, y, hp)
    g3 = ard(gp_mod, np.ascontiguousarray(X[:, keep]), y, hp3)
    assert np.array_equal(g4.compute_K_train(), g3.compute_K_train())
    ll4, gr4 = g4.loglik_grad()
    ll3, gr3 = g3.loglik_grad()
    assert ll4 == ll3 and np.array_equal(gr4[[0, 1, 3, 4, 5]], gr3), (ll4, ll3, gr4, gr3)
    assert gr4[2] == 0.0
    g4.close()
    g3.close()


@extended
def test_nearly_dropped_and_overflowing_dimension(gp_mod, oracle):
    """theta_2 = 40 (w_2 = 4e-18): finite, and the 3-column model within the accuracy bound.  theta_2 = -800 (w_2
    overflows): LL is NaN and the call still returns CUGP_OK (the header's convention), no error, fault or hang."""
    X, y = synth(200, d=4, seed=11, scale=3.0)
    Xt = synth(truth.NT, d=4, seed=7, scale=3.0)[0]
    keep = [0, 1, 3]
    hp3 = [0.5, 0.7, 0.9, 0.3, -1.0]
    X3, Xt3 = np.ascontiguousarray(X[:, keep]), np.ascontiguousarray(Xt[:, keep])
    cov = truth.ARD(hp3)
    c = accuracy.case_at(oracle, cov, X3, y, Xt3, truth.Truth(X3, y, cov))
    t, noise, fl = c["t"], c["noise"], c["floor"]
    g = ard(gp_mod, X, y, [0.5, 0.7, 40.0, 0.9, 0.3, -1.0])
    ll, gr = g.loglik_grad()
    m, v = g.compute_test_means_and_variances(X, y, Xt)
    assert np.isfinite(ll) and np.all(np.isfinite(gr)) and np.all(np.isfinite(m)) and np.all(np.isfinite(v))
    rep = Report("theta2=40", cov)
    rep.add_all("", truth.errors(cov, ll, gr[[0, 1, 3, 4, 5]], m, v, t.ll, t.grad, c["tm"], c["tv"]), noise, fl)
    rep.add("g_2", abs(gr[2]) / float(np.max(np.abs(t.grad))), noise["gc"], fl["gc"])
    g.set_loghyperparam([0.5, 0.7, -800.0, 0.9, 0.3, -1.0])
    ll, gr = g.loglik_grad()                                      # raises on any return code but CUGP_OK
    assert np.isnan(ll)
    assert np.isnan(g.compute_loglikelihood())
    g.set_loghyperparam([0.5, 0.7, 0.8, 0.9, 0.3, -1.0])          # and the handle goes on working
    assert np.isfinite(g.loglik_grad()[0])
    g.close()
    rep.check()


# ------------------------------------------------------------------ 3. equal length scales meet the isotropic path
@extended
@pytest.mark.parametrize("name", ["n257_d3", "n515_dense"])
def test_equal_length_scales_meet_the_isotropic_handle(gp_mod, oracle, name):
    """Both handles are within their bounds of the same truth, so they differ by at most (F + F_ARD) yardsticks."""
    c = accuracy.live(oracle, "se", name)
    X, y, Xt, cov, hp = c["X"], c["y"], c["Xt"], c["cov"], c["cov"].hp
    d = X.shape[1]
    gi = gp_mod.Covsum(*X.shape)
    gi.set_loghyperparam(hp)
    lli, gri = gi.loglik_grad(X, y)
    mi, vi = gi.compute_test_means_and_variances(X, y, Xt)
    gi.close()
    ga = ard(gp_mod, X, y, [hp[0]] * d + [hp[1], hp[2]])
    lla, gra = ga.loglik_grad()
    ma, va = ga.compute_test_means_and_variances(X, y, Xt)
    ga.close()
    e = truth.errors(cov, lla, [gra[:d].sum(), gra[d], gra[d + 1]], ma, va, LD(lli), gri.astype(LD), mi.astype(LD), vi.astype(LD))
    rep = Report(name + "_iso", cov)
    rep.add_all("", e, c["noise"], c["floor"], truth.F + truth.F_ARD)
    rep.check()


def test_dense_8192_golden_with_ten_equal_length_scales(gp_mod):
    """The dense 8192-row golden of tests/test_gpu_golden_configs.py through an ARD handle with ten equal theta_c = hp[0]:
    the reference's LL and gradient at that file's tolerances, with the gradient and -- on a fresh handle -- through the
    LL-only path.  The only test of the two-speed schedule and the 8256-block trace under ARD."""
    c = golden_jobs.job("d8192_ll")                                        # a missing fixture fails, it does not skip
    z = np.load(os.path.join(GOLDEN, "data_siproper_9192.npz"))
    X, y = np.ascontiguousarray(z["X"][:8192]), np.ascontiguousarray(z["y"][:8192])
    hp = [c["hp"][0]] * 10 + [c["hp"][1], c["hp"][2]]
    g = ard(gp_mod, X, y, hp)
    ll, gr = g.loglik_grad()
    assert golden_jobs.ll_close(ll, c["ll"]), (ll, c["ll"])
    cg = golden_jobs.job("d8192_grad")
    g3 = [gr[:10].sum(), gr[10], gr[11]]
    assert golden_jobs.grad_close(g3, cg["grad"]), (g3, cg["grad"])
    g.close()
    g = ard(gp_mod, X, y, hp)
    assert golden_jobs.ll_close(g.compute_loglikelihood(), c["ll"])
    g.close()


# ------------------------------------------------------------------ 4. replayed graphs see new length scales
@pytest.mark.parametrize("n", [300, 1025], ids=["graph-300", "launches-1025"])
def test_new_length_scales_reach_the_kernels(gp_mod, n):
    """theta_A, theta_B, theta_A on one handle: the third evaluation equals the first bit for bit, the second a fresh
    handle's at theta_B -- also when only ONE theta_c differs.  300 rows replay a captured graph (the weights travel by
    the copy node at its head), 1025 rows are launched one by one (the same buffer, the argument path)."""
    d = 5
    X, y = synth(n, d=d, seed=n, scale=3.0)
    A = np.array([0.9, 0.5, 1.3, 0.7, 1.1, 0.2, -1.0])
    B1 = np.array([0.6, 1.2, 0.8, 1.0, 0.4, 0.3, -0.7])
    B2 = A.copy()
    B2[3] = 1.05

    def ev(g, hp, grad=True):
        g.set_loghyperparam(hp)
        return g.loglik_grad() if grad else (g.compute_loglikelihood(), np.zeros(0))
    for B in (B1, B2):
        for grad in (True, False):
            g = ard(gp_mod, X, y, A)
            first, second, third = ev(g, A, grad), ev(g, B, grad), ev(g, A, grad)
            g.close()
            f = ard(gp_mod, X, y, B)
            fresh = ev(f, B, grad)
            f.close()
            assert third[0] == first[0] and np.array_equal(third[1], first[1])
            assert second[0] == fresh[0] and np.array_equal(second[1], fresh[1])
            assert second[0] != first[0]


# ------------------------------------------------------------------ 5. reproducibility
def test_ten_evaluations_identical_bits(gp_mod):
    X, y = synth(1300, d=6, seed=5, scale=2.5)
    g = ard(gp_mod, X, y, [0.6, 0.8, 0.9, 1.0, 1.1, 1.3, 0.2, -1.0])
    ll0, gr0 = g.loglik_grad()
    for _ in range(9):
        g.set_data(X, y)                                          # invalidates what the handle holds: a full evaluation
        ll, gr = g.loglik_grad()
        assert ll == ll0 and np.array_equal(gr, gr0)
    g.close()


# ------------------------------------------------------------------ 6. d across the feature-chunk boundary
CHUNK_TOL = 1e-11


@pytest.mark.parametrize("d", [1, 15, 16, 17, 32, 33])
def test_feature_chunks_against_the_standin(gp_mod, d):
    """A wiring test (the accuracy cases hold the rounding): LL and every gradient component against the CPU stand-in
    at 1e-11 relative (gradient: to max|g|).  Stand-in and GPU are each within ~5e-13 of the truth on inputs this
    small, so 1e-11 leaves a factor of ten; the stand-in's own distance from the truth is asserted where the truth
    can be had."""
    n = 130
    X, y = synth(n, d=d, seed=100 + d, scale=2.0)
    hp = np.linspace(0.8, 1.6, d).tolist() + [0.3, -0.8]
    cov = truth.ARD(hp)
    sll, sg, _, _ = truth.standin(cov, X, y, X[:1])
    if truth.EXTENDED:
        t = truth.Truth(X, y, cov, keep=False)
        e = truth.errors_ll_grad(cov, sll, sg, t.ll, t.grad)
        print("d=%d stand-in against the truth: %s" % (d, e))
        assert max(e.values()) <= 1e-13, e
    g = ard(gp_mod, X, y, hp)
    ll, gr = g.loglik_grad()
    K = g.compute_K_train()
    g.close()
    assert np.mean(np.abs(K) > 1e-3) > 0.5                        # far from diagonal
    el, eg = abs(ll - sll) / abs(sll), np.max(np.abs(gr - sg)) / np.max(np.abs(sg))
    print("d=%d: LL %.3e, gradient %.3e (of max|g|)" % (d, el, eg))
    assert el <= CHUNK_TOL and eg <= CHUNK_TOL, (d, el, eg)


# ------------------------------------------------------------------ 7. the optimiser
def test_cg_solve_ard_finds_the_relevant_dimension(gp_mod):
    """y depends on x_0 only.  cg_solve (budget 60) on the ARD handle against cugp_cg_minimize_n driven by the CPU
    stand-in: probe for probe while the objective still moves (5e-5), end point 5e-5 (2e-3 where the run ended on
    the plateau), final objective 1e-7.  Then the point of the feature: the final -LL is lower than the isotropic
    cg_solve's on the same data, and theta_1, theta_2, theta_3 each end above theta_0 + 1."""
    X, y = synth(300, d=4, scale=3.0)
    start = [0.5] * 4 + [0.5, 0.5]

    def fn(th):
        ll, g, _, _ = truth.standin(truth.ARD(th), X, y, X[:1])
        return -ll, g
    th_cpu, tr_cpu = gp_mod.cg_minimize_n(fn, start, 60)
    g = ard(gp_mod, X, y, start)
    tr = g.cg_solve(budget=60)
    th = g.get_loghyperparam()
    f_end = -g.compute_loglikelihood()
    g.close()
    assert tr.shape[1] == 7
    f_cpu = fn(th_cpu)[0]
    n = min(len(tr), len(tr_cpu))
    err = np.abs(tr[:n, :6] - tr_cpu[:n, :6]) / np.maximum(1.0, np.abs(tr_cpu[:n, :6]))
    moving = np.abs(tr_cpu[:n, 6] - f_cpu) > 1e-9 * abs(f_cpu)
    print("ARD cg_solve: %d probes (CPU %d), %d while the objective moves, max rel. deviation there %.2e; end %s f %.10g (CPU %.10g)"
          % (len(tr), len(tr_cpu), moving.sum(), np.max(err[moving]), th, f_end, f_cpu))
    assert moving.sum() >= 20 and np.all(err[moving] <= 5e-5), (int(moving.sum()), float(np.max(err[moving])))
    assert len(tr) == len(tr_cpu) or not moving[-1], (len(tr), len(tr_cpu))
    assert np.allclose(th, th_cpu, atol=5e-5 if moving[-1] else 2e-3), (th, th_cpu)
    assert abs(f_end - f_cpu) <= 1e-7 * abs(f_cpu), (f_end, f_cpu)

    gi = gp_mod.Covsum(300, 4)
    gi.set_loghyperparam([0.5, 0.5, 0.5])
    tri = gi.cg_solve(X, y, budget=60)
    f_iso = -gi.compute_loglikelihood()
    gi.close()
    print("isotropic cg_solve: %d probes, end f %.10g" % (len(tri), f_iso))
    assert f_end < f_iso - 50.0, (f_end, f_iso)
    assert np.all(th[1:4] > th[0] + 1.0), th


# ------------------------------------------------------------------ 8. refusals
def test_refusals(gp_mod):
    L = capi.lib()
    INV = capi.CUGP_ERR_INVALID
    X, y = synth(150, d=3, seed=8, scale=3.0)
    hp = [0.9, 0.5, 1.2, 0.2, -1.0]
    g = ard(gp_mod, X, y, hp)
    want = g.loglik_grad()
    h = g.handle
    v, ll, ne, ng, nh = np.zeros(8), C.c_double(), C.c_int(), C.c_int(), C.c_int()
    p = capi.ptr(v)
    S = np.empty((150, 150))
    assert L.cugp_num_hyper(h, C.byref(nh)) == 0 and nh.value == 5
    for name, call, use in [
            ("cugp_set_loghyper", lambda: L.cugp_set_loghyper(h, p), b"cugp_set_loghyper_ard"),
            ("cugp_get_loghyper", lambda: L.cugp_get_loghyper(h, p), b"cugp_get_loghyper_ard"),
            ("cugp_loglik_grad", lambda: L.cugp_loglik_grad(h, C.byref(ll), p), b"cugp_loglik_grad_ard"),
            ("cugp_grad", lambda: L.cugp_grad(h, p), b"cugp_loglik_grad_ard"),
            ("cugp_loglik_grad_fetch", lambda: L.cugp_loglik_grad_fetch(h, C.byref(ll), p), b"cugp_loglik_grad_fetch_ard"),
            ("cugp_cg_solve", lambda: L.cugp_cg_solve(h, 5, None, 0, C.byref(ne)), b"cugp_cg_solve_ard"),
            ("cugp_cg_solve_sparing", lambda: L.cugp_cg_solve_sparing(h, 5, None, 0, C.byref(ne), C.byref(ng)), b"cugp_cg_solve_ard"),
            ("cugp_rprop_solve", lambda: L.cugp_rprop_solve(h, 5, None, 0, C.byref(ne)), b"cugp_cg_solve_ard"),
            ("cugp_compute_squared_dist", lambda: L.cugp_compute_squared_dist(h, 1.0, capi.ptr(S)), b"cugp_compute_K_train")]:
        assert call() == INV, name
        msg = L.cugp_last_error()
        assert name.encode() in msg and use in msg, (name, msg)
    assert L.cugp_loglik_grad_fetch(h, C.byref(ll), None) == 0 and ll.value == want[0]    # allowed without a gradient
    for bad in (4, 6, 3):
        assert L.cugp_set_loghyper_ard(h, p, bad) == INV and L.cugp_get_loghyper_ard(h, p, bad) == INV
        assert L.cugp_loglik_grad_ard(h, C.byref(ll), p, bad) == INV
        assert L.cugp_loglik_grad_fetch_ard(h, C.byref(ll), p, bad) == INV
    got = g.loglik_grad()
    g.set_data(X, y)
    again = g.loglik_grad()
    assert got[0] == want[0] and np.array_equal(got[1], want[1]) and again[0] == want[0] and np.array_equal(again[1], want[1])
    assert np.array_equal(g.get_loghyperparam(), hp)
    g.close()

    gi = gp_mod.Covsum(150, 3)
    gi.set_loghyperparam([0.9, 0.2, -1.0])
    wi = gi.loglik_grad(X, y)
    hi = gi.handle
    assert L.cugp_num_hyper(hi, C.byref(nh)) == 0 and nh.value == 3
    assert L.cugp_set_loghyper_ard(hi, p, 5) == INV and L.cugp_get_loghyper_ard(hi, p, 5) == INV
    assert L.cugp_loglik_grad_ard(hi, C.byref(ll), p, 5) == INV and L.cugp_loglik_grad_ard(hi, C.byref(ll), p, 3) == INV
    assert L.cugp_loglik_grad_fetch_ard(hi, C.byref(ll), p, 5) == INV
    assert L.cugp_cg_solve_ard(hi, 5, None, 0, C.byref(ne)) == INV
    assert b"isotropic" in L.cugp_last_error()
    gi.set_data(X, y)
    ai = gi.loglik_grad()
    assert ai[0] == wi[0] and np.array_equal(ai[1], wi[1])
    gi.close()


# ------------------------------------------------------------------ 9. no state leaks into isotropic handles
_ISOLATION = r"""
import json, sys
import numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import cugp_amd.gp as gp
from conftest import synth

def iso(n):
    X, y = synth(n, d=5, seed=n, scale=3.0)
    g = gp.Covsum(n, 5)
    g.set_loghyperparam([0.9, 0.2, -1.0])
    ll, gr = g.loglik_grad(X, y)
    m, v = g.compute_test_means_and_variances(X, y, X[:7] * 0.5)
    g.close()
    return [float(ll).hex()] + [float(x).hex() for x in np.concatenate([gr, m, v])]

def run_ard(n, d):
    X, y = synth(n, d=d, seed=n + d, scale=3.0)
    g = gp.Covsum(n, d, ard=True)
    g.set_data(X, y)
    g.set_loghyperparam(np.linspace(0.6, 1.2, d).tolist() + [0.2, -1.0])
    g.loglik_grad()
    g.compute_test_means_and_variances(X, y, X[:7] * 0.5)
    g.compute_loglikelihood()
    g.close()

before = {n: iso(n) for n in (300, 1025)}          # no ARD handle has existed in this process yet
for n, d in ((300, 5), (1025, 5), (200, 17), (1300, 3)):
    run_ard(n, d)
after = {n: iso(n) for n in (300, 1025)}
print("ISOLATION " + json.dumps(dict(before=before, after=after)))
"""


def test_isotropic_bits_do_not_depend_on_ard_handles():
    """An isotropic handle evaluated before any ARD handle exists in the process (a fresh child process), and a new one
    on the same data after ARD handles of the same and of other sizes have run and been destroyed: identical bits (LL,
    gradient, prediction) at 300 rows (graph path) and 1025 rows."""
    script = _ISOLATION % dict(root=ROOT, tests=os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [s for s in r.stdout.splitlines() if s.startswith("ISOLATION ")][-1]
    out = json.loads(line[len("ISOLATION "):])
    assert out["before"] == out["after"]
    assert all(len(v) == 1 + 3 + 14 for v in out["before"].values())
