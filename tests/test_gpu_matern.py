"""GPU tests of the Matern 3/2 and 5/2 kernels (cugp_create_kernel, Covsum(kernel=), BCM(kernel=)).

Accuracy is held to fp64 rounding against the extended-precision truth of tests/truth.py (the truth.Matern descriptor),
through the harness of tests/accuracy.py:

    err_gpu(q) <= F_MATERN * max(noise(q), floor(q))

with the yardstick from the CPU oracle's linear algebra on the fp64 Matern K
(data as given and seven permutations) and F_MATERN = 16 set from the CPU stand-in (tests/test_truth_matern_cpu.py,
docs/ACCURACY.md) -- never from the GPU.  K and k_test entries are held to the rounding count of
truth_matern.k_entry_bound.  Every figure is printed before it is asserted ("ACC <case> <quantity> err noise floor
ratio"; run with -s).  One process, one device (the isolation test starts one fresh child process); nothing outside
the tree is read.
"""
import ctypes as C
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import accuracy
import truth
import truth_matern as tm
from accuracy import Report
from conftest import GOLDEN, ROOT, synth
from cugp_amd import capi

sys.path.insert(0, GOLDEN)
import make_truth  # noqa: E402

pytestmark = pytest.mark.gpu
extended = pytest.mark.skipif(not truth.EXTENDED, reason="numpy.longdouble is not an extended-precision type here")

LD = truth.LD
KINDS = [pytest.param(k, id=tm.KIND_NAMES[k]) for k in tm.KINDS]
TUNE_GRAPHS, TUNE_FINALIZE_FUSE_MAX = 5, 12                      # kernels.h TUNE_*
HP = [0.9, 0.2, -1.0]


@pytest.fixture(scope="module")
def gp_mod():
    import cugp_amd.gp as gp
    return gp


def handle(gp_mod, X, y, hp, kind, overlap=None, tuning=None):
    g = gp_mod.Covsum(X.shape[0], X.shape[1], kernel=kind)
    if overlap is not None:
        g.set_overlap(overlap)
    for k, v in (tuning or {}).items():
        g.set_tuning(k, v)
    g.set_data(X, y)
    g.set_loghyperparam(hp)
    return g


def same_bits(a, b):
    """Bit-equal; a NaN on both sides counts as equal (its payload is not part of any contract)."""
    a, b = [np.concatenate([np.atleast_1d(np.asarray(x, dtype=np.float64)).ravel() for x in v]) for v in (a, b)]
    return a.shape == b.shape and bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


# ------------------------------------------------------------------ 1. accuracy
@extended
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(truth.MATERN_CASES))
def test_accuracy_live(gp_mod, oracle, name, kind):
    """loglik_grad, the LL-only path, prediction at 64 points, alpha and 64 rows of K^-1 (F_SOLVE); n1025_dense also
    with the inverse streams off."""
    c = accuracy.live(oracle, tm.KIND_NAMES[kind], name)
    X, y, cov = c["X"], c["y"], c["cov"]

    def fresh(g):
        assert g.kernel == tm.KIND_NAMES[kind]
    accuracy.hold_live_case(Report("%s/%s" % (name, tm.KIND_NAMES[kind]), cov), c,
                            lambda overlap=None: handle(gp_mod, X, y, cov.hp, kind, overlap),
                            overlaps=(False, True) if name == "n1025_dense" else (True,), fresh=fresh)


@extended
def test_accuracy_fixture_n2049_m52(gp_mod):
    """17 tiles, nu = 5/2, against the committed truth (tests/golden/make_truth.py)."""
    X, y, Xt, cov, _ = make_truth.inputs("n2049_m52")
    accuracy.hold_fixture_case(Report("n2049_m52", cov), make_truth.load("n2049_m52"),       # a missing fixture fails, it does not skip
                               X, y, Xt, cov, lambda: handle(gp_mod, X, y, cov.hp, cov.kind))


# ------------------------------------------------------------------ 2. K and k_test
@extended
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["n65", "n300_d17", "n515_d33", "n515_dense", "n1300_d6"])
def test_K_and_k_test_entries(gp_mod, name, kind):
    """cugp_compute_K_train and cugp_compute_k_test entry by entry against the truth, inside the derived K-entry bound
    (truth_matern.k_entry_bound; relative to the true entry); K exactly symmetric, its diagonal bit-equal to
    sf2 + sn2 as fp64 forms it."""
    X, y, Xt, hp = truth.live_inputs(name)
    n, d = X.shape
    l2, sf2, sn2 = truth.hyper(hp)
    g = handle(gp_mod, X, y, hp, kind)
    K = g.compute_K_train()
    Ks = g.compute_k_test(Xt)
    g.close()
    assert np.array_equal(K, K.T)
    assert np.all(np.diag(K) == math.exp(hp[1] * 2) + math.exp(hp[2] * 2))       # the host's exp(2 theta), as scalars() forms them
    off = ~np.eye(n, dtype=bool)
    worst = {}
    for tag, got, A, mask in (("K", K, X, off), ("k_test", Ks, Xt, np.ones(Ks.shape, dtype=bool))):
        true = truth.matern_kernel(truth.sqdist(A, X) / l2, sf2, kind)[0]
        bound = tm.k_entry_bound(tm.a_of(A, X, hp, kind), d, kind)
        rel = (np.abs(got.astype(LD) - true) / true)[mask]
        worst[tag] = float(np.max(rel / bound[mask]))
        print("ACC %s/%s %s: largest |entry - truth| / bound %.3f" % (name, tm.KIND_NAMES[kind], tag, worst[tag]))
    assert worst["K"] <= 1.0 and worst["k_test"] <= 1.0, worst


# ------------------------------------------------------------------ 3. kind 0 is the existing handle
def everything(g, X, y, Xt):
    ll, gr = g.loglik_grad()
    m, v = g.compute_test_means_and_variances(X, y, Xt)
    mj, cov = g.compute_test_joint(X, y, Xt, with_noise=True)
    g.set_data(X, y)
    return [ll, gr, m, v, mj, cov, g.compute_loglikelihood()]


@pytest.mark.parametrize("graphs", [1, 0], ids=["graph", "launches"])
@pytest.mark.parametrize("n", [300, 1025])
def test_kind_zero_is_cugp_create(gp_mod, n, graphs):
    """Kind 0 through cugp_create_kernel against cugp_create: LL, gradient, prediction and joint covariance bit for bit,
    replaying a captured graph (tuning key 5 = 1; 300 rows) and launch by launch (key 5 = 0)."""
    X, y = synth(n, d=5, seed=n, scale=3.0)
    Xt = synth(40, d=5, seed=7, scale=3.0)[0]
    L = capi.lib()
    ref = gp_mod.Covsum(n, 5)
    h = C.c_void_p()
    capi.check(L.cugp_create_kernel(n, 5, 0, 0, capi.CUGP_KERNEL_SE, C.byref(h)))
    new = gp_mod.Covsum.__new__(gp_mod.Covsum)
    new.n, new.d, new.device, new.ard, new.nh, new._kind, new._h, new._data_key = n, 5, 0, False, 3, 0, h, None
    assert new.kernel == "se" and ref.kernel == "se"
    out = []
    for g in (ref, new):
        g.set_tuning(TUNE_GRAPHS, graphs)
        g.set_data(X, y)
        g.set_loghyperparam(HP)
        out.append(everything(g, X, y, Xt))
        g.close()
    assert same_bits(out[0], out[1])


_ISOLATION = r"""
import json, sys
import numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import cugp_amd.gp as gp
from conftest import synth

def se(n):
    X, y = synth(n, d=5, seed=n, scale=3.0)
    g = gp.Covsum(n, 5)
    g.set_loghyperparam([0.9, 0.2, -1.0])
    ll, gr = g.loglik_grad(X, y)
    m, v = g.compute_test_means_and_variances(X, y, X[:7] * 0.5)
    g.close()
    return [float(ll).hex()] + [float(x).hex() for x in np.concatenate([gr, m, v])]

def run_matern(n, d, kernel):
    X, y = synth(n, d=d, seed=n + d, scale=3.0)
    g = gp.Covsum(n, d, kernel=kernel)
    g.set_data(X, y)
    g.set_loghyperparam([0.9, 0.2, -1.0])
    g.loglik_grad()
    g.compute_test_means_and_variances(X, y, X[:7] * 0.5)
    g.compute_test_joint(X, y, X[:7] * 0.5)
    g.compute_loglikelihood()
    g.close()

before = {n: se(n) for n in (300, 1025)}          # no Matern handle has existed in this process yet
for n, d in ((300, 5), (1025, 5), (200, 17), (1300, 3)):
    for kernel in ("matern32", "matern52"):
        run_matern(n, d, kernel)
after = {n: se(n) for n in (300, 1025)}
print("ISOLATION " + json.dumps(dict(before=before, after=after)))
"""


def test_se_bits_do_not_depend_on_matern_handles():
    """An SE handle evaluated before any Matern handle exists in the process (a fresh child process), and a new one on
    the same data after Matern handles of the same and of other sizes have run and been destroyed: identical bits (LL,
    gradient, prediction) at 300 rows (graph path) and 1025 rows."""
    script = _ISOLATION % dict(root=ROOT, tests=os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [s for s in r.stdout.splitlines() if s.startswith("ISOLATION ")][-1]
    out = json.loads(line[len("ISOLATION "):])
    assert out["before"] == out["after"]
    assert all(len(v) == 1 + 3 + 14 for v in out["before"].values())


# ------------------------------------------------------------------ 4. extremes, beside an SE handle on the same data
@pytest.mark.parametrize("kind", KINDS)
def test_extreme_length_scales(gp_mod, kind):
    """theta_0 = 400 (l^2 = inf, s = 0 everywhere): K, LL, g1, g2 bit-equal to SE's, g0 == 0.  theta_0 = -400 (l^2 = 0,
    s = +inf off the diagonal): the off-diagonal of K is exactly 0 with no NaN, LL has SE's bits, g0 == 0 wherever SE's
    is.  (On the diagonal s = 0 / 0 for every kind, SE included: K_ii is NaN for both and LL with it -- the header's
    convention for a covariance that cannot be factored; a NaN on both sides counts as equal bits.)  theta_0 = -5 and
    -7, where exp(-a) underflows for most and for nearly all pairs: finite results, exactly 0 where a > 750 and a
    positive (possibly denormal) entry where a < 740."""
    n, d = 200, 4
    X, y = synth(n, d=d, seed=11, scale=3.0)
    off = ~np.eye(n, dtype=bool)
    for th0 in (400.0, -400.0):
        hp = [th0, 0.3, -0.8]
        gs, gm = handle(gp_mod, X, y, hp, "se"), handle(gp_mod, X, y, hp, kind)
        Ks, Km = gs.compute_K_train(), gm.compute_K_train()
        lls, grs = gs.loglik_grad()
        llm, grm = gm.loglik_grad()
        gs.close()
        gm.close()
        print("theta0 %g kind %d: LL %r (SE %r) g %s (SE %s)" % (th0, kind, llm, lls, grm, grs))
        assert same_bits([llm], [lls])
        if th0 > 0:
            assert np.array_equal(Km, Ks) and np.all(Km[off] == np.exp(2 * hp[1]))
            assert np.isfinite(llm) and same_bits([grm[1], grm[2]], [grs[1], grs[2]])
            assert grm[0] == 0.0 and grs[0] == 0.0
        else:
            assert np.all(Km[off] == 0.0) and not np.any(np.isnan(Km[off]))
            assert same_bits(np.diag(Km), np.diag(Ks))
            assert same_bits([grm[0]], [grs[0]]) and (grm[0] == 0.0 or np.isnan(grs[0]))
    for th0 in (-5.0, -7.0):
        g = handle(gp_mod, X, y, [th0, 0.3, -0.8], kind)
        K = g.compute_K_train()
        ll, gr = g.loglik_grad()
        m, v = g.compute_test_means_and_variances(X, y, X[:9] + 1e-3)
        g.close()
        print("theta0 %g kind %d: LL %r g %s, %d of %d off-diagonal entries are 0" % (th0, kind, ll, gr, int(np.sum(K[off] == 0)), off.sum()))
        assert np.all(np.isfinite(K)) and np.isfinite(ll) and np.all(np.isfinite(gr))
        assert np.all(np.isfinite(m)) and np.all(np.isfinite(v))
        a = tm.a_of(X, X, [th0, 0.3, -0.8], kind)                  # exp(-a) underflows to 0 just above a = 745.13
        assert np.sum(K[off] == 0) > 0 and np.all(K[a > 750] == 0.0) and np.all(K[off & (a < 740)] > 0.0)


# ------------------------------------------------------------------ 5. new hyper-parameters, repeatability
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [300, 1025], ids=["graph-300", "launches-1025"])
def test_new_hyperparameters_reach_the_kernels(gp_mod, n, kind):
    """theta_A, theta_B, theta_A on one handle: the third evaluation equals the first bit for bit, the second a fresh
    handle's at theta_B -- also when only theta_0 differs.  300 rows replay a captured graph (the hyper-scalars travel
    by the copy node at its head), and again launch by launch (tuning key 5 = 0); 1025 rows are launched one by one."""
    X, y = synth(n, d=5, seed=n, scale=3.0)
    A = np.array(HP)
    B1 = np.array([0.6, 0.3, -0.7])
    B2 = A.copy()
    B2[0] = 1.05

    def ev(g, hp, grad=True):
        g.set_loghyperparam(hp)
        return g.loglik_grad() if grad else (g.compute_loglikelihood(), np.zeros(0))
    for tuning in ({}, {TUNE_GRAPHS: 0}) if n == 300 else ({},):
        for B in (B1, B2):
            for grad in (True, False):
                g = handle(gp_mod, X, y, A, kind, tuning=tuning)
                first, second, third = ev(g, A, grad), ev(g, B, grad), ev(g, A, grad)
                g.close()
                f = handle(gp_mod, X, y, B, kind, tuning=tuning)
                fresh = ev(f, B, grad)
                f.close()
                assert third[0] == first[0] and np.array_equal(third[1], first[1])
                assert second[0] == fresh[0] and np.array_equal(second[1], fresh[1])
                assert second[0] != first[0]


@pytest.mark.parametrize("kind", KINDS)
def test_ten_evaluations_identical_bits(gp_mod, kind):
    X, y = synth(1300, d=6, seed=5, scale=2.5)
    g = handle(gp_mod, X, y, HP, kind)
    ll0, gr0 = g.loglik_grad()
    for _ in range(9):
        g.set_data(X, y)                                          # invalidates what the handle holds: a full evaluation
        ll, gr = g.loglik_grad()
        assert ll == ll0 and np.array_equal(gr, gr0)
    g.close()


# ------------------------------------------------------------------ 6. feature chunks, fused final sums
CHUNK_TOL = 1e-11


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("d", [1, 15, 16, 17, 32, 33])
def test_feature_chunks_against_the_standin(gp_mod, d, kind):
    """A wiring test (the accuracy cases hold the rounding): LL and every gradient component against the CPU stand-in
    at 1e-11 relative (gradient: to max|g|).  Stand-in and GPU are each within ~5e-13 of the truth on inputs this
    small, so 1e-11 leaves a factor of ten; the stand-in's own distance from the truth is asserted where the truth
    can be had.  Tuning key 12 = 0 (k_finalize as its own launch) and its default (the last block of the trace takes
    the final sums): identical bits."""
    n = 130
    X, y = synth(n, d=d, seed=100 + d, scale=2.0)
    hp = [0.5 * np.log(d) + 1.2, 0.3, -0.8]
    cov = truth.Matern(hp, kind)
    sll, sg, _, _ = truth.standin(cov, X, y, X[:1])
    if truth.EXTENDED:
        t = truth.Truth(X, y, cov, keep=False)
        e = truth.errors_ll_grad(cov, sll, sg, t.ll, t.grad)
        print("d=%d stand-in against the truth: %s" % (d, e))
        assert max(e.values()) <= 1e-13, e
    g = handle(gp_mod, X, y, hp, kind)
    assert g.get_tuning(TUNE_FINALIZE_FUSE_MAX) > 3              # 130 rows: 6 trace blocks, fused by default
    ll, gr = g.loglik_grad()
    K = g.compute_K_train()
    g.close()
    g = handle(gp_mod, X, y, hp, kind, tuning={TUNE_FINALIZE_FUSE_MAX: 0})
    ll2, gr2 = g.loglik_grad()
    g.close()
    assert same_bits([ll, gr], [ll2, gr2])
    assert np.mean(np.abs(K) > 1e-3) > 0.5                        # far from diagonal
    el, eg = abs(ll - sll) / abs(sll), np.max(np.abs(gr - sg)) / np.max(np.abs(sg))
    print("d=%d kind %d: LL %.3e, gradient %.3e (of max|g|)" % (d, kind, el, eg))
    assert el <= CHUNK_TOL and eg <= CHUNK_TOL, (d, el, eg)


@pytest.mark.parametrize("kind", KINDS)
def test_fused_and_separate_final_sums_1300(gp_mod, kind):
    """The same at 1300 rows (231 trace blocks, hand-over blocks of the inverse)."""
    X, y = synth(1300, d=6, seed=5, scale=2.5)
    out = []
    for tuning in ({}, {TUNE_FINALIZE_FUSE_MAX: 0}):
        g = handle(gp_mod, X, y, HP, kind, tuning=tuning)
        out.append(list(g.loglik_grad()))
        g.close()
    assert same_bits(out[0], out[1])


# ------------------------------------------------------------------ 7. joint covariance and draws
@extended
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(truth.JOINT_CASES))
def test_joint_covariance_and_draws(gp_mod, oracle, name, kind):
    """cugp_predict_cov with and without noise against the truth's joint covariance, at the bound tests/test_gpu_accuracy.py
    and tests/test_gpu_predict_joint.py hold the SE joint covariance to (the variance's yardstick, the covariance floor)
    with F_MATERN; cov exactly symmetric, the mean cugp_predict's bits.  Draws: zero normals give the mean's bits, unit
    normals pick columns of the Cholesky factor of the library's own covariance (against LAPACK's factor of the same
    fp64 matrix: two backward-stable factorisations differ by about nt eps cond(cov) relative to the factor's scale)."""
    c = accuracy.live(oracle, tm.KIND_NAMES[kind], name)
    X, y, Xt, hp, t, noise, fl = c["X"], c["y"], c["Xt"], c["cov"].hp, c["t"], c["noise"], c["floor"]
    rep = Report("%s/%s" % (name, tm.KIND_NAMES[kind]), c["cov"])
    g = handle(gp_mod, X, y, hp, kind)
    m, _ = g.compute_test_means_and_variances(X, y, Xt)
    for with_noise in (True, False):
        tmj, tcov = t.joint(Xt, with_noise)
        mj, cov = g.compute_test_joint(X, y, Xt, with_noise=with_noise)
        assert np.array_equal(cov, cov.T) and same_bits([mj], [m])
        tag = "joint_noise_" if with_noise else "joint_latent_"
        rep.add(tag + "mean", np.max(np.abs(mj.astype(LD) - tmj)), noise["mean"], fl["mean"])
        rep.add(tag + "cov", np.max(np.abs(cov.astype(LD) - tcov)), noise["var"], fl["cov"])
    nt = Xt.shape[0]
    mj, cov = g.compute_test_joint(X, y, Xt, with_noise=True)
    z0 = g.sample_posterior(X, y, Xt, 2, with_noise=True, normals=np.zeros((2, nt)))
    assert same_bits([z0[0], z0[1]], [mj, mj])
    units = np.eye(nt)[[0, nt // 2, nt - 1]]
    draws = g.sample_posterior(X, y, Xt, 3, with_noise=True, normals=units)
    Lc = np.linalg.cholesky(cov)
    sv = float(np.exp(2 * hp[1]) + np.exp(2 * hp[2]))
    for s, k in enumerate((0, nt // 2, nt - 1)):
        err = np.max(np.abs(draws[s] - mj - Lc[:, k]))
        print("draw along unit normal %d: |sample - mean - C[:, k]| %.3e" % (k, err))
        assert err <= nt * 2.0 ** -52 * np.linalg.cond(cov) * np.sqrt(sv), (k, err)
    g.close()
    rep.check()


# ------------------------------------------------------------------ 8. BCM
@extended
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N, K", [(3 * 300, 3), (5 * 261 + 2, 5)], ids=["3x300", "5-uneven"])
def test_bcm_against_the_truth(gp_mod, oracle, N, K, kind):
    """A 3-expert group of equal experts (cugp_bcm_create_kernel + expert data) and an uneven 5-expert split
    (cugp_bcm_create_split's partition through BCM.split): summed LL and gradient and the product-of-experts prediction
    against truth.bcm_truth with the Matern truth, same bound.  cugp_bcm_predict equals the per-expert predictions
    combined in expert order by cugp_poe_finish, bit for bit."""
    d = 5
    X, y = synth(N, d=d, seed=N + K, scale=3.0)
    Xt = synth(truth.NT, d=d, seed=7, scale=3.0)[0]
    cov = truth.Matern(HP, kind)
    tb = truth.bcm_truth(X, y, cov, K, Xt)
    noise = truth.bcm_yardstick(oracle, cov, X, y, K, Xt, tb)[0]       # every expert through the oracle's linear algebra
    fl = truth.floors(cov, truth.scales(cov, tb["ll"], tb["grad"], tb["mean"]))
    parts = truth.bcm_rows(N, K)
    if K == 3:
        b = gp_mod.BCM([r for _, r in parts], d, kernel=kind)
        for k, (off, r) in enumerate(parts):
            b.set_expert_data(k, X[off: off + r], y[off: off + r])
    else:
        b = gp_mod.BCM.split(X, y, K, kernel=kind)
    assert b.rows == [r for _, r in parts] and b.kernel == tm.KIND_NAMES[kind]
    assert all(b.expert(k).kernel == tm.KIND_NAMES[kind] for k in range(K))
    b.set_BCM_log_hyperparam(HP)
    ll, gr, per = b.loglik_grad()
    m, v = b.compute_BCM_test_means_and_var(Xt)
    rep = Report("bcm%dx/%s" % (K, tm.KIND_NAMES[kind]), cov)
    rep.add_all("", truth.errors(cov, ll, gr, m, v, tb["ll"], tb["grad"], tb["mean"], tb["var"]), noise, fl)
    sp, spm = np.zeros(truth.NT), np.zeros(truth.NT)
    for k in range(K):
        mk, vk = b.expert(k).compute_test_means_and_variances(None, None, Xt)
        sp, spm = sp + 1.0 / vk, spm + (1.0 / vk) * mk
    pm, pv = gp_mod.poe_finish(sp, spm)
    print("bcm_predict against poe_finish of the experts: mean %.3e var %.3e" % (np.max(np.abs(pm - m)), np.max(np.abs(pv - v))))
    tr = b.cg_solve(budget=4)                                     # cugp_bcm_cg_solve runs on a Matern BCM
    assert tr.shape[0] >= 2 and tr.shape[1] == 4 and np.all(np.isfinite(tr)) and tr[-1, 3] <= tr[0, 3]
    b.close()
    assert same_bits([pm, pv], [m, v])
    rep.check()


def test_group_of_mixed_kinds_is_refused(gp_mod):
    L = capi.lib()
    L.cugp_group_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_void_p)]
    L.cugp_group_destroy.argtypes = [C.c_void_p]
    L.cugp_group_destroy.restype = None
    gs = [gp_mod.Covsum(200, 3, kernel=k) for k in ("matern32", "matern32", "matern52", "se")]
    grp = C.c_void_p()
    for pair in ((0, 2), (0, 3), (3, 2)):
        hs = (C.c_void_p * 2)(*[gs[i].handle for i in pair])
        assert L.cugp_group_create(hs, 2, C.byref(grp)) == capi.CUGP_ERR_INVALID
        assert b"kernel kinds" in L.cugp_last_error() and not grp.value
    hs = (C.c_void_p * 2)(gs[0].handle, gs[1].handle)
    capi.check(L.cugp_group_create(hs, 2, C.byref(grp)))
    L.cugp_group_destroy(grp)
    for g in gs:
        g.close()


@pytest.mark.parametrize("kind", KINDS)
def test_sharded_bcm_one_rank_has_bcm_bits(gp_mod, kind):
    """ShardedBCM(kernel=) at one rank through the library's exchange (cugp_bcm_loglik_grad_allgather,
    cugp_bcm_predict_allgather; a world of one needs no RCCL): the bits of gp.BCM over the same experts."""
    import torch
    from cugp_amd.bcm import ShardedBCM
    X, y = synth(3 * 300, 5, seed=4)
    experts = [(X[300 * k:300 * (k + 1)], y[300 * k:300 * (k + 1)]) for k in range(3)]
    Xt = np.random.default_rng(1).uniform(-10, 10, (70, 5))
    env = os.environ.pop("CUGP_BCM_EXCHANGE", None)
    try:
        sb = ShardedBCM(experts, rank=0, world=1, device=0, comm_device=torch.device("cuda", 0), kernel=kind)
    finally:
        if env is not None:
            os.environ["CUGP_BCM_EXCHANGE"] = env
    assert sb.exchange_form == "library" and sb.kernel == tm.KIND_NAMES[kind]
    ref = gp_mod.BCM([300, 300, 300], 5, 0, kernel=kind)
    for k, (Xk, yk) in enumerate(experts):
        ref.set_expert_data(k, Xk, yk)
    hp = [1.2, 0.3, -0.8]
    sb.set_loghyper(hp)
    ref.set_BCM_log_hyperparam(hp)
    ll, g, per = sb.loglik_grad()
    ll0, g0, per0 = ref.loglik_grad()
    m, v = sb.predict(Xt)
    assert sb.predict_form == "library"
    m0, v0 = ref.compute_BCM_test_means_and_var(Xt)
    sb.close()
    ref.close()
    assert same_bits([ll, g, per, m, v], [ll0, g0, per0, m0, v0])


# ------------------------------------------------------------------ 9. the optimisers
@pytest.mark.parametrize("kind", KINDS)
def test_optimisers(gp_mod, kind):
    """cugp_cg_solve (budget 60) on a Matern handle against cugp_cg_minimize driven by the fp64 stand-in objective, at
    the tolerances DESIGN.md section 9 states: probe for probe while the objective still moves (5e-5), end point 5e-5,
    final objective 1e-7.  The evaluation-sparing form reaches the same end point; RPROP lowers the objective."""
    X, y = synth(300, d=4, scale=3.0)
    start = [0.5, 0.5, 0.5]
    fn = tm.standin_objective(X, y, kind)
    th_cpu, tr_cpu = gp_mod.cg_minimize(fn, start, 60)
    g = handle(gp_mod, X, y, start, kind)
    tr = g.cg_solve(budget=60)
    th = g.get_loghyperparam()
    f_end = -g.compute_loglikelihood()
    g.close()
    f_cpu = fn(th_cpu)[0]
    n = min(len(tr), len(tr_cpu))
    err = np.abs(tr[:n, :3] - tr_cpu[:n, :3]) / np.maximum(1.0, np.abs(tr_cpu[:n, :3]))
    moving = np.abs(tr_cpu[:n, 3] - f_cpu) > 1e-9 * abs(f_cpu)
    print("cg_solve kind %d: %d probes (CPU %d), %d while the objective moves, max rel. deviation there %.2e; end %s f %.10g (CPU %.10g)"
          % (kind, len(tr), len(tr_cpu), moving.sum(), np.max(err[moving]), th, f_end, f_cpu))
    assert moving.sum() >= 10 and np.all(err[moving] <= 5e-5), (int(moving.sum()), float(np.max(err[moving])))
    assert np.allclose(th, th_cpu, atol=5e-5), (th, th_cpu)
    assert abs(f_end - f_cpu) <= 1e-7 * abs(f_cpu), (f_end, f_cpu)

    g = handle(gp_mod, X, y, start, kind)
    trs, ng = g.cg_solve_sparing(budget=60)
    ths = g.get_loghyperparam()
    g.close()
    print("sparing: %d probes, %d gradients, end %s" % (len(trs), ng, ths))
    assert ng < len(trs) and np.allclose(ths, th, atol=5e-5), (ths, th)

    g = handle(gp_mod, X, y, start, kind)
    f0 = -g.compute_loglikelihood()
    trr = g.rprop_solve(iters=30)
    f1 = -g.compute_loglikelihood()
    g.close()
    print("rprop: %d rows, -LL %.10g -> %.10g" % (len(trr), f0, f1))
    assert len(trr) == 60 and f1 < f0 - 1.0, (f0, f1)
