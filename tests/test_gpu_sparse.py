"""GPU tests of sparse variational GP regression on inducing points (cugp_sparse_*; SparseGP).

Accuracy is held to fp64 rounding against the extended-precision truth of tests/truth_sparse.py:

    err_gpu(q) <= F_SPARSE[family] * max(yardstick(q), 4 ulp of q's scale)

for F (relative), every gradient component (relative to max|g|), the mean (largest absolute error) and the variance (largest
absolute error, floored at 4 ulp of sf2 + sn2) at 20 test points; the yardstick is the computed form in fp64 numpy / LAPACK
on the whole data at once over the data as given and truth.permutations; F_SPARSE was fixed on the CPU
(tests/test_truth_sparse_cpu.py, docs/ACCURACY.md), never from the GPU.  Every figure is printed before it is asserted
("ACC <case> <quantity> err noise floor ratio"; run with -s).  One process, one device; nothing outside the tree is read.

What the accuracy cases cover (truth_sparse.CASES: family, N, M, d, chunk_rows):
  se 128 / 128 / 2 / 128            no padding anywhere, one chunk
  se 300 / 65 / 2 / 128             three chunks, a ragged last chunk of 44 rows, identity padding of mpad
  se 1300 / 200 / 6 / 512           two M tiles, three lower output tiles, the Gram launch split in 2 over k
  matern32 300 / 65 / 2 / 128
  ard 300 / 130 / 17 / 256          two feature chunks, two M tiles
  matern52_ard 257 / 64 / 3 / 128
  se 300 / 2 x 60 / 2 / 128         Z = 60 rows and the same rows shifted by 1e-4: cond(Kuu) ~ sf2 M / eps
  se 800 / 65 / 3 / 0               the default chunk: one 896-row pass, the Gram launch split in 3 at kstep 304 -- 19, 19 and
                                    18 stages of 16: the odd-stage tail of the double-buffered loop, a shorter last split
  matern52 800 / 65 / 3 / 0         the same shape on isotropic Matern 5/2
  matern32_ard 1000 / 130 / 3 / 896 Matern-3/2-ARD; two passes (896 rows split in 3, then 104 added to P), two M tiles
  matern32_ard 257 / 64 / 3 / 128   its sibling with a central-difference check of the truth (tests/test_truth_sparse_cpu.py)
  se 1300 / 260 / 6 / 0             mpad 384: six lower output tiles, 6 x 6 grids of the 64-wide passes, the products over
                                    k = 384; one 1408-row pass split in 5 at kstep 288 (18, 18, 18, 18 and 16 stages)
  matern52 300 / 65 / 32 / 128      d an exact multiple of the feature chunk of 16
  ard 300 / 65 / 33 / 128           three feature chunks, the last of one feature
  se 300 / 16 / 3 / 0               the model of the two-pass prediction (tests/test_gpu_sparse_wide.py)
"""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

import truth
import truth_sparse as ts
from accuracy import Report
from cugp_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import sparse_bits_record  # noqa: E402

pytestmark = pytest.mark.gpu
extended = pytest.mark.skipif(not truth.EXTENDED, reason="numpy.longdouble is not an extended-precision type here")

LD = truth.LD
NAMES = list(ts.CASES)


@pytest.fixture(scope="module")
def gp_mod():
    import cugp_amd.gp as gp
    return gp


def make(gp_mod, name, chunk_rows=None, hp=None, data=True, inducing=True):
    """A SparseGP of the case with its hyper-parameters, data and inducing inputs set -> (handle, inputs)."""
    family, N, M, d = ts.CASES[name][:4]
    X, y, Z, Xt, cov, chunk = ts.inputs(name)
    kernel = family if family.startswith("matern") else "se"
    s = gp_mod.SparseGP(N, M, d, kernel=kernel, ard=family == "ard", jitter=ts.JITTER,
                        chunk_rows=chunk if chunk_rows is None else chunk_rows)
    if data:
        s.set_data(X, y)
    if inducing:
        s.set_inducing(Z)
    s.set_loghyperparam(cov.hp if hp is None else hp)
    return s, (X, y, Z, Xt, cov)


def bits(*arrays):
    return [np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).copy() for a in arrays]


def same_bits(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(bits(*a), bits(*b)))


def everything(s, Xt):
    """(F, grad, mean, var) of a handle, ready for bit comparison."""
    F, g = s.bound_grad()
    return (np.float64(F), g) + s.predict(Xt)


# ------------------------------------------------------------------ 1. accuracy
@extended
@pytest.mark.parametrize("name", NAMES)
def test_accuracy(gp_mod, name):
    c = ts.case(name)
    s, (X, y, Z, Xt, cov) = make(gp_mod, name)
    assert len(s.plan()) == -(-len(y) // ts.chunk_of(c["chunk"]))
    only = s.bound()
    F, g, m, v = everything(s, Xt)
    assert same_bits([only], [F])                              # the bound alone carries the bits of the full call
    assert g.shape == (len(cov.hp),) and m.shape == v.shape == (ts.NT,)
    rep = Report("sparse/" + name, cov)
    ts.hold(rep, c, F, g, m, v)
    ml, vl = s.predict(Xt, with_noise=False)
    assert same_bits([ml], [m])
    rep.add("latent_var", np.max(np.abs(vl.astype(LD) - (c["tv"] - cov.sn2))), c["noise"]["var"], c["floor"]["var"],
            ts.F_SPARSE[c["family"]])
    s.close()
    rep.check()


# ------------------------------------------------------------------ 2. determinism
@pytest.mark.parametrize("name", ["se_n1300_m200", "ard_n300_m130_d17", "se_n800_m65_d3_c0", "se_n1300_m260_c0"])
def test_bit_identical_on_repeat_and_on_a_second_handle(gp_mod, name):
    s, (X, y, Z, Xt, cov) = make(gp_mod, name)
    first = everything(s, Xt)
    moved = np.asarray(cov.hp) + 0.25
    s.set_loghyperparam(moved)
    away = everything(s, Xt)
    assert not same_bits(away[:1], first[:1])
    s.set_loghyperparam(cov.hp)                                 # moved back: a new evaluation, the same bits
    assert same_bits(everything(s, Xt), first)
    s.set_data(X, y)                                            # the same data again: launched again, the same bits
    assert same_bits(everything(s, Xt), first)
    twin, _ = make(gp_mod, name)
    assert same_bits(everything(twin, Xt), first)
    # the bound alone, then the gradient on top of it: the bits of the one call
    third, _ = make(gp_mod, name)
    F = third.bound()
    assert same_bits([F], first[:1]) and same_bits(everything(third, Xt), first)
    for h in (s, twin, third):
        h.close()


# ------------------------------------------------------------------ 3. chunk independence, to the bound
@extended
def test_chunk_rows_128_against_256(gp_mod):
    name = "se_n300_m65"
    c = ts.case(name)
    outs = []
    for chunk in (128, 256):
        s, (X, y, Z, Xt, cov) = make(gp_mod, name, chunk_rows=chunk)
        assert [p[1] for p in s.plan()] == ([128, 128, 44] if chunk == 128 else [256, 44])
        out = everything(s, Xt)
        rep = Report("sparse/%s/chunk%d" % (name, chunk), cov)
        ts.hold(rep, c, *out)
        rep.check()
        outs.append(out)
        s.close()
    print("CHUNK F 128: %.17g  256: %.17g" % (outs[0][0], outs[1][0]))


@extended
def test_chunk_rows_at_the_odd_split(gp_mod):
    """The default chunk (0) and 896 give the same plan -- one 896-row pass split in 3 at kstep 304 -- and so the same bits;
    512 and 128 give other partial sums in another order: each is held to the bound."""
    name = "se_n800_m65_d3_c0"
    c = ts.case(name)
    rows = {0: [800], 896: [800], 512: [512, 288], 128: [128] * 6 + [32]}
    outs = {}
    for chunk in (0, 896, 512, 128):
        s, (X, y, Z, Xt, cov) = make(gp_mod, name, chunk_rows=chunk)
        if chunk in (0, 896):
            assert s.plan() == [(0, 800, 896, 3, 304)]
        assert [p[1] for p in s.plan()] == rows[chunk]
        out = everything(s, Xt)
        rep = Report("sparse/%s/chunk%d" % (name, chunk), cov)
        ts.hold(rep, c, *out)
        rep.check()
        outs[chunk] = out
        s.close()
    print("CHUNK F " + "  ".join("%d: %.17g" % (k, v[0]) for k, v in outs.items()))
    assert same_bits(outs[0], outs[896])


# ------------------------------------------------------------------ 4. staleness
def test_predict_after_set_loghyper_re_evaluates(gp_mod):
    name = "matern32_n300_m65"
    s, (X, y, Z, Xt, cov) = make(gp_mod, name)
    old = s.predict(Xt)
    hp2 = np.asarray(cov.hp) - 0.2
    fresh, _ = make(gp_mod, name, hp=hp2)
    want = fresh.predict(Xt)                                    # (a prediction first: it evaluates the bound itself)
    s.set_loghyperparam(hp2)
    got = s.predict(Xt)
    assert same_bits(got, want) and not same_bits(got, old)
    assert same_bits([s.bound()], [fresh.bound()])
    s.set_inducing(Z[::-1].copy())                              # new inducing inputs: stale again
    s.set_inducing(Z)
    assert same_bits(s.predict(Xt), want)
    s.close()
    fresh.close()


# ------------------------------------------------------------------ 5. a lower bound on the exact model's LL
@extended
@pytest.mark.parametrize("name", [n for n in NAMES if ts.CASES[n][1] == 300])
def test_bound_is_below_the_exact_log_likelihood(gp_mod, name):
    """F <= cugp_loglik of an exact handle at the same theta.  The tolerance is the two quantities' own bounds: F is held to
    F_SPARSE max(yardstick, 4 ulp) |F| (test_accuracy), LL to the family's factor times 4 ulp |LL| at least."""
    family = ts.CASES[name][0]
    s, (X, y, Z, Xt, cov) = make(gp_mod, name)
    F = s.bound()
    g = gp_mod.Covsum(X.shape[0], X.shape[1], ard=family == "ard", kernel=family if family.startswith("matern") else "se")
    g.set_loghyperparam(cov.hp)
    ll = g.compute_loglikelihood(X, y)
    c = ts.case(name)
    tol = ts.F_SPARSE[family] * max(c["noise"][cov.quantities[0]], truth.U4) * abs(F) + cov.F * truth.U4 * abs(ll)
    print("BOUND %-24s F %.12f  LL %.12f  tolerance %.3e" % (name, F, ll, tol))
    assert F <= ll + tol
    g.close()
    s.close()


# ------------------------------------------------------------------ 6. the optimiser
@pytest.mark.parametrize("name", ["se_n300_m65", "matern52_ard_n257_m64"])
def test_cg_solve(gp_mod, name):
    """The first trace row is -F at the start, to the bit; the objective never rises along the trace and ends below its
    start; the last row is the end point, which stays set; the row behind the last is NaN and nothing beyond is written."""
    s, (X, y, Z, Xt, cov) = make(gp_mod, name)
    start = np.asarray(cov.hp, dtype=np.float64)
    F0 = s.bound()
    tr = s.cg_solve(budget=12)
    end = s.get_loghyperparam()
    f = tr[:, -1]
    print("CG-SPARSE %s objective along the trace:" % name, " ".join("%.6f" % v for v in f))
    assert tr.shape[1] == len(start) + 1 and tr.shape[0] >= 2
    assert np.array_equal(tr[0, :-1], start) and same_bits([tr[0, -1]], [-F0])
    assert np.all(np.isfinite(tr)) and np.array_equal(tr[-1, :-1], end)
    assert np.all(f[1:] <= f[:-1]) and f[-1] < f[0], f
    assert same_bits([-s.bound()], [f[-1]])
    s.set_loghyperparam(start)
    raw, ne = np.full((4 * 12 + 8, len(start) + 1), 7.0), C.c_int()
    capi.check(capi.lib().cugp_sparse_cg_solve(s.handle, 12, capi.ptr(raw), raw.shape[0], C.byref(ne)))
    k = tr.shape[0]
    assert k <= ne.value <= 13
    assert same_bits([raw[:k]], [tr]) and np.all(np.isnan(raw[k])) and np.all(raw[k + 1:] == 7.0)
    s.close()


# ------------------------------------------------------------------ 7. the existing results of other handles
def test_an_ordinary_covsum_before_and_after(gp_mod):
    X, y, Xt, cov = truth.family_inputs("se", "n257_d3")

    def existing():
        g = gp_mod.Covsum(X.shape[0], X.shape[1])
        g.set_loghyperparam(cov.hp)
        ll, gr = g.loglik_grad(X, y)
        m, v = g.compute_test_means_and_variances(X, y, Xt)
        out = (np.float64(ll), gr, m, v, g.get_K_inverse(), g.get_alpha())
        g.close()
        return out
    before = existing()
    s, (_, _, _, Xs, _) = make(gp_mod, "se_n1300_m200")
    everything(s, Xs)
    during = existing()                                         # the sparse handle still alive
    s.close()
    assert same_bits(during, before) and same_bits(existing(), before)


# ------------------------------------------------------------------ 8. refusals, on the device
def test_refusals(gp_mod):
    L = capi.lib()
    name = "se_n300_m65"
    s, (X, y, Z, Xt, cov) = make(gp_mod, name)
    a, _ = make(gp_mod, "matern52_ard_n257_m64")
    out, F, ne, h = np.zeros(8), C.c_double(7.0), C.c_int(7), C.c_void_p()

    def refused(rc, call):
        return rc == capi.CUGP_ERR_INVALID and call.encode() in L.cugp_last_error()
    for bad in ((100, 0, 2, 0, 0, 0, 1e-6, 0), (100, 10, 2, 0, 3, 0, 1e-6, 0), (100, 10, 2, 0, 0, 0, 1e-6, 100),
                (100, 32769, 2, 0, 0, 0, 1e-6, 0), (100, 10, 2, 0, 0, 0, 0.0, 0)):
        assert refused(L.cugp_sparse_create(*bad, C.byref(h)), "cugp_sparse_create") and not h.value
    assert refused(L.cugp_sparse_set_loghyper(s.handle, capi.ptr(out), 4), "cugp_sparse_set_loghyper")     # isotropic: 3
    assert refused(L.cugp_sparse_get_loghyper(a.handle, capi.ptr(out), 3), "cugp_sparse_get_loghyper")     # this ARD handle: 5
    assert refused(L.cugp_sparse_bound_grad(s.handle, C.byref(F), capi.ptr(out), 4), "cugp_sparse_bound_grad")
    assert refused(L.cugp_sparse_bound_grad(a.handle, C.byref(F), capi.ptr(out), 3), "cugp_sparse_bound_grad")
    assert refused(L.cugp_sparse_bound(s.handle, None), "cugp_sparse_bound")
    assert refused(L.cugp_sparse_predict(s.handle, capi.ptr(out), 0, 1, capi.ptr(out), capi.ptr(out)), "cugp_sparse_predict")
    assert refused(L.cugp_sparse_predict(s.handle, None, 1, 1, capi.ptr(out), capi.ptr(out)), "cugp_sparse_predict")
    for budget in (0, -1):
        assert refused(L.cugp_sparse_cg_solve(s.handle, budget, None, 0, C.byref(ne)), "cugp_sparse_cg_solve")
    nodata, _ = make(gp_mod, name, data=False)
    noz, _ = make(gp_mod, name, inducing=False)
    for e in (nodata, noz):
        assert refused(L.cugp_sparse_bound(e.handle, C.byref(F)), "cugp_sparse_bound")
        assert refused(L.cugp_sparse_bound_grad(e.handle, C.byref(F), capi.ptr(out), 3), "cugp_sparse_bound_grad")
        assert refused(L.cugp_sparse_predict(e.handle, capi.ptr(out), 1, 1, capi.ptr(out), capi.ptr(out)), "cugp_sparse_predict")
        assert refused(L.cugp_sparse_cg_solve(e.handle, 5, None, 0, C.byref(ne)), "cugp_sparse_cg_solve")
    assert (F.value, ne.value) == (7.0, 7) and not out.any()
    # the refusals left the handles usable
    assert np.isfinite(s.bound()) and a.bound_grad()[1].shape == (5,)
    nodata.set_data(X, y)
    assert same_bits([nodata.bound()], [s.bound()])
    for e in (s, a, nodata, noz):
        e.close()


# ------------------------------------------------------------------ 9. the recorded bits
@pytest.mark.parametrize("model", sorted(sparse_bits_record.MODELS))
def test_own_y_and_targets_keep_the_recorded_bits(model):
    """tests/golden/sparse_own_bits.json holds the fp64 words of bound, bound_grad, bound_grad_z, predict, predict_joint and
    predict_grad for the handle's own y on two small models, and of bound_grad_targets with p = 1 and p = 3 on the first
    (tools/sparse_bits_record.py: the models, and what each reaches), recorded on an MI355X at the last commit that had a
    kernel family of its own for the handle's y.  The one family that serves both sides now gives every one of these words:
    equality to the bit, no tolerance."""
    with open(os.path.join(ROOT, "tests", "golden", "sparse_own_bits.json")) as f:
        want = json.load(f)[model]
    got = sparse_bits_record.results(model)
    assert sorted(got) == sorted(want)
    differ = {k: sum(a != b for a, b in zip(got[k], want[k])) for k in want if got[k] != want[k]}
    for k in sorted(want):
        print("BITS %s %-28s %4d words  %s" % (model, k, len(want[k]), "same" if k not in differ else "%d DIFFER" % differ[k]))
    assert all(len(got[k]) == len(want[k]) for k in want) and not differ, differ
