"""GPU tests of multi-target regression over one set of inducing points (cugp_sparse_*_targets; SparseGP.*_targets).

Accuracy is held to fp64 rounding against the extended-precision truth of tests/truth_sparse_targets.py:

    err_gpu(q) <= F_SPARSE_TARGETS[family] * max(yardstick(q), 4 ulp of q's scale)         (gZ: F_SPARSE_TARGETS_Z)

for F and every F_t (relative), every gradient component (relative to max|g|), gZ (relative to max|gZ|), the means of all
targets (largest absolute error) and the variance (largest absolute error) at 20 test points; the yardstick is
truth_sparse.computed_form per target, summed in target order, over the data as given and truth.permutations; the factors
were fixed on the CPU (tests/test_truth_sparse_targets_cpu.py, docs/ACCURACY.md), never from the GPU.  Every figure is
printed before it is asserted (run with -s).  One process, one device; nothing outside the tree is read.

What the accuracy cases cover (truth_sparse_targets.CASES: case of truth_sparse.CASES, p):
  se_n128_m128 / 1             one target, no padding anywhere
  se_n300_m65 / 3              three chunks, a ragged last chunk of 44 rows, identity padding of mpad
  se_n1300_m200 / 17           two M tiles, split-k; three groups of 8 targets in the Q pass, two staging rounds of 16 in the
                               H and weight passes, the last group and round of ONE target
  ard_n300_m130_d17 / 5        two feature chunks, two M tiles
  matern32_ard_n1000_m130 / 9  two passes of the data, W_c recomputed; a second group of one target
  matern52_n800_m65_d3_c0 / 2  the default chunk
  se_n300_dup60 / 3            near-singular Kuu
"""
import ctypes as C

import numpy as np
import pytest

import truth
import truth_sparse as ts
import truth_sparse_targets as tst
from accuracy import Report
from cugp_amd import capi

pytestmark = pytest.mark.gpu
extended = pytest.mark.skipif(not truth.EXTENDED, reason="numpy.longdouble is not an extended-precision type here")

LD = truth.LD


@pytest.fixture(scope="module")
def gp_mod():
    import cugp_amd.gp as gp
    return gp


def make(gp_mod, name, p=None, chunk_rows=None, hp=None, data=True, inducing=True):
    """A SparseGP of the case with its hyper-parameters, data, inducing inputs and (p given) targets set."""
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
    if p:
        s.set_targets(tst.targets(name, p).T)
    return s, (X, y, Z, Xt, cov)


def bits(*arrays):
    return [np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).copy() for a in arrays]


def same_bits(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(bits(*a), bits(*b)))


def everything(s, Xt):
    """(F, grad, F_each, means [p, nt], var, gZ) of a handle's targets, ready for bit comparison and for tst.hold."""
    F, g, gZ, each = s.bound_grad_z_targets()
    m, v = s.predict_targets(Xt)
    return np.float64(F), g, each, m, v, gZ


def single(s, Xt):
    """The single-target calls on the handle's own y."""
    F, g = s.bound_grad()
    Fz, gz_, gZ = s.bound_grad_z()
    return (np.float64(F), g, np.float64(Fz), gz_, gZ) + s.predict(Xt)


# ------------------------------------------------------------------ 1. accuracy
@extended
@pytest.mark.parametrize("name, p", tst.CASES, ids=["%s-p%d" % c for c in tst.CASES])
def test_accuracy(gp_mod, name, p):
    c = tst.case(name, p)
    s, (X, y, Z, Xt, cov) = make(gp_mod, name, p)
    assert s.num_targets == p
    F0, each0 = s.bound_targets()
    F1, g1, each1 = s.bound_grad_targets()
    F, g, each, m, v, gZ = everything(s, Xt)
    # the bound alone, the gradient, and the gradient with gZ carry the same bits
    assert same_bits([F0, each0], [F1, each1]) and same_bits([F1, g1, each1], [F, g, each])
    assert g.shape == (len(cov.hp),) and each.shape == (p,) and m.shape == (p, ts.NT) and v.shape == (ts.NT,)
    assert gZ.shape == Z.shape
    rep = Report("sparse_targets/%s/p%d" % (name, p), cov)
    tst.hold(rep, c, F, g, each, m, v, gZ)
    ml, vl = s.predict_targets(Xt, with_noise=False)
    assert same_bits([ml], [m])
    rep.add("latent_var", np.max(np.abs(vl.astype(LD) - (c["tv"] - cov.sn2))), c["noise"]["var"], c["floor"]["var"],
            tst.factor(c, "var"))
    s.close()
    rep.check()


# ------------------------------------------------------------------ 2. beyond one test tile
@extended
@pytest.mark.parametrize("nt", [129, 257])
def test_wide(gp_mod, nt):
    name, p = "se_n300_m65", 3
    c = tst.case(name, p)
    w = tst.wide_case(name, p, nt)
    s, _ = make(gp_mod, name, p)
    m, v = s.predict_targets(w["Xt"])
    assert m.shape == (p, nt) and v.shape == (nt,)
    rep = Report("sparse_targets/%s/nt%d" % (name, nt), c["cov"])
    tst.hold_wide(rep, c, w, m, v)
    assert same_bits([v], [s.predict(w["Xt"])[1]])
    s.close()
    rep.check()


@extended
def test_two_passes(gp_mod):
    """nt = P + 129 on the model of truth_sparse's two-pass prediction with p = 2: the second pass writes each target's row
    at its offset of the [p][nt] result.  Every row of both target rows is held."""
    name, p = ts.TWO_PASS_NAME, 2
    c = tst.case(name, p)
    s, (X, y, Z, _, cov) = make(gp_mod, name, p)
    P = gp_mod.sparse_predict_plan(s.m, 1 << 30)[0][1]
    nt = P + 129
    assert s.predict_plan(nt) == [(0, P), (P, 129)]
    w = tst.wide_case(name, p, nt, z_row=P, data_row=P - 1)
    m, v = s.predict_targets(w["Xt"])
    assert m.shape == (p, nt) and np.all(np.isfinite(m)) and np.all(np.isfinite(v))
    rep = Report("sparse_targets/%s/two_passes" % name, cov)
    tst.hold_wide(rep, c, w, m, v)
    # the rows of the second pass predicted alone: the same bits at an offset
    m2, v2 = s.predict_targets(w["Xt"][P:])
    assert same_bits([m[:, P:], v[P:]], [m2, v2])
    assert same_bits([v], [s.predict(w["Xt"])[1]])
    s.close()
    rep.check()


# ------------------------------------------------------------------ 3. the variance and the existing results
@pytest.mark.parametrize("name, p", [("se_n1300_m200", 17), ("matern32_ard_n1000_m130", 9)])
def test_variance_and_single_target_results_are_untouched(gp_mod, name, p):
    s, (X, y, Z, Xt, cov) = make(gp_mod, name)
    before = single(s, Xt)
    s.set_targets(tst.targets(name, p).T)
    assert same_bits(single(s, Xt), before)                     # after set_targets
    out = everything(s, Xt)                                     # a targets evaluation: b and P are rewritten
    assert same_bits([out[4]], [before[-1]])                    # predict_targets' var has predict's bits
    assert same_bits(single(s, Xt), before)                     # ... and the single-target calls evaluate again
    assert same_bits(everything(s, Xt), out)                    # ... as do the targets', with their bits
    # interleaved without a full evaluation in between
    assert same_bits([s.predict(Xt)[1]], [s.predict_targets(Xt)[1]])
    assert same_bits([s.bound()], [before[0]]) and same_bits([s.bound_targets()[0]], [out[0]])
    s.close()


# ------------------------------------------------------------------ 4. independence of the targets
def test_a_target_does_not_depend_on_the_others(gp_mod):
    name = "se_n1300_m200"
    wide, (X, y, Z, Xt, cov) = make(gp_mod, name, 17)
    narrow, _ = make(gp_mod, name, 3)
    F17, each17 = wide.bound_targets()
    F3, each3 = narrow.bound_targets()
    m17, m3 = wide.predict_targets(Xt)[0], narrow.predict_targets(Xt)[0]
    assert same_bits([each17[:3], m17[:3]], [each3, m3]) and F17 != F3
    Y = tst.targets(name, 3)
    Y[1] = Y[1][::-1] * 0.5
    narrow.set_targets(Y.T)
    F3b, each3b = narrow.bound_targets()
    m3b = narrow.predict_targets(Xt)[0]
    assert same_bits([each3b[[0, 2]], m3b[[0, 2]]], [each3[[0, 2]], m3[[0, 2]]])
    assert each3b[1] != each3[1] and not np.array_equal(m3b[1], m3[1])
    # target 0 is the handle's own y: its F_t is the single-target bound to rounding (another order of the M-side products)
    assert abs(each3[0] - narrow.bound()) <= 1e-10 * abs(each3[0])
    for h in (wide, narrow):
        h.close()


# ------------------------------------------------------------------ 5. determinism
@pytest.mark.parametrize("name, p", [("se_n1300_m200", 17), ("ard_n300_m130_d17", 5)])
def test_bit_identical_on_repeat_and_on_a_second_handle(gp_mod, name, p):
    s, (X, y, Z, Xt, cov) = make(gp_mod, name, p)
    first = everything(s, Xt)
    s.set_loghyperparam(np.asarray(cov.hp) + 0.25)
    away = everything(s, Xt)
    assert not same_bits(away[:1], first[:1])
    s.set_loghyperparam(cov.hp)
    assert same_bits(everything(s, Xt), first)
    twin, _ = make(gp_mod, name, p)
    assert same_bits(everything(twin, Xt), first)
    third, _ = make(gp_mod, name, p)                             # the bound alone, then the rest on top of it
    assert same_bits([third.bound_targets()[0]], first[:1]) and same_bits(everything(third, Xt), first)
    for h in (s, twin, third):
        h.close()


# ------------------------------------------------------------------ 6. chunk independence, to the bound
@extended
def test_chunk_rows_128_against_256(gp_mod):
    name, p = "se_n300_m65", 3
    c = tst.case(name, p)
    Fs = []
    for chunk in (128, 256):
        s, (X, y, Z, Xt, cov) = make(gp_mod, name, p, chunk_rows=chunk)
        assert [q[1] for q in s.plan()] == ([128, 128, 44] if chunk == 128 else [256, 44])
        out = everything(s, Xt)
        rep = Report("sparse_targets/%s/chunk%d" % (name, chunk), cov)
        tst.hold(rep, c, *out)
        rep.check()
        Fs.append(out[0])
        s.close()
    print("CHUNK-TARGETS F 128: %.17g  256: %.17g" % tuple(Fs))


# ------------------------------------------------------------------ 7. staleness
def test_staleness(gp_mod):
    name, p = "se_n300_m65", 3
    s, (X, y, Z, Xt, cov) = make(gp_mod, name, p)
    old = everything(s, Xt)
    hp2 = np.asarray(cov.hp) - 0.2
    fresh, _ = make(gp_mod, name, p, hp=hp2)
    want = everything(fresh, Xt)
    s.set_loghyperparam(hp2)
    got = s.predict_targets(Xt)                                 # (a prediction first: it evaluates by itself)
    assert same_bits(got, want[3:5]) and not same_bits(got[:1], old[3:4])
    assert same_bits(everything(s, Xt), want)
    s.set_inducing(Z[::-1].copy())                              # new inducing inputs: stale
    other = everything(s, Xt)
    assert not same_bits(other[:1], want[:1])
    s.set_inducing(Z)
    assert same_bits(everything(s, Xt), want)
    Y = tst.targets(name, p)
    s.set_targets((Y * 1.5).T)                                  # new targets: stale
    scaled = everything(s, Xt)
    assert not same_bits(scaled[:1], want[:1]) and same_bits([scaled[4]], [want[4]])
    s.set_targets(tst.targets(name, 5).T)                       # another p
    assert s.num_targets == 5 and s.bound_targets()[1].shape == (5,) and s.predict_targets(Xt)[0].shape == (5, ts.NT)
    s.set_targets(Y.T)
    assert s.num_targets == p and same_bits(everything(s, Xt), want)
    s.set_data(X, y)                                            # the same data again: the targets persist, the same bits
    assert s.num_targets == p and same_bits(everything(s, Xt), want)
    for h in (s, fresh):
        h.close()


# ------------------------------------------------------------------ 8. the optimiser
@pytest.mark.parametrize("inducing", [False, True])
def test_cg_solve_targets(gp_mod, inducing):
    name, p = "matern52_n800_m65_d3_c0", 2
    s, (X, y, Z, Xt, cov) = make(gp_mod, name, p)
    start = np.asarray(cov.hp, dtype=np.float64)
    F0 = s.bound_targets()[0]
    tr = s.cg_solve_targets(budget=8, inducing=inducing)
    end = s.get_loghyperparam()
    f = tr[:, -1]
    print("CG-SPARSE-TARGETS inducing %s objective along the trace:" % inducing, " ".join("%.6f" % v for v in f))
    assert tr.shape[1] == len(start) + 1 and tr.shape[0] >= 2
    assert np.array_equal(tr[0, :-1], start) and same_bits([tr[0, -1]], [-F0])
    assert np.all(np.isfinite(tr)) and np.array_equal(tr[-1, :-1], end)
    assert np.all(f[1:] <= f[:-1]) and f[-1] < f[0], f
    assert same_bits([-s.bound_targets()[0]], [f[-1]])          # at the returned theta (and Z)
    assert np.array_equal(s.get_inducing(), Z) != inducing
    s.close()


# ------------------------------------------------------------------ 9. refusals, on the device
def test_refusals(gp_mod):
    L = capi.lib()
    name = "se_n300_m65"
    s, (X, y, Z, Xt, cov) = make(gp_mod, name, 3)
    out, big, F, ne = np.zeros(8), np.zeros(3 * 300), C.c_double(7.0), C.c_int(7)
    P = capi.ptr

    def refused(rc, call):
        return rc == capi.CUGP_ERR_INVALID and call.encode() in L.cugp_last_error()
    assert refused(L.cugp_sparse_set_targets(s.handle, None, 3), "cugp_sparse_set_targets")
    assert refused(L.cugp_sparse_set_targets(s.handle, P(big), 0), "cugp_sparse_set_targets")
    assert refused(L.cugp_sparse_set_targets(s.handle, P(big), -2), "cugp_sparse_set_targets")
    assert refused(L.cugp_sparse_num_targets(s.handle, None), "cugp_sparse_num_targets")
    assert refused(L.cugp_sparse_bound_targets(s.handle, None, P(out)), "cugp_sparse_bound_targets")
    assert refused(L.cugp_sparse_bound_grad_targets(s.handle, C.byref(F), P(out), 4, None), "cugp_sparse_bound_grad_targets")
    assert refused(L.cugp_sparse_bound_grad_targets(s.handle, C.byref(F), None, 3, None), "cugp_sparse_bound_grad_targets")
    assert refused(L.cugp_sparse_bound_grad_z_targets(s.handle, C.byref(F), P(out), 3, None, None),
                   "cugp_sparse_bound_grad_z_targets")
    assert refused(L.cugp_sparse_bound_grad_z_targets(s.handle, C.byref(F), P(out), 5, P(big), None),
                   "cugp_sparse_bound_grad_z_targets")
    assert refused(L.cugp_sparse_predict_targets(s.handle, P(out), 0, 1, P(big), P(out)), "cugp_sparse_predict_targets")
    assert refused(L.cugp_sparse_predict_targets(s.handle, None, 1, 1, P(big), P(out)), "cugp_sparse_predict_targets")
    assert refused(L.cugp_sparse_predict_targets(s.handle, P(out), 1, 1, None, P(out)), "cugp_sparse_predict_targets")
    for budget in (0, -1):
        assert refused(L.cugp_sparse_cg_solve_targets(s.handle, budget, 0, None, 0, C.byref(ne)), "cugp_sparse_cg_solve_targets")
    nodata, _ = make(gp_mod, name, data=False)
    assert refused(L.cugp_sparse_set_targets(nodata.handle, P(big), 3), "cugp_sparse_set_targets")
    notargets, _ = make(gp_mod, name)
    noz, _ = make(gp_mod, name, inducing=False)
    noz.set_targets(tst.targets(name, 3).T)
    p = C.c_int(7)
    assert L.cugp_sparse_num_targets(notargets.handle, C.byref(p)) == capi.CUGP_OK and p.value == 0
    for e in (notargets, noz, nodata):
        assert refused(L.cugp_sparse_bound_targets(e.handle, C.byref(F), None), "cugp_sparse_bound_targets")
        assert refused(L.cugp_sparse_bound_grad_targets(e.handle, C.byref(F), P(out), 3, None), "cugp_sparse_bound_grad_targets")
        assert refused(L.cugp_sparse_bound_grad_z_targets(e.handle, C.byref(F), P(out), 3, P(big), None),
                       "cugp_sparse_bound_grad_z_targets")
        assert refused(L.cugp_sparse_predict_targets(e.handle, P(out), 1, 1, P(big), P(out)), "cugp_sparse_predict_targets")
        assert refused(L.cugp_sparse_cg_solve_targets(e.handle, 5, 0, None, 0, C.byref(ne)), "cugp_sparse_cg_solve_targets")
    assert (F.value, ne.value) == (7.0, 7) and not out.any() and not big.any()
    # the refusals left the handles usable; var may be NULL
    assert np.isfinite(s.bound_targets()[0])
    m = np.empty((3, ts.NT))
    capi.check(L.cugp_sparse_predict_targets(s.handle, P(Xt), ts.NT, 1, P(m), None))
    assert same_bits([m], [s.predict_targets(Xt)[0]])
    notargets.set_targets(tst.targets(name, 3).T)
    assert same_bits([notargets.bound_targets()[0]], [s.bound_targets()[0]])
    for e in (s, nodata, notargets, noz):
        e.close()


# ------------------------------------------------------------------ 10. not positive definite
def test_not_positive_definite_gives_nan_with_ok(gp_mod):
    """Duplicated inducing inputs under a jitter of 1e-300: Kuu is singular to rounding, and its factorisation fails or
    leaves a B that is not positive definite -- NaN results with CUGP_OK, as the single-target calls give."""
    name, p = "se_n300_m65", 3
    family, N, M, d = ts.CASES[name][:4]
    X, y, Z, Xt, cov, chunk = ts.inputs(name)
    s = gp_mod.SparseGP(N, M, d, jitter=1e-300, chunk_rows=chunk)
    s.set_data(X, y)
    Zd = Z.copy()
    Zd[1::2] = Zd[0:-1:2][: len(Zd[1::2])]
    s.set_inducing(Zd)
    s.set_loghyperparam(cov.hp)
    s.set_targets(tst.targets(name, p).T)
    assert np.isnan(s.bound())
    F, g, gZ, each = s.bound_grad_z_targets()
    m, v = s.predict_targets(Xt)
    assert np.isnan(F) and np.all(np.isnan(g)) and np.all(np.isnan(gZ)) and np.all(np.isnan(each)) and each.shape == (p,)
    assert np.all(np.isnan(m)) and np.all(np.isnan(v)) and m.shape == (p, ts.NT)
    # the handle's own y at the same theta: one rule for both sides, nothing is copied out of a failed evaluation
    F1, g1 = s.bound_grad()
    Fz, gz1, gZ1 = s.bound_grad_z()
    m1, v1 = s.predict(Xt)
    assert np.isnan(F1) and np.all(np.isnan(g1)) and g1.shape == (len(cov.hp),)
    assert np.isnan(Fz) and np.all(np.isnan(gz1)) and np.all(np.isnan(gZ1)) and gZ1.shape == Z.shape
    assert np.all(np.isnan(m1)) and np.all(np.isnan(v1)) and m1.shape == (ts.NT,) and v1.shape == (ts.NT,)
    s.set_inducing(Z)                                        # a usable handle afterwards
    s2, _ = make(gp_mod, name, p)
    s2.close()
    s.close()
