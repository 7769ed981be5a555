"""GPU tests of the gradient of the sparse model's bound with respect to the inducing inputs (cugp_sparse_bound_grad_z,
cugp_sparse_get_inducing, cugp_sparse_cg_solve_z; SparseGP.bound_grad_z / get_inducing / cg_solve(inducing=True)).

Accuracy is held to fp64 rounding against the extended-precision truth of tests/truth_sparse_z.py:

    err_gpu(gZ) <= F_SPARSE_Z[family] * max(yardstick, 4 ulp)

with err the largest |gZ - truth| over all m d entries relative to max|truth gZ|; the yardstick is truth_sparse's computed
form in fp64 numpy / LAPACK over the data as given and truth.permutations; F_SPARSE_Z was fixed on the CPU
(tests/test_truth_sparse_z_cpu.py, docs/ACCURACY.md), never from the GPU.  Every figure is printed before it is asserted
("ACC <case> gZ err noise floor ratio"; run with -s).  One process, one device; nothing outside the tree is read.

What the cases reach (truth_sparse_z.CASES): no padding anywhere and two chunks; a ragged last chunk with mp padding beyond
column 65; several row tiles per workgroup range with four column tiles; Matern 3/2; Matern 5/2; two feature chunks
(d = 17); Matern-ARD; the default chunk (chunk_rows 0) with one 896-row pass in row ranges of 5, 5 and 4 tiles, on SE and
on Matern 5/2; Matern-3/2-ARD over two passes and two column tiles, and on 257 rows; mpad 384 with one 1408-row pass in
ranges of 5, 5, 5, 5 and 2 tiles and six column tiles; d = 32, an exact multiple of the feature chunk; d = 33, three feature
chunks with the last of one feature; M = 16.
"""
import ctypes as C

import numpy as np
import pytest

import truth
import truth_sparse_z as tz
from accuracy import Report
from cugp_amd import capi

pytestmark = pytest.mark.gpu
extended = pytest.mark.skipif(not truth.EXTENDED, reason="numpy.longdouble is not an extended-precision type here")

NAMES = list(tz.CASES)
_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int)


@pytest.fixture(scope="module")
def gp_mod():
    import cugp_amd.gp as gp
    return gp


def make(gp_mod, name, chunk_rows=None, hp=None, data=True, inducing=True):
    """A SparseGP of the case with its hyper-parameters, data and inducing inputs set -> (handle, inputs)."""
    family, N, M, d = tz.CASES[name][:4]
    X, y, Z, cov, chunk = tz.inputs(name)
    kernel = family if family.startswith("matern") else "se"
    s = gp_mod.SparseGP(N, M, d, kernel=kernel, ard=family == "ard", jitter=tz.JITTER,
                        chunk_rows=chunk if chunk_rows is None else chunk_rows)
    if data:
        s.set_data(X, y)
    if inducing:
        s.set_inducing(Z)
    s.set_loghyperparam(cov.hp if hp is None else hp)
    return s, (X, y, Z, cov)


def bits(*arrays):
    return [np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).copy() for a in arrays]


def same_bits(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(bits(*a), bits(*b)))


def all_three(s):
    F, g, gZ = s.bound_grad_z()
    return np.float64(F), g, gZ


# ------------------------------------------------------------------ 1. accuracy
@extended
@pytest.mark.parametrize("name", NAMES)
def test_accuracy(gp_mod, name):
    c = tz.case(name)
    s, (X, y, Z, cov) = make(gp_mod, name)
    F, g, gZ = all_three(s)
    assert gZ.shape == Z.shape and g.shape == (len(cov.hp),) and np.all(np.isfinite(gZ))
    rep = Report("sparse-z/" + name, cov)
    tz.hold(rep, c, gZ)
    s.close()
    rep.check()


# ------------------------------------------------------------------ 2. F and g carry bound_grad's bits
@pytest.mark.parametrize("name", ["se_n300_m65_d3", "se_n1300_m200", "ard_n300_m130_d17", "matern32_n300_m65",
                                  "se_n800_m65_d3_c0", "se_n1300_m260_c0"])
def test_bound_and_hyper_gradient_keep_their_bits(gp_mod, name):
    s, _ = make(gp_mod, name)
    twin, _ = make(gp_mod, name)
    F, g, gZ = all_three(s)
    F2, g2 = twin.bound_grad()
    assert same_bits([F, g], [np.float64(F2), g2])
    # the results are kept: the plain calls on the same handle answer with the same bits, and a Z gradient on top of a
    # plain gradient evaluates again to the same
    F3, g3 = s.bound_grad()
    assert same_bits([F, g], [np.float64(F3), g3]) and same_bits([s.bound()], [F])
    assert same_bits(all_three(twin), [F, g, gZ])
    s.close()
    twin.close()


# ------------------------------------------------------------------ 3. determinism
@pytest.mark.parametrize("name", ["se_n1300_m200", "ard_n300_m130_d17", "se_n800_m65_d3_c0", "se_n1300_m260_c0"])
def test_bit_identical_on_repeat_second_handle_and_after_a_detour(gp_mod, name):
    s, (X, y, Z, cov) = make(gp_mod, name)
    first = all_three(s)
    s.set_data(X, y)                                            # the same data again: launched again, the same bits
    assert same_bits(all_three(s), first)
    s.set_loghyperparam(np.asarray(cov.hp) + 0.25)              # a detour: other hyper-parameters and another Z
    s.set_inducing(Z[::-1] + 0.125)
    away = all_three(s)
    assert not same_bits(away[2:], first[2:]) and np.all(np.isfinite(away[2]))
    s.set_loghyperparam(cov.hp)
    s.set_inducing(Z)
    assert same_bits(all_three(s), first)
    twin, _ = make(gp_mod, name)
    assert same_bits(all_three(twin), first)
    s.close()
    twin.close()


# ------------------------------------------------------------------ 4. chunk size, to the bound
@extended
def test_chunk_rows_128_against_256(gp_mod):
    name = "se_n300_m65_d3"
    c = tz.case(name)
    for chunk in (128, 256):
        s, (X, y, Z, cov) = make(gp_mod, name, chunk_rows=chunk)
        assert [p[1] for p in s.plan()] == ([128, 128, 44] if chunk == 128 else [256, 44])
        rep = Report("sparse-z/%s/chunk%d" % (name, chunk), cov)
        tz.hold(rep, c, s.bound_grad_z()[2])
        rep.check()
        s.close()


@extended
def test_chunk_rows_at_the_ragged_ranges(gp_mod):
    """The default chunk (0) and 896 give the same plan -- one 896-row pass, row ranges of 5, 5 and 4 tiles -- and so the
    same bits; 512 and 128 give other partial sums: each is held to the bound."""
    name = "se_n800_m65_d3_c0"
    c = tz.case(name)
    rows = {0: [800], 896: [800], 512: [512, 288], 128: [128] * 6 + [32]}
    outs = {}
    for chunk in (0, 896, 512, 128):
        s, (X, y, Z, cov) = make(gp_mod, name, chunk_rows=chunk)
        if chunk in (0, 896):
            assert s.plan() == [(0, 800, 896, 3, 304)]
        assert [p[1] for p in s.plan()] == rows[chunk]
        outs[chunk] = all_three(s)
        rep = Report("sparse-z/%s/chunk%d" % (name, chunk), cov)
        tz.hold(rep, c, outs[chunk][2])
        rep.check()
        s.close()
    assert same_bits(outs[0], outs[896])


# ------------------------------------------------------------------ 5. nothing beyond m d doubles is written
@pytest.mark.parametrize("name", ["se_n300_m65_d3", "ard_n300_m130_d17", "se_n800_m65_d3_c0"])
def test_guard_band_stays_intact(gp_mod, name):
    s, (X, y, Z, cov) = make(gp_mod, name)
    want = s.bound_grad_z()[2]
    md, guard = Z.size, 256
    buf, g, F = np.full(md + guard, 7.0), np.full(len(cov.hp) + guard, 7.0), C.c_double()
    s.set_inducing(Z)                                           # (stale: the call below evaluates)
    capi.check(capi.lib().cugp_sparse_bound_grad_z(s.handle, C.byref(F), capi.ptr(g), len(cov.hp), capi.ptr(buf)))
    assert same_bits([buf[:md]], [want.ravel()]) and np.all(buf[md:] == 7.0) and np.all(g[len(cov.hp):] == 7.0)
    zb = np.full(md + guard, 7.0)
    capi.check(capi.lib().cugp_sparse_get_inducing(s.handle, capi.ptr(zb)))
    assert same_bits([zb[:md]], [Z.ravel()]) and np.all(zb[md:] == 7.0)
    s.close()


# ------------------------------------------------------------------ 6. staleness
def test_bound_grad_z_after_set_inducing_re_evaluates(gp_mod):
    name = "matern52_n300_m65_d3"
    s, (X, y, Z, cov) = make(gp_mod, name)
    old = all_three(s)
    Z2 = np.ascontiguousarray(Z + 0.0625 * np.cos(np.arange(Z.size)).reshape(Z.shape))
    fresh, _ = make(gp_mod, name)
    fresh.set_inducing(Z2)
    want = all_three(fresh)
    s.set_inducing(Z2)
    got = all_three(s)
    assert same_bits(got, want) and not same_bits(got[2:], old[2:]) and same_bits([s.get_inducing()], [Z2])
    s.set_loghyperparam(np.asarray(cov.hp) - 0.2)               # and after new hyper-parameters
    fresh.set_loghyperparam(np.asarray(cov.hp) - 0.2)
    assert same_bits(all_three(s), all_three(fresh))
    s.close()
    fresh.close()


# ------------------------------------------------------------------ 7. the optimiser over [theta, vec Z]
def test_cg_solve_inducing(gp_mod):
    """f never rises along the trace and ends below its start; bound() afterwards has the last row's bits; Z moved; and
    theta, Z and the trace are, bit for bit, those of cugp_cg_minimize_n_iterates driven from here with bound_grad_z as
    the objective on a second handle."""
    name, budget = "se_n300_m65_d3", 15
    s, (X, y, Z, cov) = make(gp_mod, name)
    nh, md = len(cov.hp), Z.size
    F0 = s.bound()
    tr = s.cg_solve(budget=budget, inducing=True)
    f = tr[:, -1]
    print("CG-SPARSE-Z objective along the trace:", " ".join("%.6f" % v for v in f))
    assert tr.shape[1] == nh + 1 and tr.shape[0] >= 2 and np.all(np.isfinite(tr))
    assert np.array_equal(tr[0, :-1], np.asarray(cov.hp)) and same_bits([tr[0, -1]], [-F0])
    assert np.all(f[1:] <= f[:-1]) and f[-1] < f[0], f
    end, Zend = s.get_loghyperparam(), s.get_inducing()
    assert np.array_equal(tr[-1, :-1], end) and same_bits([-s.bound()], [f[-1]])
    assert not np.array_equal(Zend, Z) and np.all(np.isfinite(Zend))

    twin, _ = make(gp_mod, name)
    L = capi.lib()
    fn = L.cugp_cg_minimize_n_iterates
    fn.restype = C.c_int
    fn.argtypes = [capi.OBJECTIVE_N, C.c_void_p, _dp, C.c_int, C.c_int, _dp, C.c_int, _ip, _ip]

    @capi.OBJECTIVE_N
    def objective(_ctx, v, nv, fo, go):
        vec = np.array([v[i] for i in range(nv)])
        twin.set_loghyperparam(vec[:nh])
        twin.set_inducing(vec[nh:].reshape(Z.shape))
        F, g, gZ = twin.bound_grad_z()
        fo[0] = -F
        for i, val in enumerate(np.concatenate([g, gZ.ravel()])):
            go[i] = val
    v = np.concatenate([np.asarray(cov.hp, dtype=np.float64), Z.ravel()])
    rows, ne, nr = np.full((4 * budget + 8, nh + md + 1), np.nan), C.c_int(), C.c_int()
    assert fn(objective, None, capi.ptr(v), nh + md, budget, capi.ptr(rows), rows.shape[0], C.byref(ne), C.byref(nr)) == 0
    k = nr.value
    assert k == tr.shape[0]
    assert same_bits([rows[:k, :nh], rows[:k, -1]], [tr[:, :nh], tr[:, -1]])
    assert same_bits([v[:nh], v[nh:]], [end, Zend.ravel()])
    # the raw call: the row behind the last is NaN and nothing beyond is written
    s.set_loghyperparam(cov.hp)
    s.set_inducing(Z)
    raw, ne2 = np.full((4 * budget + 8, nh + 1), 7.0), C.c_int()
    capi.check(L.cugp_sparse_cg_solve_z(s.handle, budget, capi.ptr(raw), raw.shape[0], C.byref(ne2)))
    assert ne2.value == ne.value <= budget + 1
    assert same_bits([raw[:k]], [tr]) and np.all(np.isnan(raw[k])) and np.all(raw[k + 1:] == 7.0)
    assert same_bits([s.get_inducing()], [Zend])
    s.close()
    twin.close()


# ------------------------------------------------------------------ 8. the existing results of other handles
def test_other_handles_before_and_after(gp_mod):
    X, y, Xt, cov = truth.family_inputs("se", "n257_d3")

    def existing():
        g = gp_mod.Covsum(X.shape[0], X.shape[1])
        g.set_loghyperparam(cov.hp)
        ll, gr = g.loglik_grad(X, y)
        m, v = g.compute_test_means_and_variances(X, y, Xt)
        g.close()
        p, _ = make(gp_mod, "se_n1300_m200")
        F, gs = p.bound_grad()
        p.close()
        return np.float64(ll), gr, m, v, np.float64(F), gs
    before = existing()
    s, _ = make(gp_mod, "se_n1300_m200")
    all_three(s)
    s.cg_solve(budget=2, inducing=True)
    during = existing()                                         # the handle that took the Z gradient still alive
    s.close()
    assert same_bits(during, before) and same_bits(existing(), before)


# ------------------------------------------------------------------ 9. refusals, on the device
def test_refusals(gp_mod):
    L = capi.lib()
    name = "se_n300_m65_d3"
    s, (X, y, Z, cov) = make(gp_mod, name)
    a, _ = make(gp_mod, "matern52_ard_n257_m64")
    out, F, ne = np.zeros(400), C.c_double(7.0), C.c_int(7)

    def refused(rc, call):
        return rc == capi.CUGP_ERR_INVALID and call.encode() in L.cugp_last_error()
    p = capi.ptr(out)
    assert refused(L.cugp_sparse_bound_grad_z(s.handle, C.byref(F), p, 4, p), "cugp_sparse_bound_grad_z")      # isotropic: 3
    assert refused(L.cugp_sparse_bound_grad_z(a.handle, C.byref(F), p, 3, p), "cugp_sparse_bound_grad_z")      # this ARD handle: 5
    assert refused(L.cugp_sparse_bound_grad_z(s.handle, None, p, 3, p), "cugp_sparse_bound_grad_z")
    assert refused(L.cugp_sparse_bound_grad_z(s.handle, C.byref(F), None, 3, p), "cugp_sparse_bound_grad_z")
    assert refused(L.cugp_sparse_bound_grad_z(s.handle, C.byref(F), p, 3, None), "cugp_sparse_bound_grad_z")
    assert refused(L.cugp_sparse_get_inducing(s.handle, None), "cugp_sparse_get_inducing")
    for budget in (0, -1):
        assert refused(L.cugp_sparse_cg_solve_z(s.handle, budget, None, 0, C.byref(ne)), "cugp_sparse_cg_solve_z")
    nodata, _ = make(gp_mod, name, data=False)
    noz, _ = make(gp_mod, name, inducing=False)
    for e in (nodata, noz):
        assert refused(L.cugp_sparse_bound_grad_z(e.handle, C.byref(F), p, 3, p), "cugp_sparse_bound_grad_z")
        assert refused(L.cugp_sparse_cg_solve_z(e.handle, 5, None, 0, C.byref(ne)), "cugp_sparse_cg_solve_z")
    assert refused(L.cugp_sparse_get_inducing(noz.handle, p), "cugp_sparse_get_inducing")
    assert (F.value, ne.value) == (7.0, 7) and not out.any()
    # the refusals left the handles usable
    assert np.all(np.isfinite(s.bound_grad_z()[2])) and a.bound_grad_z()[2].shape == (64, 3)
    nodata.set_data(X, y)
    assert same_bits(all_three(nodata), all_three(s))
    for e in (s, a, nodata, noz):
        e.close()
