"""GPU tests of the sparse model's prediction beyond one 128-row test tile and beyond one pass (cugp_sparse_predict,
cugp_sparse_predict_plan; SparseGP.predict / predict_plan).

tests/test_gpu_sparse.py predicts at 20 points: one test tile, rows below 128 of k_sparse_predict_finish, one pass.  Here:

  two and three test tiles   129, 200 and 257 points (truth_sparse.wide_case: truth.wide_points of the case's data, the last
                             but one a training row, row 128 -- the first of the second tile -- the inducing input Z[0]) on
                             four models: the default chunk with the odd split (se 800 / 65), mpad 384 (se 1300 / 260),
                             Matern-3/2-ARD over two passes of the data (1000 / 130), three feature chunks (ard 300 / 65 / 33)
  two passes                 nt = P + 129 on se 300 / 16 / 3, P = cugp_sparse_predict_plan's first pass (349440 rows at mpad
                             128): the second pass reads its test points, and writes its means and variances, at an offset

Mean, variance and latent variance are held to

    err_gpu(q) <= F_SPARSE[family] * max(yardstick(q), 4 ulp of q's scale)

against truth_sparse.Truth.predict in longdouble at the same points -- ALL rows of the two-pass call --; the yardstick is
truth_sparse.computed_form there over the data as given and truth.permutations, the floors are truth_sparse.case's, the
factors were fixed on the CPU (tests/test_truth_sparse_cpu.py, docs/ACCURACY.md), never from the GPU.  Every figure is
printed before it is asserted (run with -s).  One process, one device; nothing outside the tree is read.
"""
import numpy as np
import pytest

import truth
import truth_sparse as ts
from accuracy import Report

pytestmark = pytest.mark.gpu
extended = pytest.mark.skipif(not truth.EXTENDED, reason="numpy.longdouble is not an extended-precision type here")


@pytest.fixture(scope="module")
def gp_mod():
    import cugp_amd.gp as gp
    return gp


def make(gp_mod, name):
    """A SparseGP of the case with its hyper-parameters, data and inducing inputs set -> (handle, inputs)."""
    family, N, M, d = ts.CASES[name][:4]
    X, y, Z, Xt, cov, chunk = ts.inputs(name)
    s = gp_mod.SparseGP(N, M, d, kernel=family if family.startswith("matern") else "se", ard=family == "ard",
                        jitter=ts.JITTER, chunk_rows=chunk)
    s.set_data(X, y)
    s.set_inducing(Z)
    s.set_loghyperparam(cov.hp)
    return s, (X, y, Z, Xt, cov)


def same_bits(a, b):
    def bits(arrays):
        return [np.ascontiguousarray(x, dtype=np.float64).view(np.uint64) for x in arrays]
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(bits(a), bits(b)))


def both(s, Xt):
    """(mean, var with noise, latent mean, latent var) of a handle at Xt."""
    return s.predict(Xt) + s.predict(Xt, with_noise=False)


# ------------------------------------------------------------------ 1. two and three test tiles
@extended
@pytest.mark.parametrize("nt", ts.WIDE_NTS)
@pytest.mark.parametrize("name", ts.WIDE_NAMES)
def test_accuracy_beyond_one_tile(gp_mod, name, nt):
    c, w = ts.case(name), ts.wide_case(name, nt)
    s, (X, y, Z, _, cov) = make(gp_mod, name)
    assert s.predict_plan(nt) == [(0, nt)] and -(-nt // 128) in (2, 3) and w["Xt"].shape == (nt, X.shape[1])
    m, v, ml, vl = both(s, w["Xt"])
    assert m.shape == v.shape == vl.shape == (nt,)
    rep = Report("sparse-wide/%s/nt%d" % (name, nt), cov)
    ts.hold_wide(rep, c, w, m, v, latent_var=vl)
    assert same_bits([ml], [m])                                 # the latent mean has the noisy mean's bits
    assert same_bits(both(s, w["Xt"]), (m, v, ml, vl))          # a second call: the same bits
    s.close()
    rep.check()


# ------------------------------------------------------------------ 2. the scratch shrinks logically
@pytest.mark.parametrize("name", ts.WIDE_NAMES)
def test_a_smaller_prediction_after_a_larger_one(gp_mod, name):
    """257 points and then 129 on the same handle -- the scratch stays at its size, its partition moves -- give the bits of
    a fresh handle."""
    big, small = ts.wide_points(name, 257), ts.wide_points(name, 129)
    s, _ = make(gp_mod, name)
    both(s, big)
    got = both(s, small)
    fresh, _ = make(gp_mod, name)
    assert same_bits(got, both(fresh, small))
    s.close()
    fresh.close()


# ------------------------------------------------------------------ 3. two passes
@extended
def test_two_passes(gp_mod):
    """nt = P + 129: two passes, the second of two test tiles.  Xt[P], the first row of the second pass, is Z[0]; Xt[P - 1],
    the last of the first, a data row.  Every one of the nt means and variances is held to the bound.

    The rows [P - 128, nt) predicted alone lie in the first pass of their call, at the same positions inside their tiles
    (P - 128 is a multiple of 128).  Their bits are those of the long call, and that is asserted, because it follows from
    the kernels: k_cross computes an entry from its own test row and inducing input, k_predict_gemm an output tile from the
    test tile's rows and the factor's rows over a k range that ends at the factor tile's diagonal -- neither the tile's index
    nor the number of test tiles enters --, and k_sparse_predict_finish gives a row to a wave whatever its index."""
    name = ts.TWO_PASS_NAME
    c = ts.case(name)
    s, (X, y, Z, _, cov) = make(gp_mod, name)
    P = gp_mod.sparse_predict_plan(s.m, 1 << 30)[0][1]
    nt = P + 129
    assert P == 349440 and s.predict_plan(nt) == [(0, P), (P, 129)]
    w = ts.wide_case(name, nt, z_row=P, data_row=P - 1)
    Xt = w["Xt"]
    assert np.array_equal(Xt[P], Z[0]) and np.any(np.all(X == Xt[P - 1], axis=1))
    m, v, ml, vl = both(s, Xt)
    assert m.shape == v.shape == (nt,)
    rep = Report("sparse-wide/%s/nt%d" % (name, nt), cov)
    ts.hold_wide(rep, c, w, m, v, latent_var=vl)
    for tag, rows in (("pass1/", slice(0, P)), ("pass2/", slice(P, nt))):       # (which pass a miss would lie in)
        part = dict(w, tm=w["tm"][rows], tv=w["tv"][rows])
        ts.hold_wide(rep, c, part, m[rows], v[rows], tag=tag)
    assert same_bits([ml], [m])
    tail = slice(P - 128, nt)
    assert s.predict_plan(nt - (P - 128)) == [(0, 257)]
    mt, vt = s.predict(np.ascontiguousarray(Xt[tail]))
    same = same_bits((mt, vt), (m[tail], v[tail]))
    print("TWO-PASS rows [P - 128, nt) alone against the long call: %s" % ("same bits" if same else "DIFFERENT bits"))
    part = dict(w, tm=w["tm"][tail], tv=w["tv"][tail])
    ts.hold_wide(rep, c, part, mt, vt, tag="tail-alone/")
    s.close()                                                   # (about 1.1 GiB of device scratch until here)
    rep.check()
    assert same
