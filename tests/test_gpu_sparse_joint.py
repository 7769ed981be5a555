"""GPU tests of the sparse model's joint predictive covariance, posterior draws and input gradients
(cugp_sparse_predict_cov, _sample, _grad, _cov_plan; SparseGP.predict_joint / sample_posterior / predict_grad /
predict_cov_plan).

The latent and the noisy covariance, dmean and dvar are held to

    err_gpu(q) <= factor(family) * max(yardstick(q), 4 ulp of q's scale)

against tests/truth_sparse_joint.py's longdouble truth; the yardstick is the fp64 computed form over the data as given and
truth.permutations, the factor was fixed on the CPU (tests/test_truth_sparse_joint_cpu.py, docs/ACCURACY.md), never from
the GPU.  The draws and their factor are held to the derived bounds of tests/test_gpu_predict_wide.py (truth.factor_bound_worst,
truth.draw_bound_worst): no measured tolerance.  Everything else is an identity in bits.  Every figure is printed before it
is asserted (run with -s).  One process, one device; nothing outside the tree is read.
"""
import ctypes as C

import numpy as np
import pytest

import truth
import truth_sparse as ts
import truth_sparse_joint as tj
from accuracy import Report
from cugp_amd import capi

pytestmark = pytest.mark.gpu
extended = pytest.mark.skipif(not truth.EXTENDED, reason="numpy.longdouble is not an extended-precision type here")
LD = truth.LD
TUNE_COV_SPLIT, COV_SPLIT_DEFAULT = 20, 1024      # kernels.h TUNE_COV_SPLIT and its built-in default (kernels.hip: g_tune_init)
IDS = ["%s-%s" % (n, "nt%d" % nt if nt else "own") for n, nt in tj.ALL_CASES]


@pytest.fixture(scope="module")
def gp_mod():
    import cugp_amd.gp as gp
    return gp


def make(gp_mod, name, hp=None, Z=None, jitter=ts.JITTER):
    """A SparseGP of the case with its hyper-parameters, data and inducing inputs set -> (handle, inputs)."""
    family, N, M, d = tj.case_row(name)[:4]
    X, y, Z0, Xt, cov, chunk = tj.inputs(name)
    s = gp_mod.SparseGP(N, M, d, kernel=family if family.startswith("matern") else "se", ard=family == "ard",
                        jitter=jitter, chunk_rows=chunk)
    s.set_data(X, y)
    s.set_inducing(Z0 if Z is None else Z)
    s.set_loghyperparam(cov.hp if hp is None else hp)
    return s, (X, y, Z0, Xt, cov)


def same_bits(a, b):
    def bits(arrays):
        return [np.ascontiguousarray(x, dtype=np.float64).view(np.uint64) for x in arrays]
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(bits(a), bits(b)))


def everything(s, Xt, ns=3):
    """Every output of the three calls at Xt, noisy and latent, as one tuple of arrays (draws from fixed normals)."""
    z = np.random.default_rng(len(Xt)).standard_normal((ns, len(Xt)))
    out = ()
    for noise in (True, False):
        out += s.predict_joint(Xt, with_noise=noise) + s.predict_grad(Xt, with_noise=noise)
        out += (s.sample_posterior(Xt, ns, with_noise=noise, normals=z),)
    return out


# ------------------------------------------------------------------ 1. accuracy
@extended
@pytest.mark.parametrize("name, nt", tj.ALL_CASES, ids=IDS)
def test_accuracy(gp_mod, name, nt):
    c = tj.case(name, nt)
    s, (X, y, Z, _, cov) = make(gp_mod, name)
    Xt = c["Xt"]
    _, cov_n = s.predict_joint(Xt)
    _, cov_l = s.predict_joint(Xt, with_noise=False)
    _, _, dm, dv = s.predict_grad(Xt)
    s.close()
    assert cov_n.shape == cov_l.shape == (len(Xt),) * 2 and dm.shape == dv.shape == Xt.shape
    rep = Report("sparse-joint/%s/nt%d" % (name, len(Xt)), cov)
    tj.hold(rep, c, cov_l, dm, dv, cov_noise=cov_n)
    rep.check()


# ------------------------------------------------------------------ 2. the forms of the product launch
@extended
@pytest.mark.parametrize("nt", [129, 257])
@pytest.mark.parametrize("name", [tj.SPLIT_NAME, "se_n1300_m260_c0"])
def test_forms(gp_mod, name, nt):
    """Tuning key 20 (process-wide: the model's inner handle has no keys of its own): 0 -- 128 x 128 tiles, no split --,
    the smallest value that gives 64 x 64 tiles (4 per lower 128-tile: no split yet), and the built-in default (at mpad
    512 the k range in 2; mpad 384 is below two chunks of 256 and never splits).  predict_cov_plan reports the form, every
    form is within the bound, repeats its bits and has them on a second handle; where the split differs the bits do."""
    c = tj.case(name, nt)
    Xt, m = c["Xt"], len(c["Z"])
    t128 = (-(-nt // 128)) * (-(-nt // 128) + 1) // 2
    rep = Report("sparse-joint-forms/%s/nt%d" % (name, nt), c["cov"])
    F = tj.factor(c["family"])
    got = {}
    try:
        for v in (0, 4 * t128, COV_SPLIT_DEFAULT):
            capi.check(capi.lib().cugp_set_tuning(TUNE_COV_SPLIT, v))
            s, _ = make(gp_mod, name)
            plan = s.predict_cov_plan(nt)
            assert plan == tj.cov_plan(m, nt) and plan[0] == -(-nt // 128) * 128
            cov = s.predict_joint(Xt, with_noise=False)[1]
            assert same_bits([cov], [s.predict_joint(Xt, with_noise=False)[1]]), (v, "repeat")
            s2, _ = make(gp_mod, name)
            assert same_bits([cov], [s2.predict_joint(Xt, with_noise=False)[1]]), (v, "second handle")
            s.close()
            s2.close()
            err = float(np.max(np.abs(cov.astype(LD) - c["tc"])))
            rep.add("cov/key%d/edge%d/split%d" % (v, plan[1], plan[2]), err, c["noise"]["cov"], c["floor"]["cov"], F)
            got[v] = (plan, cov)
    finally:
        capi.check(capi.lib().cugp_set_tuning(TUNE_COV_SPLIT, COV_SPLIT_DEFAULT))
    assert got[0][0][1:3] == (128, 1) and got[4 * t128][0][1:3] == (64, 1)
    want_split = 2 if name == tj.SPLIT_NAME else 1
    assert got[COV_SPLIT_DEFAULT][0][1:3] == (64, want_split)
    if want_split == 2:                                   # another order of summation: the form that ran is the plan's
        assert got[COV_SPLIT_DEFAULT][0][3] == 256
        assert not same_bits([got[COV_SPLIT_DEFAULT][1]], [got[4 * t128][1]])
    rep.check()


# ------------------------------------------------------------------ 3. identities
@extended
@pytest.mark.parametrize("name, nt", [("se_n800_m65_d3_c0", 257), ("matern52_n800_m65_d3_c0", None)])
def test_identities(gp_mod, name, nt):
    """Both cases have sf2 = s2 = e (conftest.HP_DEFAULT), where the diagonal identity is derived, not measured: the finish
    rounds a = fl(k_tt + s2) once (|error| <= half an ulp of sf2 + s2 < 8, that is at most one ulp of an entry >= s2 > 2),
    then fl(a - p) and fl(k_tt - p) round to half an ulp of the entry each: at most 2 ulp in all, within the 4 stated."""
    c = tj.case(name, nt)
    s, (X, y, Z, _, cov) = make(gp_mod, name)
    Xt, n = c["Xt"], len(c["Xt"])
    s2 = float(cov.fp64().sn2)
    m, v = s.predict(Xt)
    ml, vl = s.predict(Xt, with_noise=False)
    mj, cov_n = s.predict_joint(Xt)
    mjl, cov_l = s.predict_joint(Xt, with_noise=False)
    mg, vg, dm, dv = s.predict_grad(Xt)
    mgl, vgl, dml, dvl = s.predict_grad(Xt, with_noise=False)
    mo, vo, dmo, none = s.predict_grad(Xt, want_var_grad=False)
    assert same_bits((mj, mjl, mg, mgl, mo), (m,) * 5), "the mean's bits are cugp_sparse_predict's"
    assert same_bits((vg, vo, vgl), (v, v, vl)), "the variance's bits are cugp_sparse_predict's"
    assert np.array_equal(cov_n, cov_n.T) and np.array_equal(cov_l, cov_l.T), "exactly symmetric"
    off = ~np.eye(n, dtype=bool)
    assert same_bits([cov_n[off]], [cov_l[off]]), "noise moved an off-diagonal entry"
    dn, dl = np.diag(cov_n), np.diag(cov_l)
    ulps = float(np.max(np.abs(dn.astype(LD) - (dl.astype(LD) + LD(s2))) / np.spacing(dn)))
    print("IDENT %-26s nt %-4d |diag noisy - (diag latent + s2)| <= %.2f ulp of the entry" % (name, n, ulps))
    assert ulps <= 4
    rep = Report("sparse-joint-ident/%s/nt%d" % (name, n), cov)
    F = tj.factor(c["family"])
    rep.add("diag(cov)-var", float(np.max(np.abs(dn.astype(LD) - v.astype(LD)))), c["noise"]["cov"], c["floor"]["cov"], F)
    rep.add("diag(cov_f)-var_f", float(np.max(np.abs(dl.astype(LD) - vl.astype(LD)))), c["noise"]["cov"], c["floor"]["cov"], F)
    assert same_bits((dml, dvl), (dm, dv)), "the gradients depend on with_noise"
    assert none is None and same_bits([dmo], [dm]), "want_var_grad=False moved dmean"
    s.close()
    rep.check()


# ------------------------------------------------------------------ 4. a row's gradient does not depend on nt
@pytest.mark.parametrize("name", ["se_n800_m65_d3_c0", "matern32_ard_n1000_m130"])
def test_row_independence(gp_mod, name):
    Xt = tj.wide_points(name, 257)
    s, _ = make(gp_mod, name)
    whole = s.predict_grad(Xt)
    for t in (0, 63, 64, 128, 255, 256):                 # both halves of a tile, Z[0], a data row, the one row of the third tile
        alone = s.predict_grad(np.ascontiguousarray(Xt[t: t + 1]))
        assert same_bits(alone, [w[t: t + 1] for w in whole]), t
    s.close()


# ------------------------------------------------------------------ 5. two passes
@extended
def test_two_passes(gp_mod):
    """predict_grad at P + 129 points, P = cugp_sparse_predict_plan's first pass at mpad 128: the second pass reads its test
    points and writes its rows at an offset.  Xt[P] is Z[0], Xt[P - 1] a data row.  Every row is held to the bound; mean and
    variance carry predict's bits there too."""
    name = ts.TWO_PASS_NAME
    s, (X, y, Z, _, cov) = make(gp_mod, name)
    P = gp_mod.sparse_predict_plan(s.m, 1 << 30)[0][1]
    nt = P + 129
    assert P == 349440 and s.predict_plan(nt) == [(0, P), (P, 129)]
    Xt = ts.wide_points(name, nt, z_row=P, data_row=P - 1)
    c = tj.grad_case(name, Xt, "two_pass")
    m, v, dm, dv = s.predict_grad(Xt)
    mo, vo, dmo, _ = s.predict_grad(Xt, with_noise=False, want_var_grad=False)
    mp, vp = s.predict(Xt)
    _, vpl = s.predict(Xt, with_noise=False)
    s.close()
    rep = Report("sparse-joint/%s/nt%d" % (name, nt), cov)
    for tag, rows in (("", slice(None)), ("pass1/", slice(0, P)), ("pass2/", slice(P, nt))):
        tj.hold_grad(rep, c, dm, dv, rows, tag)
    assert same_bits((m, v, mo, vo), (mp, vp, mp, vpl)) and same_bits([dmo], [dm])
    rep.check()


# ------------------------------------------------------------------ 6. draws
NS = (7, 129, 257)                     # one, two and three 128-row tiles of normals


def normals(nt, ns):
    return np.random.default_rng(1000 * nt + ns).standard_normal((ns, nt))


@extended
@pytest.mark.parametrize("with_noise", [True, False], ids=["noise", "latent"])
@pytest.mark.parametrize("name", ["se_n800_m65_d3_c0", tj.SPLIT_NAME])
def test_draws(gp_mod, name, with_noise):
    """tests/test_gpu_predict_wide.py::test_draws for the sparse model, at 257 and then 129 points on the same handle.  Zero
    normals give the mean's bits.  The covariance reads no y (asserted: the same bits after set_data(X, 0)); with y = 0 the
    vector q, c' and the mean are exactly 0 (asserted), so the draws for normals = I are C^T exactly, and
        |Sigma_f - C C^T|_ij <= gamma_(nt+15) (|C||C^T|)_ij          (truth.factor_bound_worst)
    with Sigma_f the matrix that was factored: with noise (jitter 0) predict_joint's output bit for bit; latent (jitter
    1e-8 sf2) that output + jitter in longdouble, 2u (sf2 + jitter) allowed on the diagonal.  The draws:
        |s_st - (m_t + sum_k z_sk C_tk)| <= gamma_(nt+1) (|m_t| + sum_k |z_sk||C_tk|)   (truth.draw_bound_worst)."""
    s, (X, y, Z, _, cov) = make(gp_mod, name)
    Xt_all = tj.wide_points(name, 257)
    sf2 = float(cov.fp64().sf2)
    jitter = 0.0 if with_noise else 1e-8 * sf2                      # sample_posterior's default
    rep = Report("sparse-draws/%s/%s" % (name, "noise" if with_noise else "latent"))
    got = {}
    for nt in (257, 129):                                            # in this order: the smaller problem second
        Xt = np.ascontiguousarray(Xt_all[-nt:])
        m, _ = s.predict(Xt)
        assert same_bits([s.sample_posterior(Xt, 2, with_noise=with_noise, normals=np.zeros((2, nt)))], [np.stack([m, m])])
        draws = {ns: s.sample_posterior(Xt, ns, with_noise=with_noise, normals=normals(nt, ns)) for ns in NS}
        got[nt] = (Xt, m, draws, s.predict_joint(Xt, with_noise=with_noise)[1])
    s.set_data(X, np.zeros(len(y)))
    for nt in (257, 129):
        Xt, m, draws, cv = got[nt]
        m0, cv0 = s.predict_joint(Xt, with_noise=with_noise)
        assert same_bits([cv0], [cv]), "the joint covariance depends on y"
        assert not np.any(m0), "all-zero y: the mean is not exactly zero"
        Cf = np.ascontiguousarray(s.sample_posterior(Xt, nt, with_noise=with_noise, jitter=jitter, normals=np.eye(nt)).T)
        assert np.all(np.isfinite(Cf)) and np.all(np.diag(Cf) > 0)
        assert not np.any(np.triu(Cf, 1)), "strict upper triangle of the recovered factor is not zero"
        S = cv.astype(LD)
        S[np.arange(nt), np.arange(nt)] += LD(jitter)
        allow = 0.0 if with_noise else 2 * truth.U * (sf2 + jitter)
        r, at, res, bnd = truth.factor_bound_worst(S if jitter else cv, Cf, nt + truth.POTRF_EXTRA_ULPS, allow)
        rep.add("nt%d_factor@%d,%d" % ((nt,) + at), res, bnd, 0.0, 1)
        for ns in NS:
            r, at, err, bnd = truth.draw_bound_worst(draws[ns], m, normals(nt, ns), Cf)
            rep.add("nt%d_draws%d@%d,%d" % ((nt, ns) + at), err, bnd, 0.0, 1)
    s.close()
    rep.check()


# ------------------------------------------------------------------ 7. stale state is evaluated first
def test_staleness(gp_mod):
    name = "se_n800_m65_d3_c0"
    Xt = tj.wide_points(name, 129)
    s, (X, y, Z, _, cov) = make(gp_mod, name)
    first = everything(s, Xt)
    hp2 = np.asarray(cov.hp) + np.array([0.1, -0.05, 0.2])
    s.set_loghyperparam(hp2)                                           # no evaluation in between
    fresh, _ = make(gp_mod, name, hp=hp2)
    want = everything(fresh, Xt)
    assert same_bits(everything(s, Xt), want) and not same_bits(want[:2], first[:2])
    fresh.close()
    Z2 = np.ascontiguousarray(Z[::-1] + 0.01)
    s.set_inducing(Z2)
    fresh, _ = make(gp_mod, name, hp=hp2, Z=Z2)
    want = everything(fresh, Xt)
    assert same_bits(everything(s, Xt), want)
    s.set_targets(np.stack([y, 2 * y + 1], axis=1))
    for call in (s.predict_joint, s.predict_grad, lambda xt: (s.sample_posterior(xt, 3, normals=np.ones((3, len(xt)))),)):
        s.bound_targets()                                              # rewrites B's factor and c' ... for the targets
        got = call(Xt)
        assert same_bits(got, call(Xt))
    s.bound_targets()
    assert same_bits(everything(s, Xt), want)
    fresh.close()
    s.close()


# ------------------------------------------------------------------ 8. what was there keeps its bits
def test_existing_results_untouched(gp_mod):
    name = "se_n800_m65_d3_c0"
    Xt = tj.wide_points(name, 129)
    s, (X, y, Z, _, cov) = make(gp_mod, name)
    s.set_targets(np.stack([y, 2 * y + 1], axis=1))
    g = gp_mod.Covsum(300, X.shape[1])
    g.set_data(X[:300], y[:300])
    g.set_loghyperparam(cov.hp)

    def existing():
        F, gr = s.bound_grad()
        Fz, gz, gZ = s.bound_grad_z()
        return s.predict(Xt) + (np.array([F, Fz]), gr, gz, gZ) + s.predict_targets(Xt) \
            + g.compute_test_joint(None, None, Xt) + g.predict_grad(Xt)
    before = existing()
    new = everything(s, Xt)
    assert same_bits(existing(), before)
    s.bound_grad_z()                                                   # the gradient's gamma', beta' are on the device now
    assert same_bits(everything(s, Xt), new), "the new calls depend on what the last evaluation was"
    assert same_bits(existing(), before)
    g.close()
    s.close()


# ------------------------------------------------------------------ 9. refusals
def refused(rc, call):
    return rc == capi.CUGP_ERR_INVALID and call.encode() in capi.lib().cugp_last_error()


def test_refusals(gp_mod):
    name = "se_n300_m65"
    L, P = capi.lib(), capi.ptr
    X, y, Z, Xt, cov, chunk = ts.inputs(name)
    nt, d = Xt.shape
    mean, var, cv, dm, dv = np.full(nt, 7.0), np.full(nt, 7.0), np.full((nt, nt), 7.0), np.full((nt, d), 7.0), np.full((nt, d), 7.0)
    z, out = np.zeros((2, nt)), np.full((2, nt), 7.0)
    s = gp_mod.SparseGP(len(y), len(Z), d, chunk_rows=chunk)
    h = s.handle

    def all_three(why):
        assert refused(L.cugp_sparse_predict_cov(h, P(Xt), nt, 1, P(mean), P(cv)), "cugp_sparse_predict_cov"), why
        assert refused(L.cugp_sparse_predict_sample(h, P(Xt), nt, 1, 0.0, 2, P(z), P(out)), "cugp_sparse_predict_sample"), why
        assert refused(L.cugp_sparse_predict_grad(h, P(Xt), nt, 1, P(mean), P(var), P(dm), P(dv)), "cugp_sparse_predict_grad"), why
    all_three("no data")
    s.set_data(X, y)
    all_three("no inducing inputs")
    s.set_inducing(Z)
    s.set_loghyperparam(cov.hp)
    cc, sm, gr = "cugp_sparse_predict_cov", "cugp_sparse_predict_sample", "cugp_sparse_predict_grad"
    assert refused(L.cugp_sparse_predict_cov(h, None, nt, 1, P(mean), P(cv)), cc)
    assert refused(L.cugp_sparse_predict_cov(h, P(Xt), nt, 1, P(mean), None), cc)
    assert refused(L.cugp_sparse_predict_cov(h, P(Xt), 0, 1, P(mean), P(cv)), cc)
    assert refused(L.cugp_sparse_predict_sample(h, None, nt, 1, 0.0, 2, P(z), P(out)), sm)
    assert refused(L.cugp_sparse_predict_sample(h, P(Xt), nt, 1, 0.0, 2, None, P(out)), sm)
    assert refused(L.cugp_sparse_predict_sample(h, P(Xt), nt, 1, 0.0, 2, P(z), None), sm)
    assert refused(L.cugp_sparse_predict_sample(h, P(Xt), -1, 1, 0.0, 2, P(z), P(out)), sm)
    assert refused(L.cugp_sparse_predict_sample(h, P(Xt), nt, 1, 0.0, 0, P(z), P(out)), sm)
    for bad in (-1e-300, float("nan"), float("inf"), -float("inf")):
        assert refused(L.cugp_sparse_predict_sample(h, P(Xt), nt, 1, bad, 2, P(z), P(out)), sm), bad
    assert refused(L.cugp_sparse_predict_grad(h, None, nt, 1, P(mean), P(var), P(dm), P(dv)), gr)
    assert refused(L.cugp_sparse_predict_grad(h, P(Xt), 0, 1, P(mean), P(var), P(dm), P(dv)), gr)
    assert refused(L.cugp_sparse_predict_grad(h, P(Xt), nt, 1, P(mean), P(var), None, None), gr)
    for a in (mean, var, cv, dm, dv, out):
        assert np.all(a == 7.0), "a refused call wrote"
    # what may be NULL: mean of the covariance; mean, var and one of the gradients
    capi.check(L.cugp_sparse_predict_cov(h, P(Xt), nt, 1, None, P(cv)))
    capi.check(L.cugp_sparse_predict_grad(h, P(Xt), nt, 1, None, None, None, P(dv)))
    capi.check(L.cugp_sparse_predict_grad(h, P(Xt), nt, 0, None, None, P(dm), None))
    m2, cv2 = s.predict_joint(Xt)
    _, _, dm2, dv2 = s.predict_grad(Xt)
    assert same_bits((cv, dm, dv), (cv2, dm2, dv2)) and np.all(mean == 7.0) and np.all(var == 7.0)
    s.close()


def test_not_positive_definite_gives_nan_with_ok(gp_mod):
    """Duplicated inducing inputs under a jitter of 1e-300 (tests/test_gpu_sparse_targets.py's means): NaN outputs with CUGP_OK
    from all three calls, and a usable handle afterwards."""
    name = "se_n300_m65"
    X, y, Z, Xt, cov, chunk = ts.inputs(name)
    s, _ = make(gp_mod, name, jitter=1e-300)
    Zd = Z.copy()
    Zd[1::2] = Zd[0:-1:2][: len(Zd[1::2])]
    s.set_inducing(Zd)
    assert np.isnan(s.bound())
    out = everything(s, Xt)
    assert all(np.all(np.isnan(a)) for a in out) and out[1].shape == (ts.NT, ts.NT) and out[-1].shape == (3, ts.NT)
    s.close()
    s, _ = make(gp_mod, name)
    assert all(np.all(np.isfinite(a)) for a in everything(s, Xt))
    s.close()
