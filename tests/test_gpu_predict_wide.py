"""Prediction beyond one test tile, held to fp64 ROUNDING (tests/test_gpu_accuracy.py and its siblings predict at 64
test points: one 128-row tile of the prediction side).  Here: 129, 200 and 257 test points -- k_cross for test rows
>= 128, k_predict_gemm for test tiles > 0, k_predict_finish for rows >= 128, k_predict_cov<2> beyond its first three
64-tiles and k_predict_cov<4>, k_predict_cov_finish on a second and third tile row and over split chunks, the batched
BCM launches in chunked passes -- and the posterior draws: the blocked Cholesky on the internal factor handle (also
reused for a smaller problem), k_zero_upper_diag, k_predict_gemm over the factor, k_sample_finish.

1. Marginal prediction and joint covariance against the longdouble truth, the project's bound unchanged:

       err_gpu(q) <= F * max(noise(q), floor(q))

   noise: truth.noise_level (the CPU oracle over the data as given and 7 permutations) at the SAME test points; floor: 4
   ulp of the quantity's scale; every entry of the joint covariance is held to the variances' yardstick and the cov
   floor, as test_gpu_accuracy.test_live_case does.  F is truth.F (F_ARD, F_MATERN): tests/test_truth_cpu.py measures
   the stand-in on the same wide rows (the BCM splits included) on the CPU and asserts the project's rule on them
   (docs/ACCURACY.md, "Beyond one test tile") -- nothing is taken from the GPU.  Every tile form of the covariance
   product is held to the truth.
2. Draws against two DERIVED bounds (no yardstick, no measured tolerance), longdouble on the host:

       |Sigma_f - C C^T|_ij <= gamma_(nt+15) (|C||C^T|)_ij                    the factor, all rows
       |s_st - (m_t + sum_k z_sk C_tk)| <= gamma_(nt+1) (|m_t| + sum_k |z_sk||C_tk|)    the draws

   with C recovered bit for bit from the library (all-zero targets, identity normals): see test_draws.

Every figure is printed before it is asserted ("ACC <case> <quantity> err noise floor ratio"; run with -s); means,
variances and covariance are reported per 128-row test tile ("_r0", "_r1", "_r2").  One process, one device; nothing
outside the tree is read.
"""
import numpy as np
import pytest

import accuracy
import truth
from accuracy import Report
from cugp_amd import capi

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not truth.EXTENDED, reason="numpy.longdouble is not an extended-precision type here")]

LD = truth.LD
TILE = 128
TUNE_PRED_CHUNK, TUNE_COV_SPLIT = 19, 20                            # kernels.h TUNE_*


@pytest.fixture(scope="module")
def gp_mod():
    import cugp_amd.gp as gp
    return gp


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def cov_forms(nt):
    """Values of tuning key 20 -> the form of the covariance product they select (predict_gfx950.h: predict_cov_shape, with
    t128 lower 128-tiles of the padded nt x nt result): None, the default 1024: 64x64 tiles, the k range split as far
    as n allows; 0: 128x128 tiles (k_predict_cov<4>), no split; 4 t128: the smallest value that still takes 64x64
    tiles -- there are more than 2 t128 of them, so the quotient that sets the split is 1: no split."""
    tiles = -(-nt // TILE)
    return (("split64", None), ("whole128", 0), ("whole64", 4 * (tiles * (tiles + 1) // 2)))


def tile_rows(nt):
    return [(r, slice(r * TILE, min(nt, (r + 1) * TILE))) for r in range(-(-nt // TILE))]


def hold_prediction(rep, g, c):
    """cugp_predict and cugp_predict_cov (with and without noise, every tile form) at the wide test points of the
    case c (accuracy.wide) against the truth, reported per 128-row test tile."""
    X, y, Xt, tmean, tvar, tcov, noise, fl = c["X"], c["y"], c["Xt"], c["tm"], c["tv"], c["tcov"], c["noise"], c["floor"]
    nt = len(Xt)
    tcn = tcov.copy()
    tcn[np.arange(nt), np.arange(nt)] += c["cov"].sn2
    m, v = g.compute_test_means_and_variances(X, y, Xt)
    for r, sl in tile_rows(nt):
        rep.add("mean_r%d" % r, np.max(np.abs(m[sl].astype(LD) - tmean[sl])), noise["mean"], fl["mean"])
        rep.add("var_r%d" % r, np.max(np.abs(v[sl].astype(LD) - tvar[sl])), noise["var"], fl["var"])
    try:
        for form, value in cov_forms(nt):
            if value is not None:
                g.set_tuning(TUNE_COV_SPLIT, value)
            for with_noise, tc in ((True, tcn), (False, tcov)):
                mj, cov = g.compute_test_joint(X, y, Xt, with_noise=with_noise)
                assert same_bits(mj, m), (form, with_noise)             # the mean has cugp_predict's bits
                assert np.array_equal(cov, cov.T), (form, with_noise)
                err = np.abs(cov.astype(LD) - tc)
                for r, sl in tile_rows(nt):
                    rep.add("cov_%s_%s_r%d" % ("noise" if with_noise else "latent", form, r), np.max(err[sl]),
                            noise["var"], fl["cov"])
    finally:
        g.set_tuning(TUNE_COV_SPLIT, 0, own=False)                  # back to the process default (test_tuning_key_forms)


# ------------------------------------------------------------------ 1. prediction and joint covariance
def hold_wide(gp_mod, oracle, tag, family, name, nt, **handle):
    """One family's wide case on a handle Covsum(n, d, **handle): the shared body of the three tests below."""
    c = accuracy.wide(oracle, family, name, nt)
    rep = Report("%s/nt%d" % (tag, nt), c["cov"])
    g = gp_mod.Covsum(*c["X"].shape, **handle)
    if handle:                                                      # as the family's own tests create their handles:
        g.set_data(c["X"], c["y"])                                  # data first; the SE handle binds it on first use
    g.set_loghyperparam(c["cov"].hp)
    hold_prediction(rep, g, c)
    g.close()
    rep.check()


@pytest.mark.parametrize("name,nt", [(c, nt) for c, nts in truth.WIDE_CASES.items() for nt in nts])
def test_wide_se(gp_mod, oracle, name, nt):
    """truth.WIDE_CASES: n65 (nt > n, the covariance product's k range is one block), n300_d17 (two feature chunks
    through k_cross), n384_cond1e6, n515_dense (the product splits in two over k) at 129 / 200 / 257 test points, and
    n1025_dense (a split of four) at 200."""
    hold_wide(gp_mod, oracle, name, "se", name, nt)


def test_wide_ard(gp_mod, oracle):
    """cross_body<ARD> and predict_cov_finish_body<ARD>: n257_d3 with ARD_CASES' length scales, 200 test points."""
    name = truth.WIDE_FAMILY_CASES["ard"]
    hold_wide(gp_mod, oracle, "ard_" + name, "ard", name, truth.WIDE_NT_FAMILY, ard=True)


def test_wide_matern52(gp_mod, oracle):
    """cross_body<., MATERN52> and predict_cov_finish_body<., MATERN52>: n300_d17 at nu = 5/2, 200 test points."""
    name = truth.WIDE_FAMILY_CASES["matern52"]
    hold_wide(gp_mod, oracle, "matern52_" + name, "matern52", name, truth.WIDE_NT_FAMILY, kernel=truth.MATERN52)


@pytest.mark.parametrize("N,K", truth.WIDE_BCM, ids=["3x300", "5-uneven-1307"])
def test_wide_bcm(gp_mod, oracle, N, K):
    """Three 300-row experts as a group and the uneven 5-expert split of 1307 rows at 200 test points: the batched
    (blockIdx.y) launches of k_cross, k_predict_gemm and k_predict_finish through cugp_bcm_predict, and once more in
    passes of 64 test points (tuning key 19 = 1: passes at t0 > 0) through cugp_bcm_predict_allgather in a world of
    one -- both against truth.bcm_truth, the yardstick from the oracle's BCM with the rows permuted inside each expert
    (as tests/golden/make_truth.py does for bcm3x1500)."""
    X, y, Xt, cov = truth.wide_bcm_inputs(N, K)
    nt = len(Xt)
    tb = truth.bcm_truth(X, y, cov, K, Xt)
    noise, _, _ = truth.bcm_yardstick(oracle, cov, X, y, K, Xt, tb)
    fl = truth.floors(cov, truth.scales(cov, tb["ll"], tb["grad"], tb["mean"]))
    rep = Report("bcm%dx%d/nt%d" % (K, N, nt), cov)
    b = gp_mod.BCM.split(X, y, K)
    try:
        assert b.rows == [r for _, r in truth.bcm_rows(N, K)]
        b.set_BCM_log_hyperparam(cov.hp)
        m, v = b.compute_BCM_test_means_and_var(Xt)
        comm = gp_mod.Comm(None, 0, 1, 0)
        try:
            capi.check(capi.lib().cugp_set_tuning(TUNE_PRED_CHUNK, 1))
            mc, vc = comm.predict_allgather(b, K, K, Xt)
        finally:
            capi.check(capi.lib().cugp_set_tuning(TUNE_PRED_CHUNK, 0))     # the built-in default
            comm.close()
    finally:
        b.close()
    for tag, mm, vv in (("", m, v), ("chunk64_", mc, vc)):
        for r, sl in tile_rows(nt):
            e = truth.errors_pred(mm[sl], vv[sl], tb["mean"][sl], tb["var"][sl])
            rep.add("%smean_r%d" % (tag, r), e["mean"], noise["mean"], fl["mean"])
            rep.add("%svar_r%d" % (tag, r), e["var"], noise["var"], fl["var"])
    rep.check()


# ------------------------------------------------------------------ 2. posterior draws
NS = (7, 129, 257)                     # one, two and three 128-row tiles of normals


def normals(nt, ns):
    return np.random.default_rng(1000 * nt + ns).standard_normal((ns, nt))


@pytest.mark.parametrize("with_noise", [True, False], ids=["noise", "latent"])
@pytest.mark.parametrize("name", ["n300_d17", "n515_dense"])
def test_draws(gp_mod, name, with_noise):
    """s = m + C z with C = chol(Sigma_f), at 257 and then 129 test points on the same handle (the second factorisation
    runs in the larger factor handle's buffers, with another leading dimension), for 7, 129 and 257 draws.  Comparing C
    with a truth factor would measure cond(Sigma), not the kernels; what the kernels answer for is checked instead.

    C is recovered bit for bit: Sigma does not depend on y (asserted: cugp_predict_cov returns the same bits after
    set_data(X, 0)); with all-zero targets alpha and the mean are exactly 0 (asserted), so the draws for normals = I
    are C^T exactly -- products with 1 and 0 are exact, and so is 0 + x.  Its strict upper triangle is exactly zero.

    The factor, componentwise on all rows (truth.factor_bound_worst; the index is test_factor_residual's, the kernels
    are the same):   |Sigma_f - C C^T|_ij <= gamma_(nt+15) (|C||C^T|)_ij.
    Sigma_f is the matrix that was factored.  With noise (jitter 0) it is cugp_predict_cov's output bit for bit: adding
    0.0 is exact.  Latent (jitter 1e-8 sf2): the returned covariance + jitter on the diagonal, formed in longdouble,
    with 2u (sf2 + jitter) allowed on diagonal entries: the kernel rounds fl(k_tt + jitter) and then the difference
    with the product, the returned covariance rounds the difference alone -- two roundings of at most u (sf2 + jitter)
    each, in another order.

    The draws, with the library's own cugp_predict mean m and fixed-seed normals z (truth.draw_bound_worst):
        |s_st - (m_t + sum_k z_sk C_tk)| <= gamma_(nt+1) (|m_t| + sum_k |z_sk||C_tk|)
    which holds for any order of summation, with or without fma, plus the one rounding of k_sample_finish.
    C comes back through the same k_predict_gemm and k_sample_finish as the draws, so the draw bound is blind by
    construction to a defect of that path that is LINEAR in F = Z C^T (rows of F scaled, say): it lands in the recovered
    C' as well, and s and m + Z C'^T still agree to rounding.  Such a defect is caught by the factor bound alone, which
    holds C' to Sigma_f (|Sigma_f - C' C'^T|); the draw bound sees what is not linear in Z: a wrong tile read for other
    rows of normals, the mean, the final sum.
    (n515_dense latent: cond(Sigma_f) ~ 1e8 with the default jitter; the bounds are componentwise and hold there.)"""
    X, y, Xt_all, cov = truth.wide_inputs(name, 257)
    hp = cov.hp
    sf2 = float(np.exp(2.0 * hp[1]))
    jitter = 0.0 if with_noise else 1e-8 * sf2                      # sample_posterior's default
    rep = Report("%s/%s" % (name, "noise" if with_noise else "latent"))
    g = gp_mod.Covsum(*X.shape)
    g.set_data(X, y)
    g.set_loghyperparam(hp)
    got = {}
    for nt in (257, 129):                                            # in this order: the smaller problem second
        Xt = np.ascontiguousarray(Xt_all[-nt:])
        m, _ = g.compute_test_means_and_variances(None, None, Xt)
        draws = {ns: g.sample_posterior(None, None, Xt, ns, with_noise=with_noise, normals=normals(nt, ns)) for ns in NS}
        _, cov = g.compute_test_joint(None, None, Xt, with_noise=with_noise)
        got[nt] = (Xt, m, draws, cov)
    g.set_data(X, np.zeros(len(y)))
    for nt in (257, 129):
        Xt, m, draws, cov = got[nt]
        m0, cov0 = g.compute_test_joint(None, None, Xt, with_noise=with_noise)
        assert same_bits(cov0, cov), "the joint covariance depends on y"
        assert not np.any(m0) and not np.any(g.get_alpha()), "all-zero targets: alpha and the mean are not exactly zero"
        C = np.ascontiguousarray(g.sample_posterior(None, None, Xt, nt, with_noise=with_noise, normals=np.eye(nt)).T)
        assert np.all(np.isfinite(C)) and np.all(np.diag(C) > 0)
        assert not np.any(np.triu(C, 1)), "strict upper triangle of the recovered factor is not zero"
        S = cov.astype(LD)
        S[np.arange(nt), np.arange(nt)] += LD(jitter)
        allow = 0.0 if with_noise else 2 * truth.U * (sf2 + jitter)
        r, at, res, bnd = truth.factor_bound_worst(S if jitter else cov, C, nt + truth.POTRF_EXTRA_ULPS, allow)
        rep.add("nt%d_factor@%d,%d" % ((nt,) + at), res, bnd, 0.0, 1)
        for ns in NS:
            r, at, err, bnd = truth.draw_bound_worst(draws[ns], m, normals(nt, ns), C)
            rep.add("nt%d_draws%d@%d,%d" % ((nt, ns) + at), err, bnd, 0.0, 1)
    g.close()
    rep.check()
