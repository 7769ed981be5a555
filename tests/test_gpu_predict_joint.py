"""Joint predictive covariance and posterior draws on the GPU (cugp_predict_cov, cugp_predict_sample): k_predict_cov
(Sigma = k(Xt,Xt) (+ sn2 I) - W W^T, W = Ks L^-T), the library's blocked Cholesky on an internal factor handle, and
k_predict_gemm over the factor for the draws.  Ground truth is numpy fp64 on the host:
    K = k(X,X) + sn2 I,  Sigma_ref = k(Xt,Xt) (+ sn2 I) - Ks K^-1 Ks^T,  C_ref = cholesky(Sigma_ref + jitter I)."""
import numpy as np
import pytest

from conftest import HP_DEFAULT, HP_DENSE, synth

pytestmark = pytest.mark.gpu

TUNE_COV_SPLIT = 20


@pytest.fixture(scope="module")
def gp():
    import cugp_amd.gp as gp
    return gp


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _se(A, B, hp):
    """sf2 exp(-|a - b|^2 / (2 l^2)), the squared distance summed over the dimensions in order"""
    d2 = np.zeros((A.shape[0], B.shape[0]))
    for k in range(A.shape[1]):
        d2 += (A[:, k, None] - B[None, :, k]) ** 2
    return np.exp(2 * hp[1]) * np.exp(-0.5 * d2 / np.exp(2 * hp[0]))


def _scales(hp):
    sf2, sn2 = np.exp(2 * hp[1]), np.exp(2 * hp[2])
    return sf2, sn2


def _ref_cov(X, Xt, hp, with_noise):
    sf2, sn2 = _scales(hp)
    K = _se(X, X, hp) + sn2 * np.eye(X.shape[0])
    Ks = _se(Xt, X, hp)
    S = _se(Xt, Xt, hp) - Ks @ np.linalg.solve(K, Ks.T)
    S = 0.5 * (S + S.T)
    if with_noise:
        S = S + sn2 * np.eye(Xt.shape[0])
    return S


def _test_points(nt, d, seed=21):
    return np.random.default_rng(seed).uniform(-10, 10, (nt, d))


def _model(gp, n, d, hp, seed=3, npad_min=0):
    X, y = synth(n, d, seed=seed)
    g = gp.Covsum(n, d, 0, npad_min=npad_min)
    g.set_data(X, y)
    g.set_loghyperparam(hp)
    return g, X, y


NTS = [1, 63, 64, 65, 129, 1000]


@pytest.mark.parametrize("hp", [HP_DEFAULT, HP_DENSE], ids=["hp_default", "hp_dense"])
@pytest.mark.parametrize("d", [1, 5, 10])
@pytest.mark.parametrize("n", [130, 1000, 2000])
def test_cov_against_numpy(gp, n, d, hp):
    """Every nt of NTS (the leading points of one set of 1000), both noise settings: within 1e-10 (sf2 + sn2) of
    numpy, exactly symmetric, the same bits on a repeated call; the mean has cugp_predict's bits and diag(cov) with
    noise is its variance up to rounding."""
    sf2, sn2 = _scales(hp)
    tol = 1e-10 * (sf2 + sn2)
    g, X, y = _model(gp, n, d, hp)
    Xt_all = _test_points(max(NTS), d)
    ref = {w: _ref_cov(X, Xt_all, hp, w) for w in (False, True)}
    for nt in NTS:
        Xt = Xt_all[:nt]
        m0, v0 = g.compute_test_means_and_variances(None, None, Xt)
        for w in (False, True):
            m, cov = g.compute_test_joint(None, None, Xt, with_noise=w)
            err = np.max(np.abs(cov - ref[w][:nt, :nt]))
            assert err <= tol, (nt, w, err, tol)
            assert np.array_equal(cov, cov.T), (nt, w)
            assert _same(m, m0), (nt, w)
            m2, cov2 = g.compute_test_joint(None, None, Xt, with_noise=w)
            assert _same(cov2, cov) and _same(m2, m), (nt, w)
            if w:
                assert np.max(np.abs(np.diag(cov) - v0)) <= 1e-12 * (sf2 + sn2), (nt, np.max(np.abs(np.diag(cov) - v0)))
    g.close()


def test_predict_unchanged_around_joint_calls(gp):
    """cugp_predict before and after the new calls, same handle and points: the same bits."""
    g, X, y = _model(gp, 1000, 5, HP_DENSE)
    Xt = _test_points(300, 5)
    m0, v0 = g.compute_test_means_and_variances(None, None, Xt)
    g.compute_test_joint(None, None, Xt, with_noise=True)
    g.sample_posterior(None, None, Xt, 5, with_noise=True, rng=1)
    g.compute_test_joint(None, None, Xt[:70], with_noise=False)
    m1, v1 = g.compute_test_means_and_variances(None, None, Xt)
    assert _same(m0, m1) and _same(v0, v1)
    g.close()


def test_hyperparameter_change_without_evaluation(gp):
    """set_loghyperparam, then the covariance with no evaluation in between: the reference at the new point."""
    g, X, y = _model(gp, 1000, 5, HP_DEFAULT)
    Xt = _test_points(200, 5)
    g.compute_test_joint(None, None, Xt)
    hp2 = [0.9, -0.2, -0.8]
    g.set_loghyperparam(hp2)
    _, cov = g.compute_test_joint(None, None, Xt, with_noise=True)
    sf2, sn2 = _scales(hp2)
    assert np.max(np.abs(cov - _ref_cov(X, Xt, hp2, True))) <= 1e-10 * (sf2 + sn2)
    g.close()


def test_padded_handle(gp):
    """a handle padded far beyond its rows (cugp_create_padded) matches its own reference"""
    hp = HP_DENSE
    g, X, y = _model(gp, 300, 5, hp, npad_min=900)
    Xt = _test_points(129, 5)
    sf2, sn2 = _scales(hp)
    for w in (False, True):
        _, cov = g.compute_test_joint(None, None, Xt, with_noise=w)
        assert np.max(np.abs(cov - _ref_cov(X, Xt, hp, w))) <= 1e-10 * (sf2 + sn2), w
    Z = np.random.default_rng(4).standard_normal((7, 129))
    s = g.sample_posterior(None, None, Xt, 7, with_noise=True, normals=Z)
    m, _ = g.compute_test_means_and_variances(None, None, Xt)
    C = np.linalg.cholesky(_ref_cov(X, Xt, hp, True))
    assert np.max(np.abs(s - (m + Z @ C.T))) <= 1e-9 * np.sqrt(sf2 + sn2)
    g.close()


def test_bcm_expert(gp):
    """expert 1 of a three-expert BCM matches the reference over its own rows"""
    rows, d, hp = [300, 300, 300], 5, HP_DEFAULT
    X, y = synth(sum(rows), d, seed=11)
    b = gp.BCM(rows, d, 0)
    for k in range(3):
        b.set_expert_data(k, X[300 * k:300 * (k + 1)], y[300 * k:300 * (k + 1)])
    b.set_BCM_log_hyperparam(hp)
    e = b.expert(1)
    Xt = _test_points(65, d)
    sf2, sn2 = _scales(hp)
    m0, v0 = e.compute_test_means_and_variances(None, None, Xt)
    m, cov = e.compute_test_joint(None, None, Xt, with_noise=True)
    assert _same(m, m0)
    assert np.max(np.abs(cov - _ref_cov(X[300:600], Xt, hp, True))) <= 1e-10 * (sf2 + sn2)
    s = e.sample_posterior(None, None, Xt, 3, with_noise=False, rng=2)
    assert s.shape == (3, 65) and np.all(np.isfinite(s))
    b.close()


@pytest.fixture(scope="module")
def sample_model(gp):
    g, X, y = _model(gp, 300, 5, HP_DEFAULT, seed=7)
    yield g, X
    g.close()


def test_zero_normals_give_the_mean(gp, sample_model):
    g, X = sample_model
    Xt = _test_points(129, 5)
    m0, _ = g.compute_test_means_and_variances(None, None, Xt)
    for w in (False, True):
        s = g.sample_posterior(None, None, Xt, 3, with_noise=w, normals=np.zeros((3, 129)))
        for r in s:
            assert _same(r, m0), w


@pytest.mark.parametrize("w", [False, True], ids=["latent", "noise"])
def test_unit_normals_pick_factor_columns(gp, sample_model, w):
    """normals = e_k: exactly the mean above row k (a stray value above the diagonal of a diagonal tile shows here),
    mean + C_ref[:, k] from row k on"""
    g, X = sample_model
    hp, nt = HP_DEFAULT, 129
    sf2, sn2 = _scales(hp)
    Xt = _test_points(nt, 5)
    m0, _ = g.compute_test_means_and_variances(None, None, Xt)
    jit = 0.0 if w else 1e-8 * sf2
    C = np.linalg.cholesky(_ref_cov(X, Xt, hp, w) + jit * np.eye(nt))
    ks = [0, 63, 64, 128]
    Z = np.zeros((len(ks), nt))
    for i, k in enumerate(ks):
        Z[i, k] = 1.0
    s = g.sample_posterior(None, None, Xt, len(ks), with_noise=w, normals=Z)
    for i, k in enumerate(ks):
        assert _same(s[i, :k], m0[:k]), k
        assert np.max(np.abs(s[i, k:] - (m0[k:] + C[k:, k]))) <= 1e-9 * np.sqrt(sf2 + sn2), k


@pytest.mark.parametrize("ns", [1, 7, 64, 200])
@pytest.mark.parametrize("w", [False, True], ids=["latent", "noise"])
def test_random_normals(gp, sample_model, ns, w):
    g, X = sample_model
    hp, nt = HP_DEFAULT, 129
    sf2, sn2 = _scales(hp)
    Xt = _test_points(nt, 5)
    m0, _ = g.compute_test_means_and_variances(None, None, Xt)
    Z = np.random.default_rng(ns).standard_normal((ns, nt))
    s = g.sample_posterior(None, None, Xt, ns, with_noise=w, normals=Z)
    jit = 0.0 if w else 1e-8 * sf2
    C = np.linalg.cholesky(_ref_cov(X, Xt, hp, w) + jit * np.eye(nt))
    assert np.max(np.abs(s - (m0 + Z @ C.T))) <= 1e-9 * np.sqrt(sf2 + sn2)
    s2 = g.sample_posterior(None, None, Xt, ns, with_noise=w, normals=Z)
    assert _same(s2, s)


def test_dense_hyperparameters_with_noise(gp):
    """HP_DENSE (long length scale: the latent covariance is nearly singular, so draws with the noise term)"""
    hp, nt, ns = HP_DENSE, 200, 16
    sf2, sn2 = _scales(hp)
    g, X, y = _model(gp, 1000, 5, hp)
    Xt = _test_points(nt, 5)
    m0, _ = g.compute_test_means_and_variances(None, None, Xt)
    Z = np.random.default_rng(6).standard_normal((ns, nt))
    s = g.sample_posterior(None, None, Xt, ns, with_noise=True, normals=Z)
    C = np.linalg.cholesky(_ref_cov(X, Xt, hp, True))
    assert np.max(np.abs(s - (m0 + Z @ C.T))) <= 1e-9 * np.sqrt(sf2 + sn2)
    g.close()


def test_large_factorisation(gp):
    """nt = 6200 (49 tiles) against 300 rows: the internal factor handle takes the two-speed Cholesky"""
    from cugp_amd import capi
    import ctypes as C
    v = C.c_int()
    probe = gp.Covsum(8, 1, 0)
    capi.check(capi.lib().cugp_get_handle_tuning(probe.handle, 8, C.byref(v)))
    P = v.value
    capi.check(capi.lib().cugp_get_handle_tuning(probe.handle, 10, C.byref(v)))
    min_nt = v.value
    probe.close()
    nt = 6200
    assert (nt + 127) // 128 >= max(3 * P, min_nt), (P, min_nt)
    hp = HP_DEFAULT
    sf2, sn2 = _scales(hp)
    g, X, y = _model(gp, 300, 5, hp)
    Xt = _test_points(nt, 5, seed=5)
    S = _ref_cov(X, Xt, hp, True)
    m0, _ = g.compute_test_means_and_variances(None, None, Xt)
    m, cov = g.compute_test_joint(None, None, Xt, with_noise=True)
    assert _same(m, m0)
    assert np.max(np.abs(cov - S)) <= 1e-10 * (sf2 + sn2)
    del cov
    Z = np.random.default_rng(8).standard_normal((7, nt))
    s = g.sample_posterior(None, None, Xt, 7, with_noise=True, normals=Z)
    Cr = np.linalg.cholesky(S)
    assert np.max(np.abs(s - (m0 + Z @ Cr.T))) <= 1e-9 * np.sqrt(sf2 + sn2)
    # a smaller problem afterwards runs in the same factor handle's buffers
    Xs = Xt[:100]
    Z = np.random.default_rng(9).standard_normal((5, 100))
    s = g.sample_posterior(None, None, Xs, 5, with_noise=True, normals=Z)
    Cr = np.linalg.cholesky(S[:100, :100])
    assert np.max(np.abs(s - (m0[:100] + Z @ Cr.T))) <= 1e-9 * np.sqrt(sf2 + sn2)
    g.close()


def test_sample_statistics(gp, sample_model):
    """nt = 40, 20 000 draws from a fixed seed: every entry of the empirical covariance within 5 standard errors"""
    g, X = sample_model
    nt, ns = 40, 20000
    Xt = _test_points(nt, 5, seed=12)
    m, cov = g.compute_test_joint(None, None, Xt, with_noise=False)
    s = g.sample_posterior(None, None, Xt, ns, with_noise=False, rng=np.random.default_rng(1234))
    assert s.shape == (ns, nt)
    d = s - m
    emp = d.T @ d / ns
    se = np.sqrt((np.outer(np.diag(cov), np.diag(cov)) + cov ** 2) / ns)
    z = np.abs(emp - cov) / se
    assert np.max(z) <= 5.0, np.max(z)
    assert np.max(np.abs(s.mean(0) - m) / np.sqrt(np.diag(cov) / ns)) <= 5.0


def test_metric_size(gp):
    """N = 8192, D = 10, nt = 1000 (the bench model): diag(cov) is cugp_predict's variance, the mean its bits"""
    hp = [np.log(3.0), 0.0, np.log(0.1)]
    sf2, sn2 = _scales(hp)
    g, X, y = _model(gp, 8192, 10, hp, seed=15618)
    Xt = _test_points(1000, 10)
    m0, v0 = g.compute_test_means_and_variances(None, None, Xt)
    m, cov = g.compute_test_joint(None, None, Xt, with_noise=True)
    assert _same(m, m0)
    assert np.max(np.abs(np.diag(cov) - v0)) <= 1e-12 * (sf2 + sn2)
    assert np.array_equal(cov, cov.T)
    s = g.sample_posterior(None, None, Xt, 64, with_noise=True, rng=3)
    assert s.shape == (64, 1000) and np.all(np.isfinite(s))
    g.close()


@pytest.mark.parametrize("nt", [65, 1000])
def test_tuning_key_forms(gp, nt):
    """tuning key 20: no split with 128x128 tiles (0), and other split counts / tile forms, against the default on
    the same inputs; each form repeats its own bits"""
    hp = HP_DENSE
    sf2, sn2 = _scales(hp)
    g, X, y = _model(gp, 2000, 10, hp)
    Xt = _test_points(nt, 10)
    _, c0 = g.compute_test_joint(None, None, Xt)
    for v in (0, 8, 256, 4096, 1 << 20):
        g.set_tuning(TUNE_COV_SPLIT, v)
        _, c = g.compute_test_joint(None, None, Xt)
        _, c2 = g.compute_test_joint(None, None, Xt)
        assert _same(c, c2), v
        assert np.max(np.abs(c - c0)) <= 1e-12 * (sf2 + sn2), (v, np.max(np.abs(c - c0)))
        s = g.sample_posterior(None, None, Xt, 4, with_noise=True, rng=5)
        assert np.all(np.isfinite(s)), v
    g.set_tuning(TUNE_COV_SPLIT, 0, own=False)
    g.close()
