"""The combination rules' surface and their host arithmetic, no GPU: header, ctypes binding and built library agree on
the new symbols and constants; cugp_poe_combine (pure host code, the twin of the device kernel k_poe_reduce_mode) against
a numpy.longdouble restatement on synthetic rows; the identities the formulas imply; the refusals.

The tolerance of the longdouble comparison is derived, not measured.  Every sum is over K terms that enter with the
magnitudes |beta_k| p_k (and |1 - sum beta_k| / sf2 for the prior term), every operation rounded once, so with u = 2^-53
and c = 2 K + 8 roundings along the longest path

    |prec - prec*| <= c u A,   A = sum (|beta_k| + delta) p_k + (|1 - sum beta_k| + K delta) / sf2

where delta = 1 for rbcm only: its beta_k = 1/2 log(sf2 p_k) carries an ABSOLUTE error of a few u (the rounding of the
product under the log moves the log by one relative rounding of its argument), whatever the size of beta_k.  Then
|var - var*| <= c u (A / prec*) var* and |mean - mean*| <= c u ((A / prec*) |mean*| + var* sum (|beta_k| + delta) |pm_k|).
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cugp_amd.gp as gp
from cugp_amd import capi
from cugp_amd.capi import ptr
from conftest import ROOT

LD = np.longdouble
U = 2.0 ** -53
MODES = ("poe", "gpoe", "bcm", "rbcm")
SF2, SN2 = 1.4918246976412703, 0.1353352832366127


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def ulps(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b)) / np.spacing(np.abs(np.asarray(b))))


# ------------------------------------------------------------------ the surface
@pytest.mark.parametrize("name,nargs", [("cugp_predict_latent", 5), ("cugp_poe_combine", 9), ("cugp_bcm_predict_mode", 7),
                                        ("cugp_bcm_predict_allgather_mode", 12)])
def test_symbols_declared_bound_and_exported(name, nargs):
    text = open(os.path.join(ROOT, "include", "cugp.h")).read()
    assert re.search(r"\bint %s\s*\(" % name, text)
    assert name in capi.SIGNATURES
    assert len(capi.SIGNATURES[name][1]) == nargs
    assert hasattr(capi.lib(), name)


def test_constants_agree():
    text = open(os.path.join(ROOT, "include", "cugp.h")).read()
    for name, value in (("POE", 0), ("GPOE", 1), ("BCM", 2), ("RBCM", 3)):
        assert re.search(r"#define CUGP_COMBINE_%s %d\b" % (name, value), text)
        assert getattr(capi, "CUGP_COMBINE_" + name) == value
        assert gp.COMBINE[name.lower()] == value
        assert gp.combine_mode(name.lower()) == value
    for cite in ("Tresp 2000", "Cao & Fleet 2014", "Deisenroth & Ng 2015"):
        assert cite in text


def test_python_surface():
    import inspect
    from cugp_amd.bcm import ShardedBCM
    for fn in (gp.BCM.predict, ShardedBCM.predict):
        p = inspect.signature(fn).parameters
        assert p["combine"].default is None and p["with_noise"].default is True
    p = inspect.signature(gp.Comm.predict_allgather).parameters
    assert p["combine"].default is None and "with_noise" in p and "sf2" in p and "sn2" in p
    assert callable(gp.Covsum.predict_latent) and callable(gp.poe_combine)


# ------------------------------------------------------------------ the arithmetic
def synthetic_rows(K, nt, seed):
    """var_f,k in (0.02, 1] sf2, some experts exactly uninformative (var_f = sf2), means of both signs."""
    rng = np.random.default_rng(seed)
    v = SF2 * rng.uniform(0.02, 1.0, (K, nt))
    v[rng.uniform(size=(K, nt)) < 0.15] = SF2
    m = rng.standard_normal((K, nt))
    rows = np.empty((K, 2, nt))
    rows[:, 0] = 1.0 / v
    rows[:, 1] = (1.0 / v) * m
    return rows


def longdouble_truth(rows, mode):
    """-> (mean, var_f, A / prec, var_f sum (|beta| + delta) |pm|) in longdouble from the fp64 rows."""
    p, pm = rows[:, 0].astype(LD), rows[:, 1].astype(LD)
    K = len(p)
    sf2 = LD(SF2)
    if mode == "gpoe":
        beta = np.full_like(p, LD(1) / LD(K))
    elif mode == "rbcm":
        beta = LD(0.5) * np.log(sf2 * p)
    else:
        beta = np.ones_like(p)
    delta = 1 if mode == "rbcm" else 0
    sp, spm, sb = (beta * p).sum(0), (beta * pm).sum(0), beta.sum(0)
    prior = mode in ("bcm", "rbcm")
    prec = sp + (1 - sb) / sf2 if prior else sp
    A = ((np.abs(beta) + delta) * p).sum(0) + ((np.abs(1 - sb) + K * delta) / sf2 if prior else 0)
    tv = 1 / prec
    return tv * spm, tv, A / prec, tv * ((np.abs(beta) + delta) * np.abs(pm)).sum(0)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("K,nt", [(K, nt) for K in (1, 3, 16) for nt in (1, 257)])
def test_combine_against_longdouble(K, nt, mode):
    rows = synthetic_rows(K, nt, 100 * K + nt)
    tm, tv, cond, ms = longdouble_truth(rows, mode)
    c = (2 * K + 8) * U
    mean, var = gp.poe_combine(rows, mode, SF2, SN2, with_noise=False)
    ev, em = np.abs(var.astype(LD) - tv), np.abs(mean.astype(LD) - tm)
    bv, bm = c * cond * tv, c * (cond * np.abs(tm) + ms)
    print("COMBINE K%-2d nt%-3d %-4s var err/bound %.3f  mean err/bound %.3f  cond %.1f" % (
        K, nt, mode, float(np.max(ev / bv)), float(np.max(em / bm)), float(np.max(cond))))
    assert np.all(ev <= bv) and np.all(em <= bm)
    assert np.all(var > 0)
    if mode in ("bcm", "rbcm"):
        assert np.all(var <= SF2 * (1 + c * np.max(cond)))


@pytest.mark.parametrize("mode", MODES)
def test_with_noise_adds_exactly_sn2(mode):
    rows = synthetic_rows(3, 257, 5)
    ml, vl = gp.poe_combine(rows, mode, SF2, SN2, with_noise=False)
    mn, vn = gp.poe_combine(rows, mode, SF2, SN2, with_noise=True)
    assert same_bits(mn, ml) and same_bits(vn, vl + SN2)


@pytest.mark.parametrize("mode", ("poe", "gpoe", "bcm"))
def test_one_expert_is_returned(mode):
    rng = np.random.default_rng(3)
    v = SF2 * rng.uniform(0.02, 1.0, 257)
    m = rng.standard_normal(257)
    rows = np.stack([1.0 / v, (1.0 / v) * m])[None]
    mean, var = gp.poe_combine(rows, mode, SF2, SN2, with_noise=False)
    assert ulps(var, v) <= 2 and ulps(mean, m) <= 2


@pytest.mark.parametrize("K", (1, 2, 3, 16))
def test_uninformative_experts(K):
    """p_k = RN(1 / sf2) for every k: bcm and rbcm give back the prior, var_f = sf2; poe gives sf2 / K -- the defect of the
    plain product that the other rules remove.

    4 ulp is what the fixed order of operations allows for rbcm at every K (beta_k = 1/2 log(sf2 p_k) is a rounding error,
    so prec = (1 - O(u)) / sf2 + O(u) p) and for bcm up to K = 3: 2 p is exact, 3 p rounds once (at most 2 ulp of p),
    (1 - K) / sf2 is -(K - 1) p exactly for K - 1 a power of two, so prec = p to 2 ulp and 1 / prec adds one more.  Beyond
    that bcm subtracts RN((K - 1) / sf2) from a K-term sum of about the same size: K p and (K - 1) / sf2 are each off by up
    to some K / 2 ulp of p and the difference is p.  No implementation of the stated arithmetic can hold 4 ulp there; K = 16
    is held to the derived bound of test_combine_against_longdouble, (2 K + 8) u A / prec with A / prec = 2 K - 1."""
    rows = np.zeros((K, 2, 5))
    rows[:, 0] = 1.0 / SF2
    mean, var = gp.poe_combine(rows, "rbcm", SF2, SN2, with_noise=False)
    assert ulps(var, np.full(5, SF2)) <= 4 and np.all(mean == 0)
    mean, var = gp.poe_combine(rows, "bcm", SF2, SN2, with_noise=False)
    print("UNINFORMATIVE K%-2d bcm var_f off sf2 by %.1f ulp" % (K, ulps(var, np.full(5, SF2))))
    if K <= 3:
        assert ulps(var, np.full(5, SF2)) <= 4
    else:
        assert np.all(np.abs(var - SF2) <= (2 * K + 8) * U * (2 * K - 1) * SF2)
    assert np.all(mean == 0)
    _, var = gp.poe_combine(rows, "poe", SF2, SN2, with_noise=False)
    assert ulps(var, np.full(5, SF2 / K)) <= 4
    _, var = gp.poe_combine(rows, "gpoe", SF2, SN2, with_noise=False)
    assert ulps(var, np.full(5, SF2)) <= 4


def test_nonpositive_and_nan_variances_propagate():
    rows = synthetic_rows(3, 4, 9)
    rows[1, 0, 0] = np.nan
    rows[1, 0, 1] = -rows[1, 0, 1]
    rows[:, 0, 2] = 0.0                                   # var_f = inf everywhere: prec 0 for poe
    for mode in MODES:
        mean, var = gp.poe_combine(rows, mode, SF2, SN2, with_noise=False)     # CUGP_OK: no exception
        assert np.isnan(var[0]) and np.isnan(mean[0])
        assert np.isfinite(var[3]) and np.isfinite(mean[3])
    _, var = gp.poe_combine(rows, "poe", SF2, SN2, with_noise=False)
    assert np.isinf(var[2])
    _, var = gp.poe_combine(rows, "rbcm", SF2, SN2, with_noise=False)
    assert np.isnan(var[1])                               # log of a negative number


# ------------------------------------------------------------------ refusals
def test_refusals():
    lib = capi.lib()
    rows = synthetic_rows(2, 3, 1)
    m, v = np.empty(3), np.empty(3)
    ok = lambda mode, K=2, nt=3, r=ptr(rows), pm=ptr(m), pv=ptr(v): lib.cugp_poe_combine(r, K, nt, mode, SF2, SN2, 1, pm, pv)
    assert ok(0) == capi.CUGP_OK
    for mode in (-1, 4, 99):
        assert ok(mode) == capi.CUGP_ERR_INVALID
    assert b"cugp_poe_combine" in lib.cugp_last_error()
    assert ok(0, K=0) == capi.CUGP_ERR_INVALID and ok(0, K=-1) == capi.CUGP_ERR_INVALID
    assert ok(0, nt=0) == capi.CUGP_ERR_INVALID and ok(0, nt=-5) == capi.CUGP_ERR_INVALID
    assert ok(0, r=None) == capi.CUGP_ERR_INVALID
    assert ok(0, pm=None) == capi.CUGP_ERR_INVALID
    assert ok(0, pv=None) == capi.CUGP_ERR_INVALID
    # the device-side calls refuse bad arguments before any device call: no GPU is needed to be told so
    Xt = np.zeros((3, 2))
    null = C.c_void_p()
    assert lib.cugp_predict_latent(null, ptr(Xt), 3, ptr(m), ptr(v)) == capi.CUGP_ERR_INVALID
    assert lib.cugp_bcm_predict_mode(null, ptr(Xt), 3, 0, 1, ptr(m), ptr(v)) == capi.CUGP_ERR_INVALID
    assert lib.cugp_bcm_predict_allgather_mode(null, null, 1, 1, ptr(Xt), 3, 0, 1, SF2, SN2, ptr(m), ptr(v)) == \
        capi.CUGP_ERR_INVALID
    assert lib.cugp_bcm_predict_allgather_mode(null, null, 1, 1, ptr(Xt), 3, 7, 1, SF2, SN2, ptr(m), ptr(v)) == \
        capi.CUGP_ERR_INVALID


def test_unknown_combine_names_raise_before_any_library_call():
    from cugp_amd.bcm import ShardedBCM
    for bad in ("product", "", "BCM2", 3, 1.5):
        with pytest.raises(ValueError):
            gp.combine_mode(bad)
    b = gp.BCM.__new__(gp.BCM)                            # no handle at all: the name is checked first
    b._h = None
    with pytest.raises(ValueError):
        b.predict(np.zeros((1, 2)), combine="robust")
    s = ShardedBCM.__new__(ShardedBCM)
    with pytest.raises(ValueError):
        s.predict(np.zeros((1, 2)), combine="robust")
    c = gp.Comm.__new__(gp.Comm)
    c._h = None
    with pytest.raises(ValueError):
        c.predict_allgather(None, 1, 1, np.zeros((1, 2)), combine="robust")
    with pytest.raises(ValueError):
        gp.poe_combine(np.zeros((1, 2, 1)), "robust", SF2, SN2)
    assert gp.combine_mode("RBCM") == capi.CUGP_COMBINE_RBCM
