"""The surface of the input gradients and their host arithmetic, no GPU: header, ctypes binding and built library agree on
the new symbols; every refusal comes back as CUGP_ERR_INVALID before any device call; cugp_poe_combine_grad (pure host
code) against a numpy.longdouble restatement of the chain rule on synthetic rows; the identities the formulas imply.

The tolerance of the longdouble comparison is derived, not measured.  With u = 2^-53, p = 1 / v, dp = -dv / v^2,
dbeta = 0 | -1/2 dv / v and delta = 1 for rbcm only (its beta = 1/2 log(sf2 p) carries an ABSOLUTE error of a few u,
whatever its size -- tests/test_poe_modes_api.py), the sums of the absolute values of the terms that enter are

    A  = sum (|beta| + delta) p + (|1 - sum beta| + K delta) / sf2            (prec;  the prior term for bcm, rbcm)
    D  = sum (|dbeta| p + (|beta| + delta) |dp|) + (sum |dbeta|) / sf2         (dprec)
    MS = sum (|beta| + delta) |p m|                                            (S)
    E  = sum (|dbeta| |p m| + (|beta| + delta) (|dp m| + p |dm|))              (dS)

dvar = -dprec / prec^2.  Roundings along its longest path: p (1), v v (1), dv / (v v) (1), beta (1; rbcm: 3, in units of
|beta| + 1), beta dp (1), rbcm's dbeta (1), dbeta p (2), their sum (1); the K-term running sum (K, each relative to the
running sum of absolute values); the prior term's K-term sum, division and subtraction (K + 2); prec prec and the division
(2): at most cv = 2 K + 16, which also covers prec's own 2 K + 8 (tests/test_poe_modes_api.py), entering twice through
A / prec:

    |dvar - dvar*| <= cv u Bv,   Bv = D / prec^2 + 2 (A / prec) |dprec| / prec^2

dmean is evaluated with the difference of the means first (include/cugp.h):  sum w_k dm_k + (sum a_k (m_k - mean)) / prec
+ [prior] mean ((sum dbeta) / sf2) / prec,  a_k = dbeta p + beta dp,  w_k = beta_k p_k / prec,  mean = sum w_k m_k.  Every
term is bounded by its absolute-value form: |w_k dm_k| and |a_k m_k| / prec are the terms of E / prec, |a_k mean| / prec and
the prior term are at most (D / prec)(MS / prec) since |mean| <= MS / prec.  Roundings: prec 2 K + 8 (in units of
A / prec >= 1), w_k + 2, mean + K + 1, the difference 1, a_k at most 9 (above), the product 1, the K-term sum K, the
division by prec 1 + (2 K + 8), the final sums 2: at most cm = 6 K + 32, all in units of A / prec:

    |dmean - dmean*| <= cm u Bm,   Bm = (A / prec) (E + D MS / prec) / prec

with every right-hand side evaluated in longdouble from the fp64 inputs.
"""
import ctypes as C
import inspect
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
MODES = ("poe", "gpoe", "bcm", "rbcm", "reference")
SF2, SN2 = 1.4918246976412703, 0.1353352832366127


def ulps(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b)) / np.spacing(np.abs(np.asarray(b))))


# ------------------------------------------------------------------ the surface
@pytest.mark.parametrize("name,nargs", [("cugp_predict_grad", 8), ("cugp_poe_combine_grad", 11), ("cugp_bcm_predict_grad", 9)])
def test_symbols_declared_bound_and_exported(name, nargs):
    text = open(os.path.join(ROOT, "include", "cugp.h")).read()
    assert re.search(r"\bint %s\s*\(" % name, text)
    assert name in capi.SIGNATURES
    assert len(capi.SIGNATURES[name][1]) == nargs
    assert hasattr(capi.lib(), name)


def test_reference_mode_constant_and_header_text():
    text = open(os.path.join(ROOT, "include", "cugp.h")).read()
    assert re.search(r"#define CUGP_COMBINE_REFERENCE \(-1\)", text)
    assert capi.CUGP_COMBINE_REFERENCE == -1
    for phrase in ("dmean / dx*_c", "dvar / dx*_c", "The reference has no counterpart", "[nt][d]", "CUGP_ERR_INVALID"):
        assert phrase in text


def test_python_surface():
    p = inspect.signature(gp.Covsum.predict_grad).parameters
    assert p["with_noise"].default is True and p["want_var_grad"].default is True
    p = inspect.signature(gp.BCM.predict_grad).parameters
    assert p["combine"].default is None and p["with_noise"].default is True
    assert callable(gp.poe_combine_grad)


# ------------------------------------------------------------------ refusals, all before any device call
def test_refusals():
    lib = capi.lib()
    null = C.c_void_p()
    fake = C.c_void_p(1)                                  # never dereferenced: every check below fails on an argument first
    Xt = np.zeros((3, 2))
    m, v, dm, dv = np.empty(3), np.empty(3), np.empty((3, 2)), np.empty((3, 2))
    assert lib.cugp_predict_grad(null, ptr(Xt), 3, 1, ptr(m), ptr(v), ptr(dm), ptr(dv)) == capi.CUGP_ERR_INVALID
    assert b"cugp_predict_grad" in lib.cugp_last_error()
    assert lib.cugp_predict_grad(fake, None, 3, 1, ptr(m), ptr(v), ptr(dm), ptr(dv)) == capi.CUGP_ERR_INVALID
    for nt in (0, -4):
        assert lib.cugp_predict_grad(fake, ptr(Xt), nt, 1, ptr(m), ptr(v), ptr(dm), ptr(dv)) == capi.CUGP_ERR_INVALID
    assert lib.cugp_predict_grad(fake, ptr(Xt), 3, 1, ptr(m), ptr(v), None, None) == capi.CUGP_ERR_INVALID
    assert lib.cugp_bcm_predict_grad(null, ptr(Xt), 3, 0, 1, ptr(m), ptr(v), ptr(dm), ptr(dv)) == capi.CUGP_ERR_INVALID
    assert b"cugp_bcm_predict_grad" in lib.cugp_last_error()
    assert lib.cugp_bcm_predict_grad(fake, None, 3, 0, 1, ptr(m), ptr(v), ptr(dm), ptr(dv)) == capi.CUGP_ERR_INVALID
    assert lib.cugp_bcm_predict_grad(fake, ptr(Xt), 0, 0, 1, ptr(m), ptr(v), ptr(dm), ptr(dv)) == capi.CUGP_ERR_INVALID
    assert lib.cugp_bcm_predict_grad(fake, ptr(Xt), 3, 0, 1, ptr(m), ptr(v), None, None) == capi.CUGP_ERR_INVALID
    for mode in (-2, 4, 99):
        assert lib.cugp_bcm_predict_grad(fake, ptr(Xt), 3, mode, 1, ptr(m), ptr(v), ptr(dm), ptr(dv)) == capi.CUGP_ERR_INVALID
    # the host chain rule
    K, nt, d = 2, 3, 2
    em, ev = np.ones((K, nt)), np.ones((K, nt))
    edm, edv = np.zeros((K, nt, d)), np.zeros((K, nt, d))
    om, ov = np.empty((nt, d)), np.empty((nt, d))

    def call(mode=0, K=K, nt=nt, d=d, a=ptr(em), b=ptr(ev), c=ptr(edm), e=ptr(edv), f=ptr(om), g=ptr(ov)):
        return lib.cugp_poe_combine_grad(a, b, c, e, K, nt, d, mode, SF2, f, g)
    for mode in (-1, 0, 1, 2, 3):
        assert call(mode) == capi.CUGP_OK
    for mode in (-2, 4, 99):
        assert call(mode) == capi.CUGP_ERR_INVALID
    assert b"cugp_poe_combine_grad" in lib.cugp_last_error()
    for kw in (dict(K=0), dict(K=-1), dict(nt=0), dict(nt=-5), dict(d=0), dict(d=-1), dict(a=None), dict(b=None),
               dict(c=None), dict(e=None), dict(f=None), dict(g=None)):
        assert call(**kw) == capi.CUGP_ERR_INVALID, kw


def test_refusals_surface_as_check_errors():
    with pytest.raises(RuntimeError):
        gp.poe_combine_grad(np.ones((1, 2)), np.ones((1, 2)), np.zeros((1, 2, 1)), np.zeros((1, 2, 1)), 7, SF2)
    with pytest.raises(ValueError):
        gp.poe_combine_grad(np.ones((1, 2)), np.ones((1, 3)), np.zeros((1, 2, 1)), np.zeros((1, 2, 1)), "poe", SF2)
    with pytest.raises(ValueError):
        gp.poe_combine_grad(np.ones((1, 2)), np.ones((1, 2)), np.zeros((1, 2, 1)), np.zeros((1, 2, 1)), "robust", SF2)
    b = gp.BCM.__new__(gp.BCM)                            # no handle at all: the name is checked first
    b._h = None
    with pytest.raises(ValueError):
        b.predict_grad(np.zeros((1, 2)), combine="robust")


# ------------------------------------------------------------------ the arithmetic
def synthetic(K, nt, d, seed):
    """var_f,k in (0.02, 1] sf2, some experts exactly uninformative, means and gradients of both signs."""
    rng = np.random.default_rng(seed)
    v = SF2 * rng.uniform(0.02, 1.0, (K, nt))
    v[rng.uniform(size=(K, nt)) < 0.15] = SF2
    m = rng.standard_normal((K, nt))
    return m, v, rng.standard_normal((K, nt, d)), 0.3 * rng.standard_normal((K, nt, d))


def longdouble_truth(m, v, dm, dv, mode):
    """-> (dmean, dvar, bound on |dmean error| / (c u), bound on |dvar error| / (c u)) in longdouble (module docstring)."""
    m, v, dm, dv = (np.asarray(a).astype(LD) for a in (m, v, dm, dv))
    K = len(v)
    sf2 = LD(SF2)
    p = 1 / v
    db = np.zeros_like(dv)
    if mode == "gpoe":
        beta = np.full_like(p, LD(1) / LD(K))
    elif mode == "rbcm":
        beta = LD(0.5) * np.log(sf2 * p)
        db = -LD(0.5) * dv / v[..., None]
    else:
        beta = np.ones_like(p)
    delta = 1 if mode == "rbcm" else 0
    prior = mode in ("bcm", "rbcm")
    ab = (np.abs(beta) + delta)[..., None]
    sb = beta.sum(0)
    prec = (beta * p).sum(0) + ((1 - sb) / sf2 if prior else 0)
    A = ((np.abs(beta) + delta) * p).sum(0) + ((np.abs(1 - sb) + K * delta) / sf2 if prior else 0)
    S, MS = (beta * p * m).sum(0), ((np.abs(beta) + delta) * np.abs(p * m)).sum(0)
    dp = -dv / (v * v)[..., None]
    pm = (p * m)[..., None]
    dprec = (db * p[..., None] + beta[..., None] * dp).sum(0) - (db.sum(0) / sf2 if prior else 0)
    D = (np.abs(db) * p[..., None] + ab * np.abs(dp)).sum(0) + (np.abs(db).sum(0) / sf2 if prior else 0)
    dS = (db * pm + beta[..., None] * dp * m[..., None] + (beta * p)[..., None] * dm).sum(0)
    E = (np.abs(db * pm) + ab * (np.abs(dp * m[..., None]) + p[..., None] * np.abs(dm))).sum(0)
    pr, cond = prec[:, None], (A / prec)[:, None]
    dvar = -dprec / (pr * pr)
    dmean = dvar * S[:, None] + dS / pr
    Bv = D / (pr * pr) + 2 * cond * np.abs(dprec) / (pr * pr)
    Bm = cond * (E + D * (MS / prec)[:, None]) / pr
    return dmean, dvar, Bm, Bv


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("K,nt,d", [(K, nt, d) for K in (1, 2, 3, 16) for nt in (1, 5) for d in (1, 3)])
def test_combine_grad_against_longdouble(K, nt, d, mode):
    m, v, dm, dv = synthetic(K, nt, d, 1000 * K + 10 * nt + d)
    if mode == "reference":
        v = v + SN2
    tdm, tdv, Bm, Bv = longdouble_truth(m, v, dm, dv, mode)
    cv, cm = (2 * K + 16) * U, (6 * K + 32) * U
    odm, odv = gp.poe_combine_grad(m, v, dm, dv, mode, SF2)
    em, ev = np.abs(odm.astype(LD) - tdm), np.abs(odv.astype(LD) - tdv)
    print("COMBINE-GRAD K%-2d nt%d d%d %-9s dvar err/bound %.3f  dmean err/bound %.3f" % (
        K, nt, d, mode, float(np.max(ev / (cv * Bv))), float(np.max(em / (cm * Bm)))))
    assert np.all(ev <= cv * Bv) and np.all(em <= cm * Bm)


def test_longdouble_chain_rule_agrees_with_the_truth_module():
    """The restatement above and tests/truth_predict_grad.py: combine_grad (checked against central differences in
    tests/test_truth_predict_grad_cpu.py) are the same function."""
    import truth_predict_grad as tpg
    m, v, dm, dv = (np.asarray(a).astype(LD) for a in synthetic(3, 5, 3, 2))
    for mode in MODES:
        a = longdouble_truth(m, v, dm, dv, mode)[:2]
        b = tpg.combine_grad(m, v, dm, dv, mode, LD(SF2))
        for x, y in zip(a, b):
            assert float(np.max(np.abs(x - y) / np.max(np.abs(y)))) <= 1e-17


def test_one_expert_poe_returns_its_gradients():
    m, v, dm, dv = synthetic(1, 5, 3, 3)
    for mode in ("poe", "reference"):
        odm, odv = gp.poe_combine_grad(m, v, dm, dv, mode, SF2)
        assert ulps(odv, dv[0]) <= 2 and ulps(odm, dm[0]) <= 2


def test_zero_gradients_in_zero_gradients_out():
    m, v, dm, dv = synthetic(3, 5, 3, 4)
    for mode in MODES:
        odm, odv = gp.poe_combine_grad(m, v, np.zeros_like(dm), np.zeros_like(dv), mode, SF2)
        assert np.all(odm == 0) and np.all(odv == 0)


@pytest.mark.parametrize("K", (2, 3, 16))
def test_gpoe_of_equal_experts_returns_one_expert(K):
    """K equal experts with weight 1 / K each: prec = p, S = p m, so dvar = dv and dmean = dm.  The K-term sums of equal
    terms and RN(1 / K) leave a few roundings each: the derived bound of test_combine_grad_against_longdouble, whose
    A / prec = 1 here."""
    m, v, dm, dv = synthetic(1, 5, 3, 5)
    rep = lambda a: np.repeat(a, K, axis=0)
    odm, odv = gp.poe_combine_grad(rep(m), rep(v), rep(dm), rep(dv), "gpoe", SF2)
    _, _, Bm, Bv = longdouble_truth(rep(m), rep(v), rep(dm), rep(dv), "gpoe")
    cv, cm = (2 * K + 16) * U, (6 * K + 32) * U
    assert np.all(np.abs(odv.astype(LD) - dv[0]) <= cv * Bv) and np.all(np.abs(odm.astype(LD) - dm[0]) <= cm * Bm)
    assert np.allclose(odv, dv[0], rtol=1e-10, atol=1e-12) and np.allclose(odm, dm[0], rtol=1e-10, atol=1e-12)
