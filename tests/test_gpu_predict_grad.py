"""Gradients of the predictive mean and variance with respect to the test inputs (include/cugp.h: cugp_predict_grad,
cugp_bcm_predict_grad) on the GPU, held to fp64 rounding against the longdouble truth of tests/truth_predict_grad.py:

    err <= F_family max(yardstick, floor)

yardstick: the family's fp64 evaluator's alpha, the reference-order Cholesky factor and two substitutions for V, the sums in
fp64 numpy, over the data as given and 7 row permutations; floor: 4 ulp of the largest true entry; F: truth.F / F_MATERN /
F_ARD -- tests/test_truth_predict_grad_cpu.py shows on the CPU that the stand-in stays below half of them on this very case
list and that the coordinate form exceeds the bound.

Shapes (tests/truth_predict_grad.py: CASES): one training tile with identity padding and the boundary at 64, two and more
training tiles, ragged n, two and three feature chunks, ill conditioning, |x| >> |x - x'|; 64 test points, then 129 and 200
(a second 128-row tile, passes of 64).  Every figure is printed before it is asserted (run with -s).  One process, one
device; nothing outside the tree is read.
"""
import numpy as np
import pytest

import truth
import truth_poe_modes as tpm
import truth_predict_grad as tpg
from accuracy import Report
from cugp_amd import capi

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not truth.EXTENDED, reason="numpy.longdouble is not an extended-precision type here")]

LD = truth.LD
TUNE_PRED_CHUNK = 19                                                # kernels.h TUNE_*
BITWISE = ("poe", "gpoe", "bcm", "reference")                      # no transcendental: host and device agree bit for bit


@pytest.fixture(scope="module")
def gp_mod():
    import cugp_amd.gp as gp
    return gp


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def make_handle(gp_mod, family, c):
    """A fresh handle of the family holding the case's data and hyper-parameters, nothing evaluated."""
    n, d = c["X"].shape
    g = gp_mod.Covsum(n, d, 0, ard=True) if family == "ard" else gp_mod.Covsum(n, d, 0, kernel=family)
    g.set_loghyperparam(c["cov"].hp)
    g.set_data(c["X"], c["y"])
    return g


@pytest.mark.parametrize("family,name", tpg.CASE_LIST)
def test_accuracy(gp_mod, oracle, family, name):
    """dmean and dvar of a case against the truth at the bound; mean / var carry the bits of the existing predictions for
    with_noise True / False; the gradients do not depend on with_noise; want_var_grad=False returns the same dmean bits."""
    c = tpg.case(oracle, family, name)
    X, y, Xt = c["X"], c["y"], c["Xt"]
    rep = Report("grad/%s/%s" % (family, name), c["cov"])
    g = make_handle(gp_mod, family, c)
    try:
        m, v, dm, dv = g.predict_grad(Xt)
        assert dm.shape == dv.shape == Xt.shape
        tpg.hold(rep, c, dm, dv)
        mp, vp = g.compute_test_means_and_variances(X, y, Xt)
        assert same_bits(m, mp) and same_bits(v, vp)
        ml, vl, dml, dvl = g.predict_grad(Xt, with_noise=False)
        mq, vq = g.predict_latent(Xt)
        assert same_bits(ml, mq) and same_bits(vl, vq)
        assert same_bits(dml, dm) and same_bits(dvl, dv)
        mo, vo, dmo, none = g.predict_grad(Xt, want_var_grad=False)
        assert none is None and same_bits(dmo, dm) and same_bits(mo, m) and same_bits(vo, v)
        # the test point that IS a training row: finite, and inside the bound on its own
        row = 5
        assert np.array_equal(Xt[row], X[len(X) // 2])
        assert np.all(np.isfinite(dm[row])) and np.all(np.isfinite(dv[row]))
        e = tpg.errors(dm[row], dv[row], c["tdm"][row], c["tdv"][row])
        for q in tpg.QUANTITIES:
            rep.add("training_row_" + q, e[q], c["noise"][q], c["floor"][q], tpg.factor(c["cov"]))
    finally:
        g.close()
    rep.check()


@pytest.mark.parametrize("nt", tpg.WIDE_NTS)
@pytest.mark.parametrize("family,name", tpg.WIDE_CASES)
def test_wide_and_passes(gp_mod, oracle, family, name, nt):
    """Two 128-row test tiles, held to the same bound; at nt = 200 passes of 64 test points (tuning key 19 = 1: four passes,
    t0 > 0) give the bits of the default single pass."""
    c = tpg.wide_case(oracle, family, name, nt)
    Xt = c["Xt"]
    rep = Report("grad/%s/%s/nt%d" % (family, name, nt), c["cov"])
    g = make_handle(gp_mod, family, c)
    try:
        m, v, dm, dv = g.predict_grad(Xt)
        tpg.hold(rep, c, dm, dv)
        if nt == 200:
            g.set_tuning(TUNE_PRED_CHUNK, 1)
            assert g.get_tuning(TUNE_PRED_CHUNK) == 1
            got = g.predict_grad(Xt)
            assert all(same_bits(a, b) for a, b in zip(got, (m, v, dm, dv)))
            got = g.predict_grad(Xt, want_var_grad=False)
            assert same_bits(got[2], dm)
    finally:
        g.close()
    rep.check()


@pytest.mark.parametrize("family,name", tpg.WIDE_CASES)
def test_rows_are_independent_and_bits_repeat(gp_mod, oracle, family, name):
    """Row t of a 200-point call equals the 1-point call at that point, bit for bit; two calls give equal bits; the bits
    are the same before and after get_K_inverse(), and on a handle that has only run compute_loglikelihood.

    That last handle reaches its L^-1 by continuing from the valid factor, which the library promises to equal the combined
    evaluation's to rounding only (tests/test_gpu_parity.py: test_gradient_continues_from_a_valid_factor).  So its call is
    held to what the new path can promise: mean / var are the bits of that handle's own cugp_predict (one path, whatever
    the handle held), the bits repeat and do not move with get_K_inverse(); and where that handle's cugp_predict agrees bit
    for bit with the first handle's -- the same L^-1 -- all four results do too, else the gradients are held to the bound."""
    c = tpg.wide_case(oracle, family, name, 200)
    Xt = c["Xt"]
    rep = Report("grad/%s/%s/ll-only-handle" % (family, name), c["cov"])
    g = make_handle(gp_mod, family, c)
    h = make_handle(gp_mod, family, c)
    try:
        ref = g.predict_grad(Xt)
        assert all(same_bits(a, b) for a, b in zip(g.predict_grad(Xt), ref))
        for t in (0, 63, 64, 127, 128, 198, 199):
            one = g.predict_grad(Xt[t: t + 1])
            assert all(same_bits(a[0], b[t]) for a, b in zip(one, ref)), t
        two = [np.concatenate(p) for p in zip(g.predict_grad(Xt[:128]), g.predict_grad(Xt[128:]))]
        assert all(same_bits(a, b) for a, b in zip(two, ref))
        g.get_K_inverse()
        assert all(same_bits(a, b) for a, b in zip(g.predict_grad(Xt), ref))
        h.compute_loglikelihood()
        got = h.predict_grad(Xt)                                    # (a stale handle is evaluated first: the continuation)
        own = h.compute_test_means_and_variances(None, None, Xt)
        assert same_bits(got[0], own[0]) and same_bits(got[1], own[1])
        assert all(same_bits(a, b) for a, b in zip(h.predict_grad(Xt), got))
        h.get_K_inverse()
        assert all(same_bits(a, b) for a, b in zip(h.predict_grad(Xt), got))
        same_inverse = same_bits(own[0], ref[0]) and same_bits(own[1], ref[1])
        print("LL-ONLY %-9s %-10s the continuation's prediction has the combined evaluation's bits: %s" % (family, name, same_inverse))
        if same_inverse:
            assert all(same_bits(a, b) for a, b in zip(got, ref))
        else:
            tpg.hold(rep, c, got[2], got[3])
    finally:
        g.close()
        h.close()
    rep.check()


@pytest.mark.parametrize("family,name", [("se", "n65"), ("matern32", "n65"), ("matern52", "n300_d17"), ("ard", "n65_d2")])
def test_far_from_the_data(gp_mod, oracle, family, name):
    """A point 1e3 length scales from all data: the cross-covariances are exact zeros (and below 1e-1000 in any precision),
    so both gradients are exactly 0 or below the floor, and never NaN."""
    c = tpg.case(oracle, family, name)
    d = c["X"].shape[1]
    ell = np.exp(np.max(c["cov"].hp[:-2]))
    Xt = np.full((1, d), float(np.max(np.abs(c["X"])) + 1e3 * ell))
    g = make_handle(gp_mod, family, c)
    try:
        _, _, dm, dv = g.predict_grad(Xt)
        print("FAR %-9s %-10s dmean %s dvar %s" % (family, name, np.max(np.abs(dm)), np.max(np.abs(dv))))
        assert not np.any(np.isnan(dm)) and not np.any(np.isnan(dv))
        assert np.all(np.abs(dm) <= c["floor"]["dmean"]) and np.all(np.abs(dv) <= c["floor"]["dvar"])
    finally:
        g.close()


@pytest.mark.parametrize("family,name", [("se", "n257_d3"), ("matern52", "n300_d17"), ("ard", "n257_d3")])
def test_existing_results_untouched(gp_mod, oracle, family, name):
    """LL, gradient, predict, predict_latent and the joint covariance give equal bits before and after a predict_grad call on
    the same handle."""
    c = tpg.case(oracle, family, name)
    X, y, Xt = c["X"], c["y"], c["Xt"]

    def existing(g):
        ll, gr = g.loglik_grad(X, y)
        return (np.array([ll]), gr) + g.compute_test_means_and_variances(X, y, Xt) + g.predict_latent(Xt) \
            + g.compute_test_joint(X, y, Xt)
    g = make_handle(gp_mod, family, c)
    try:
        before = existing(g)
        g.predict_grad(Xt)
        g.predict_grad(Xt, with_noise=False, want_var_grad=False)
        after = existing(g)
        assert all(same_bits(a, b) for a, b in zip(before, after))
    finally:
        g.close()


def test_staleness_and_refusals(gp_mod, oracle):
    """After set_loghyperparam or set_data the gradients follow without an explicit evaluation: the bits of a fresh handle
    at that point.  Refusals surface as check() errors and leave the handle usable."""
    c = tpg.case(oracle, "se", "n257_d3")
    X, y, Xt = c["X"], c["y"], c["Xt"]
    g = make_handle(gp_mod, "se", c)
    try:
        first = g.predict_grad(Xt)
        hp2 = [h + 0.1 for h in c["cov"].hp]
        g.set_loghyperparam(hp2)
        moved = g.predict_grad(Xt)
        assert not same_bits(moved[2], first[2])
        f = gp_mod.Covsum(*X.shape, 0)
        f.set_loghyperparam(hp2)
        f.set_data(X, y)
        assert all(same_bits(a, b) for a, b in zip(f.predict_grad(Xt), moved))
        y2 = y[::-1].copy()
        g.set_data(X, y2)
        f.set_data(X, y2)
        again = g.predict_grad(Xt)
        assert not same_bits(again[2], moved[2]) and same_bits(again[3], moved[3])     # (the variance does not see y)
        assert all(same_bits(a, b) for a, b in zip(f.predict_grad(Xt), again))
        f.close()
        with pytest.raises(capi.CugpError):
            g.predict_grad(np.empty((0, X.shape[1])))
        null = gp_mod.Covsum.__new__(gp_mod.Covsum)
        null._h, null.d, null.close = None, X.shape[1], lambda: None
        with pytest.raises(capi.CugpError):
            null.predict_grad(Xt)
        assert all(same_bits(a, b) for a, b in zip(g.predict_grad(Xt), again))
    finally:
        g.close()


# ------------------------------------------------------------------ the product of experts
def make_bcm(gp_mod, c, name, **kw):
    family = tpm.CASES[name][0]
    b = gp_mod.BCM.split(c["X"], c["y"], c["K"], kernel="se" if family == "ard" else family, ard=family == "ard", **kw)
    b.set_BCM_log_hyperparam(c["cov"].hp)
    return b


@pytest.mark.parametrize("name", tpg.BCM_CASES)
def test_bcm(gp_mod, oracle, name):
    """cugp_bcm_predict_grad at 200 points in every mode and for the reference product: the gradients against the experts'
    truths through the longdouble chain rule at the bound; mean / var against BCM.predict(Xt, combine=): bit for bit except
    rbcm (each side's own log), which is held to the combination's own bound."""
    c = tpg.bcm_case(oracle, name)
    pc = tpm.case(oracle, name, tpg.BCM_NT)
    Xt, cov = c["Xt"], c["cov"]
    F = tpg.factor(cov)
    rep = Report("grad-bcm/%s" % name, cov)
    b = make_bcm(gp_mod, c, name)
    try:
        for mode in tpg.BCM_MODES:
            combine = None if mode == "reference" else mode
            m, v, dm, dv = b.predict_grad(Xt, combine=combine, with_noise=False)
            t = c["modes"][mode]
            e = tpg.errors(dm, dv, t["tdm"], t["tdv"])
            for q in tpg.QUANTITIES:
                rep.add("%s_%s" % (mode, q), e[q], t["noise"][q], t["floor"][q], F)
            pm, pv = b.predict(Xt, combine=combine, with_noise=False)
            if mode in BITWISE:
                assert same_bits(m, pm) and same_bits(v, pv), mode
            else:
                fl = tpm.floors(pc, mode)
                rep.add("rbcm_host_vs_device_mean", np.max(np.abs(m - pm)), pc["yard"][mode]["mean"], fl["mean"], F)
                rep.add("rbcm_host_vs_device_var", np.max(np.abs(v - pv)), pc["yard"][mode]["var"], fl["var"], F)
            if combine is not None:
                mn, vn, dmn, dvn = b.predict_grad(Xt, combine=combine, with_noise=True)
                assert same_bits(mn, m) and same_bits(vn, v + b.prior_scalars()[1]) and same_bits(dmn, dm) and same_bits(dvn, dv)
    finally:
        b.close()
    rep.check()


def test_bcm_over_two_device_sets(gp_mod, oracle):
    """The same GPU listed twice: two device sets of one process give the bits of one."""
    name = "se_5x261p2"
    c = tpg.bcm_case(oracle, name)
    one, two = make_bcm(gp_mod, c, name), make_bcm(gp_mod, c, name, devices=[0, 0])
    try:
        for combine in (None, "rbcm"):
            a, b = one.predict_grad(c["Xt"], combine=combine), two.predict_grad(c["Xt"], combine=combine)
            assert same_bits(a[2], b[2]) and same_bits(a[3], b[3])
    finally:
        one.close()
        two.close()
