"""Below one 64-row build tile: what the case lists of the other GPU modules do not reach at n = 1, 2, 63, 64.

Whole 64 x 64 tiles of the padded matrix are padding there (the lower tiles tri_index enumerates in the trace, mirror and
outer-product passes among them), a reduction has one or two live lanes, an expert's own n in a batched launch is far from
its neighbours', and at n = 1 every off-diagonal sum is empty.  The small cases of truth.LIVE_CASES, ARD_CASES, truth_loo,
truth_targets, truth_predict_grad and truth_append run in those modules' own GPU tests; here:

  1. every family's single handle at n1, n2, n63, n64 through accuracy.hold_live_case WITH the joint covariance, and the
     prediction at one test point;
  2. the exact facts of n = 1;
  3. the LOO optimiser's first evaluation, and a LOO evaluation behind cugp_append;
  4. products of experts with explicit small expert sizes (tests/truth_small_bcm.py): LL, gradient, prediction at 64 points
     and at one, the combination rules, cugp_bcm_predict_grad, and the batched group against the same experts one by one.

Every bound is F max(yardstick, floor) of the family as it stands (tests/accuracy.py); every figure is printed before it is
asserted.  The CPU counterparts: tests/test_truth_small_bcm_cpu.py and the families' own test_truth_*_cpu.py."""
import math

import numpy as np
import pytest

import accuracy
import truth
import truth_append as ta
import truth_loo as tl
import truth_poe_modes as tpm
import truth_predict_grad as tpg
import truth_small_bcm as tsb
from accuracy import Report

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not truth.EXTENDED, reason="numpy.longdouble is not an extended-precision type here")]

LD = truth.LD
GROUP_OVERLAP, GROUP_MAX_TILES = 6, 7                               # kernels.h TUNE_*, as tests/test_gpu_launch_paths.py
BITWISE = ("poe", "gpoe", "bcm", "reference")                      # no transcendental: host and device agree bit for bit
ISO = ("se", "matern32", "matern52")
ARD = ("ard", "matern32_ard", "matern52_ard")
SINGLE = [(f, n) for f in ISO for n in ("n1", "n2", "n63", "n64")] + [(f, n + "_d2") for f in ARD for n in ("n1", "n2", "n63", "n64")]


@pytest.fixture(scope="module")
def gp_mod():
    import cugp_amd.gp as gp
    return gp


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def make(gp_mod, family, X, y, hp, overlap=None, npad_min=0):
    """A handle of the family with data and hyper-parameters set."""
    g = gp_mod.Covsum(X.shape[0], X.shape[1], npad_min=npad_min, ard=family == "ard",
                      kernel=family if family.startswith("matern") else "se")
    if overlap is not None:
        g.set_overlap(overlap)
    g.set_data(X, y)
    g.set_loghyperparam(hp)
    return g


def ulps(got, want):
    """|got - want| in units of the spacing of want."""
    return abs(float(got) - float(want)) / np.spacing(abs(float(want)))


# ------------------------------------------------------------------ 1. single handles
@pytest.mark.parametrize("family, name", SINGLE, ids=["%s-%s" % c for c in SINGLE])
def test_single_handle(gp_mod, oracle, family, name):
    """The LL-only path on a fresh handle, loglik_grad, K^-1 exactly symmetric, alpha and every row of K^-1
    (solve_rows: min(64, n)), prediction at the 64 test points (nt > n), the joint covariance with and without noise --
    accuracy.hold_live_case -- and the prediction at ONE test point: the training row among the 64 and another one, held to
    the yardstick of the 64 (a maximum over points that include both)."""
    c = accuracy.live(oracle, family, name)
    X, y, Xt, cov = c["X"], c["y"], c["Xt"], c["cov"]
    rep = Report("small/%s/%s" % (family, name), cov)
    g = make(gp_mod, family, X, y, cov.hp)
    for row in (5, 0):
        m, v = g.compute_test_means_and_variances(X, y, Xt[row: row + 1])
        assert m.shape == v.shape == (1,)
        e = truth.errors_pred(m, v, c["tm"][row: row + 1], c["tv"][row: row + 1])
        rep.add("nt1_row%d_mean" % row, e["mean"], c["noise"]["mean"], c["floor"]["mean"])
        rep.add("nt1_row%d_var" % row, e["var"], c["noise"]["var"], c["floor"]["var"])
    g.close()
    accuracy.hold_live_case(rep, c, lambda overlap=None: make(gp_mod, family, X, y, cov.hp, overlap), joint=True)


# ------------------------------------------------------------------ 2. n = 1
@pytest.mark.parametrize("family", ISO + ARD)
def test_one_row_exact_facts(gp_mod, family):
    """K is the one entry sf2 + sn2.  The length-scale components of the gradient are exactly 0.0 (the only entry is a
    diagonal one: SE dk = kf * 0, Matern q = a * a = 0, ARD's diagonal has no share), K^-1 is 1 / (sf2 + sn2) and the factor
    sqrt(sf2 + sn2), each to 1 ulp (one division, one square root; sf2 + sn2 as the host forms it)."""
    X, y, _, cov = truth.family_inputs(family, "n1_d2" if family in ARD else "n1")
    g = make(gp_mod, family, X, y, cov.hp)
    ll, gr = g.loglik_grad()
    Ki, L, K = g.get_K_inverse(), g.get_cholesky(), g.compute_K_train()
    g.close()
    k = math.exp(2 * cov.hp[-2]) + math.exp(2 * cov.hp[-1])
    print("ACC small/%s/n1 grad %s  K %.17g (%.1f ulp)  K^-1 %.1f ulp  L %.1f ulp"
          % (family, gr, K[0, 0], ulps(K[0, 0], k), ulps(Ki[0, 0], 1 / k), ulps(L[0, 0], math.sqrt(k))))
    assert gr.shape == (len(cov.hp),) and np.isfinite(ll) and np.all(np.isfinite(gr))
    assert np.all(gr[:-2] == 0.0), gr
    assert K.shape == Ki.shape == L.shape == (1, 1) and K[0, 0] == k
    assert ulps(Ki[0, 0], 1 / k) <= 1 and ulps(L[0, 0], math.sqrt(k)) <= 1


# ------------------------------------------------------------------ 3. leave-one-out
LOO_SMALL = [c for c in tl.CASES if c[1].split("_")[0] in ("n1", "n2", "n63", "n64")]


@pytest.mark.parametrize("family, name", LOO_SMALL, ids=["%s-%s" % c for c in LOO_SMALL])
def test_loo_optimiser_first_evaluation(gp_mod, oracle, family, name):
    """cugp_cg_solve_loo with a budget of one: the first trace row is the start and -cugp_loo there, to the bit, and L_LOO
    meets the bound of tests/test_gpu_loo.py at that case."""
    c = tl.case(oracle, family, name)
    cov = c["cov"]
    g = make(gp_mod, family, c["X"], c["y"], cov.hp)
    lpl, _ = g.loo()
    tr = g.cg_solve_loo(1)
    g.close()
    assert tr.shape[1] == len(cov.hp) + 1 and tr.shape[0] >= 1 and np.array_equal(tr[0, :-1], np.asarray(cov.hp))
    assert same_bits([tr[0, -1]], [-lpl])
    rep = Report("small/loo-cg/%s/%s" % (family, name), cov)
    q = cov.quantities[0]
    rep.add(q, abs(LD(-tr[0, -1]) - c["tt"]["ll"]) / abs(c["tt"]["ll"]), c["noise"][q], c["floor"][q], tl.F_LOO[family])
    rep.check()


APPEND_SMALL = [c for c in ta.CASES if truth.family_inputs(c[0], c[1])[0].shape[0] <= 65 and c[0] in tl.F_LOO]


@pytest.mark.parametrize("case", APPEND_SMALL, ids=[ta.case_id(c) for c in APPEND_SMALL])
def test_loo_behind_an_append(gp_mod, oracle, case):
    """A handle grown by cugp_append to the case's rows, then cugp_loo and cugp_loo_predict: held to the bound of a fresh
    handle on all rows (tests/test_truth_small_bcm_cpu.py pins the stand-in of exactly this on the CPU)."""
    family, name, n0, chunks = case
    c = tl.case(oracle, family, name)
    X, y, cov = c["X"], c["y"], c["cov"]
    g = make(gp_mod, family, X[:n0], y[:n0], cov.hp, npad_min=len(y))
    g.loglik_grad()
    at = n0
    for k in chunks:
        g.append(X[at: at + k], y[at: at + k])
        at += k
    assert g.n == len(y)
    lpl, gr = g.loo()
    mu, var, logp = g.loo_predict()
    g.close()
    rep = Report("small/append-loo/" + ta.case_id(case), cov)
    tl.hold(rep, c, lpl, gr, mu, var, logp)
    rep.check()


# ------------------------------------------------------------------ 4. products of experts
def make_bcm(gp_mod, family, c, rname):
    """The case as a BCM with its hyper-parameters set: the two split rows through BCM.split, the rest by explicit rows."""
    kw = dict(kernel="se" if family == "ard" else family, ard=family == "ard")
    rows = list(tsb.ROWS[rname])
    if rname in tsb.SPLITS:
        b = gp_mod.BCM.split(c["X"], c["y"], tsb.SPLITS[rname][1], **kw)
    else:
        b = gp_mod.BCM(rows, tsb.D, **kw)
        for k, (o, r) in enumerate(c["parts"]):
            b.set_expert_data(k, c["X"][o: o + r], c["y"][o: o + r])
    assert b.rows == rows
    b.set_BCM_log_hyperparam(c["cov"].hp)
    return b


@pytest.mark.parametrize("family, rname", tsb.CASES, ids=[tsb.case_id(c) for c in tsb.CASES])
def test_bcm(gp_mod, oracle, family, rname):
    """Summed LL and gradient, the product-of-experts prediction at the 64 points and at one (the training row among them,
    and another), against the experts' truths combined in longdouble."""
    c = tsb.case(oracle, family, rname)
    cov, Xt = c["cov"], c["Xt"]
    rep = Report("small/bcm/%s/%s" % (family, rname), cov)
    b = make_bcm(gp_mod, family, c, rname)
    try:
        ll, g, per = b.loglik_grad()
        m, v = b.compute_BCM_test_means_and_var(Xt)
        assert g.shape == (len(cov.hp),) and per.shape == (c["K"],) and m.shape == v.shape == (len(Xt),)
        rep.add_all("", tsb.errors(c, ll, g, m, v), c["noise"], c["floor"])
        for row in (5, 0):
            m1, v1 = b.compute_BCM_test_means_and_var(Xt[row: row + 1])
            e = truth.errors_pred(m1, v1, c["tb"]["mean"][row: row + 1], c["tb"]["var"][row: row + 1])
            rep.add("nt1_row%d_mean" % row, e["mean"], c["noise"]["mean"], c["floor"]["mean"])
            rep.add("nt1_row%d_var" % row, e["var"], c["noise"]["var"], c["floor"]["var"])
    finally:
        b.close()
    rep.check()


@pytest.mark.parametrize("family, rname", tsb.MODES_CASES, ids=[tsb.case_id(c) for c in tsb.MODES_CASES])
def test_bcm_combination_rules(gp_mod, oracle, family, rname):
    """poe, gpoe, bcm and rbcm on the experts' latent predictions (the fifth rule, the reference's product, is test_bcm's
    prediction) and every expert's own latent prediction, at the bounds of tests/test_gpu_poe_modes.py."""
    c = tsb.modes_case(oracle, family, rname)
    cov, Xt = c["cov"], c["Xt"]
    F = tpm.factor(cov)
    rep = Report("small/modes/%s/%s" % (family, rname), cov)
    b = make_bcm(gp_mod, family, c, rname)
    try:
        sn2 = b.prior_scalars()[1]
        for k in range(c["K"]):
            ml, vl = b.expert(k).predict_latent(Xt)
            err = truth.errors_pred(ml, vl, *c["experts"][k])
            fl = tpm.expert_floors(c, k)
            for q in ("mean", "var"):
                rep.add("latent%d_%s" % (k, q), err[q], c["yard"]["experts"][k][q], fl[q], F)
        for mode in tpm.MODES:
            m, v = b.predict(Xt, combine=mode, with_noise=False)
            mn, vn = b.predict(Xt, combine=mode, with_noise=True)
            assert same_bits(mn, m) and same_bits(vn, v + sn2), mode
            e = truth.errors_pred(m, v, *c["modes"][mode])
            fl = tpm.floors(c, mode)
            for q in ("mean", "var"):
                rep.add("%s_%s" % (mode, q), e[q], c["yard"][mode][q], fl[q], F)
    finally:
        b.close()
    rep.check()


@pytest.mark.parametrize("family, rname", tsb.GRAD_CASES, ids=[tsb.case_id(c) for c in tsb.GRAD_CASES])
def test_bcm_predict_grad(gp_mod, oracle, family, rname):
    """cugp_bcm_predict_grad in every mode and for the reference product against the experts' truths through the longdouble
    chain rule; mean / var carry BCM.predict's bits where the rule has no transcendental.  The mixed group runs as one
    batch of launches (form 2), 2+300 expert by expert (form 1)."""
    c = tsb.grad_case(oracle, family, rname)
    cov, Xt = c["cov"], c["Xt"]
    rep = Report("small/grad-bcm/%s/%s" % (family, rname), cov)
    b = make_bcm(gp_mod, family, c, rname)
    try:
        for mode in tpg.BCM_MODES:
            combine = None if mode == "reference" else mode
            m, v, dm, dv = b.predict_grad(Xt, combine=combine, with_noise=False)
            assert b.predict_grad_form == (2 if rname == tsb.MIXED else 1)
            assert dm.shape == dv.shape == Xt.shape
            t = c["modes"][mode]
            e = tpg.errors(dm, dv, t["tdm"], t["tdv"])
            for q in tpg.QUANTITIES:
                rep.add("%s_%s" % (mode, q), e[q], t["noise"][q], t["floor"][q], tpg.factor(cov))
            if mode in BITWISE:
                pm, pv = b.predict(Xt, combine=combine, with_noise=False)
                assert same_bits(m, pm) and same_bits(v, pv), mode
    finally:
        b.close()
    rep.check()


def record(b, Xt):
    """One evaluation of the BCM away and one back: the experts' rows, factors and inverses, and the prediction."""
    hp = b.get_loghyperparam()
    b.set_BCM_log_hyperparam(hp + 0.125)
    b.loglik_grad_rows()
    b.set_BCM_log_hyperparam(hp)
    r = {"rows": b.loglik_grad_rows()}
    for k in range(len(b.rows)):
        e = b.expert(k)
        r["L%d" % k], r["Ki%d" % k], r["alpha%d" % k] = e.get_cholesky(), e.get_K_inverse(), e.get_alpha()
    r["mean"], r["var"] = b.compute_BCM_test_means_and_var(Xt)
    return r


@pytest.mark.parametrize("family", ["se", "matern52", "ard"])
@pytest.mark.parametrize("rname", tsb.GROUPED_ROWS)
def test_group_equals_the_experts_one_by_one(gp_mod, family, rname):
    """One batched group of experts of unlike n (tests/test_gpu_launch_paths.py: test_refused_group_equals_the_group at these
    sizes): with key 7 = 0 on the lead (no expert of even one tile shares launches) the group is refused and the experts run
    one by one -- the bits of the group with key 6 = 0, in every expert's row, factor, K^-1 and alpha and in the prediction; the default group meets them in L to the
    bit."""
    X, y, Xt, cov, parts = tsb.inputs(family, rname)
    b = make_bcm(gp_mod, family, dict(X=X, y=y, cov=cov, parts=parts), rname)
    try:
        default = record(b, Xt)
        b.expert(0).set_tuning(GROUP_OVERLAP, 0)
        grouped = record(b, Xt)
        b.expert(0).set_tuning(GROUP_MAX_TILES, 0)
        alone = record(b, Xt)
    finally:
        b.close()
    for key in alone:
        assert same_bits(alone[key], grouped[key]), (family, rname, key, np.max(np.abs(alone[key] - grouped[key])))
    for k in range(len(parts)):
        assert same_bits(alone["L%d" % k], default["L%d" % k]), (family, rname, k)
        assert alone["L%d" % k].shape == (parts[k][1],) * 2
