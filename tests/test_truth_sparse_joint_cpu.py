"""The truth, the yardstick, the stand-in and the factor of the sparse model's joint covariance and input gradients
(tests/truth_sparse_joint.py), and the schedule cugp_sparse_predict_cov_plan reports -- CPU, no GPU.  What the GPU tests
(tests/test_gpu_sparse_joint.py) are held by is established here: the gradient truth agrees with central differences of the
truth's own prediction in longdouble; the covariance truth is symmetric, has the truth's latent variances on its diagonal and
is positive definite at the cases; the yardsticks are sane and below truth_sparse_joint.YARDSTICK_LIMIT; the library's
formulation in numpy (the stand-in) stays within the factor on every case, and truth.factor_rule of its largest ratio per
family is what the factor is checked against; three mutations of that formulation land far outside the bound."""
import ctypes as C

import numpy as np
import pytest

import truth
import truth_sparse as ts
import truth_sparse_joint as tj
from cugp_amd import capi

LD = truth.LD
TUNE_COV_SPLIT, COV_SPLIT_DEFAULT = 20, 1024      # kernels.h TUNE_COV_SPLIT and its built-in default (kernels.hip: g_tune_init)
pytestmark = pytest.mark.skipif(np.finfo(LD).eps > 2.0 ** -60, reason="no extended-precision long double on this host")
IDS = ["%s-%s" % (n, "nt%d" % nt if nt else "own") for n, nt in tj.ALL_CASES]


def test_cases_are_the_issues():
    assert {tj.case_row(n)[0] for n in tj.FAMILY_CASES} == set(ts.F_SPARSE)            # one case per family
    assert tj.WIDE_NTS == (129, 200, 257) and tj.WIDE_NAMES == ts.WIDE_NAMES
    assert tj.OWN_CASES[tj.SPLIT_NAME] == ("se", 600, 400, 6, 0, truth.HP_A, 2.5, False)
    for name in tj.WIDE_NAMES + (tj.SPLIT_NAME,):
        X, _, Z, _, _, _ = tj.inputs(name)
        Xt = tj.wide_points(name, 129)
        assert np.array_equal(Xt[128], Z[0]) and np.array_equal(Xt[-2], X[len(X) // 2])  # an inducing input, a data row


@pytest.mark.parametrize("name", tj.FAMILY_CASES)
def test_gradient_truth_against_central_differences(name):
    """d mean / d x and d var / d x of the truth's own prediction by central differences in longdouble, h = 1e-6: the
    truncation error is h^2 f''' / 6 ~ 1e-12 and the rounding error eps_LD / h ~ 1e-13 of the function's scale, so 1e-8 of
    the largest gradient entry is far above both and far below any error of the formula (a wrong sign or factor is 1).  A
    Matern 3/2 kernel has a kink in its gradient at distance 0: its rows that ARE an inducing input are left out."""
    m = tj.model(name)
    t, Xt = m["t"], np.asarray(m["Xt"], dtype=LD)
    _, tdm, tdv = tj.truth_at(t, Xt)
    keep = np.ones(len(Xt), dtype=bool)
    if "matern32" in m["family"]:
        keep = np.array([np.min(np.abs(x - t.Zl).sum(1)) > 0 for x in Xt])
        assert keep.sum() >= len(Xt) - 2
    h = LD(1e-6)
    for c in range(Xt.shape[1]):
        Xp, Xm = Xt.copy(), Xt.copy()
        Xp[:, c] += h
        Xm[:, c] -= h
        mp, vp = tj.truth_predict(t, Xp)
        mm, vm = tj.truth_predict(t, Xm)
        em = np.max(np.abs((mp - mm) / (2 * h) - tdm[:, c])[keep]) / np.max(np.abs(tdm))
        ev = np.max(np.abs((vp - vm) / (2 * h) - tdv[:, c])[keep]) / np.max(np.abs(tdv))
        assert em < 1e-8 and ev < 1e-8, (name, c, float(em), float(ev))


@pytest.mark.parametrize("name, nt", tj.ALL_CASES, ids=IDS)
def test_covariance_truth(name, nt):
    c = tj.case(name, nt)
    tc, scale = c["tc"], float(c["cov"].sf2)
    eps = float(np.finfo(LD).eps)
    # symmetric up to the rounding of the two orders of summation in longdouble: M eps_LD of the terms' size |Ks||D||Ks'|
    M, dmax = c["t"].D.shape[0], float(np.max(np.abs(c["t"].D)))
    print("SYM %-26s %-5s asym %.2e of %.2e" % (name, nt, float(np.max(np.abs(tc - tc.T))), M * eps * dmax * scale * scale))
    assert float(np.max(np.abs(tc - tc.T))) <= M * eps * dmax * scale * scale
    assert float(np.max(np.abs(np.diag(tc) - c["tvar"]))) <= 1e-16 * scale                # Truth.predict's latent variance
    assert float(np.linalg.eigvalsh(((tc + tc.T) / 2).astype(np.float64)).min()) > 0


@pytest.mark.parametrize("name, nt", tj.ALL_CASES, ids=IDS)
def test_yardstick_is_sane(name, nt):
    c = tj.case(name, nt)
    print("YARD %-26s %-5s %s" % (name, nt, {q: "%.2e" % c["noise"][q] for q in tj.QUANTITIES}))
    tj.assert_yardstick_is_sane(c, (name, nt))


_RATIOS = {}


def standin_ratios(name, nt):
    """The stand-in's ratios on a case, once per process."""
    if (name, nt) not in _RATIOS:
        c = tj.case(name, nt)
        _RATIOS[name, nt] = tj.ratios(c, *tj.standin(c["cov"], c["X"], c["y"], c["Z"], c["Xt"], c["chunk"]))
    return _RATIOS[name, nt]


@pytest.mark.parametrize("name, nt", tj.ALL_CASES, ids=IDS)
def test_standin_within_the_factor(name, nt):
    c = tj.case(name, nt)
    r = standin_ratios(name, nt)
    print("STANDIN %-26s %-5s plan %s %s" % (name, nt, tj.cov_plan(len(c["Z"]), c["nt"]), {q: "%.2f" % r[q] for q in r}))
    assert max(r.values()) <= tj.factor(c["family"]), r


def test_the_factor_is_the_rules():
    """truth.factor_rule of the largest stand-in ratio of a family over all cases is at most the factor the GPU is held to
    -- F_SPARSE[family], or F_SPARSE_JOINT where that is set, which must then BE the rule's value."""
    worst = {}
    for name, nt in tj.ALL_CASES:
        family = tj.case_row(name)[0]
        worst[family] = max(worst.get(family, 0.0), max(standin_ratios(name, nt).values()))
    assert set(worst) == set(ts.F_SPARSE)
    for family, w in worst.items():
        print("FACTOR %-14s largest stand-in ratio %.2f  rule %d  factor %d" % (family, w, truth.factor_rule(w), tj.factor(family)))
        assert truth.factor_rule(w) <= tj.factor(family), (family, w)
        if family in tj.F_SPARSE_JOINT:
            assert tj.F_SPARSE_JOINT[family] == truth.factor_rule(w) > ts.F_SPARSE[family]


@pytest.mark.parametrize("name, nt", [("se_n1300_m200", None), ("matern32_ard_n1000_m130", 200), (tj.SPLIT_NAME, 129)])
@pytest.mark.parametrize("mutate, q", zip(tj.MUTATIONS, ("cov", "dvar", "cov")))
def test_mutations_are_far_outside(name, nt, mutate, q):
    """+ Vt Vt' dropped, U without its LB term, eps on the diagonal: each at least 1000 bounds away on its quantity."""
    c = tj.case(name, nt)
    r = tj.ratios(c, *tj.standin(c["cov"], c["X"], c["y"], c["Z"], c["Xt"], c["chunk"], mutate=mutate))
    print("MUTATION %-14s %-26s %s" % (mutate, name, {k: "%.3g" % v for k, v in r.items()}))
    assert r[q] > 1000 * tj.factor(c["family"]), (mutate, r)


# ------------------------------------------------------------------ the schedule
def plan(m, nt):
    out = (C.c_int * 4)()
    return capi.lib().cugp_sparse_predict_cov_plan(m, nt, out), tuple(out)


@pytest.fixture
def tuning():
    yield lambda v: capi.check(capi.lib().cugp_set_tuning(TUNE_COV_SPLIT, v))
    capi.check(capi.lib().cugp_set_tuning(TUNE_COV_SPLIT, COV_SPLIT_DEFAULT))


def test_plan_default_splits_the_case_of_its_own():
    rc, (ntpad, edge, split, kstep) = plan(400, 129)
    assert rc == 0 and (ntpad, edge, split, kstep) == (256, 64, 2, 256)
    assert plan(400, 257) == (0, (384, 64, 2, 256)) and plan(260, 129) == (0, (256, 64, 1, 384))    # (mpad 384: below two chunks of 256)


@pytest.mark.parametrize("m, nt", [(16, 1), (65, 129), (260, 257), (400, 129), (400, 257), (2048, 1000), (32768, 128)])
def test_plan_every_k_in_exactly_one_split(tuning, m, nt):
    """At the built-in tuning and at the forms of the tuning key: the ranges [s kstep, min((s + 1) kstep, mpad)) ascend,
    are not empty, are whole stages of 16, and cover [0, mpad) exactly once."""
    mpad = (m + 127) // 128 * 128
    seen = set()
    for v in (None, 0, 8, 256, 4096, 1 << 20):
        if v is not None:
            tuning(v)
        rc, (ntpad, edge, split, kstep) = plan(m, nt)
        assert rc == 0 and ntpad == (nt + 127) // 128 * 128 and edge in (64, 128) and split >= 1
        if v == 0:
            assert (edge, split) == (128, 1)
        assert kstep % 16 == 0 and (split - 1) * kstep < mpad <= split * kstep
        cover = np.zeros(mpad, dtype=int)
        for s in range(split):
            cover[s * kstep: min((s + 1) * kstep, mpad)] += 1
        assert np.all(cover == 1)
        seen.add((edge, split > 1))
    if m >= 400 and nt <= 257:
        assert {(64, True), (128, False)} <= seen


def test_plan_refusals():
    L = capi.lib()
    INV = capi.CUGP_ERR_INVALID
    for m, nt in ((16, 32769), (16, 349441), (2048, 21761), (0, 10), (32769, 10), (16, 0), (16, -1)):
        rc, out = plan(m, nt)
        assert rc == INV and b"cugp_sparse_predict_cov_plan" in L.cugp_last_error() and out == (0, 0, 0, 0), (m, nt)
    assert L.cugp_sparse_predict_cov_plan(16, 10, None) == INV and b"cugp_sparse_predict_cov_plan" in L.cugp_last_error()
    # one row fewer is taken: the cap, and the last row of the first prediction pass at mpad 2048
    assert plan(16, 32768)[0] == 0 and plan(2048, 21760)[0] == 0
    out2 = (C.c_int * 2)()
    assert L.cugp_sparse_predict_plan(2048, 21761, 0, out2) == 2 and L.cugp_sparse_predict_plan(16, 349441, 0, out2) == 2
