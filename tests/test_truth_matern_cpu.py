"""CPU checks of the Matern truth (truth.Truth with the truth.Matern descriptor), of its yardstick, of the factor
F_MATERN and of the K-entry bound (tests/truth_matern.py) -- everything tests/test_gpu_matern.py leans on.

  1. the closed forms of truth.matern_kernel against the general Matern expression through scipy.special.kv;
  2. the truth's gradient against a central difference of its LL in longdouble: the only independent check of the
     derivative formulas;
  3. F_MATERN = the next power of two at or above twice the largest stand-in ratio over the case list, both kinds;
  4. every case's yardstick under the cap;
  5. the kernels' per-entry arithmetic, restated in fp64 numpy, inside the K-entry bound against longdouble.
"""
import numpy as np
import pytest

import accuracy
import truth
import truth_matern as tm
from conftest import synth

pytestmark = pytest.mark.skipif(not truth.EXTENDED, reason="numpy.longdouble is not an extended-precision type here")

LD = truth.LD
EPS = 2.0 ** -52


@pytest.mark.parametrize("kind", tm.KINDS)
def test_closed_forms_agree_with_the_bessel_expression(kind):
    """k(r) = sf2 2^(1 - nu) / Gamma(nu) a^nu K_nu(a), a = sqrt(2 nu) r, nu = 3/2 | 5/2, on a grid 0.1 <= r <= 10; dK/dlog l
    = -r dk/dr = sf2 2^(1 - nu) / Gamma(nu) a^(nu + 1) K_(nu - 1)(a)  (from d/da [a^nu K_nu] = -a^nu K_(nu - 1)).
    Tolerance: the AMOS routine behind scipy.special.kv states its relative error as P 10^S, P = the unit roundoff
    (2^-52), S = max(1, |log10 a|, |log10 nu|); Gamma, the two powers and the products add a few roundings: 8 eps."""
    from scipy.special import gamma, kv
    nu = {tm.MATERN32: 1.5, tm.MATERN52: 2.5}[kind]
    r = np.geomspace(0.1, 10.0, 200)
    a = np.sqrt(2 * nu) * r
    sf2 = 1.7
    kf, dk = truth.matern_kernel((r.astype(LD)) ** 2, LD(sf2), kind)
    c = sf2 * 2.0 ** (1 - nu) / gamma(nu)
    kb, db = c * a ** nu * kv(nu, a), c * a ** (nu + 1) * kv(nu - 1, a)
    tol = (10.0 ** np.maximum(1.0, np.abs(np.log10(a))) + 8) * EPS
    ek, ed = np.abs(kb - kf) / kf, np.abs(db - dk) / dk
    print("kind %d: k %.3e, dk %.3e of tolerance (largest ratio)" % (kind, float(np.max(ek / tol)), float(np.max(ed / tol))))
    assert np.all(ek <= tol) and np.all(ed <= tol)
    k0, d0 = truth.matern_kernel(np.zeros(1, dtype=LD), LD(sf2), kind)
    assert k0[0] == LD(sf2) and d0[0] == 0


@pytest.mark.parametrize("kind", tm.KINDS)
def test_gradient_is_the_derivative_of_ll(kind):
    """grad_k = d(-LL)/d theta_k by (LL(theta - h e_k) - LL(theta + h e_k)) / (theta+ - theta-), all in longdouble (the
    two fp64 arguments are exact; their difference is taken in longdouble).  Step: truncation h^2 |f'''| / 6 against
    rounding eps_LD |f| / h is least near h = (3 eps_LD)^(1/3) ~ 7e-7: h = 2^-20.  Tolerance, relative to max|g|:
    C (h^2 + eps_LD / h * |LL| / max|g|) with C = 100 for the size of the third derivative relative to the first on a
    log scale and for the ~n^2 roundings behind each LL (n = 40)."""
    n, d = 40, 3
    X, y = synth(n, d=d, seed=n, scale=4.0)
    hp = [0.9, 0.3, -1.0]
    h = 2.0 ** -20
    t = truth.Truth(X, y, truth.Matern(hp, kind))
    gs = np.max(np.abs(t.grad))
    tol = 100 * (h * h + truth.EPS_LD / h * float(abs(t.ll) / gs))
    for k in range(3):
        lo, hi = list(hp), list(hp)
        lo[k], hi[k] = hp[k] - h, hp[k] + h
        num = (truth.Truth(X, y, truth.Matern(lo, kind)).ll - truth.Truth(X, y, truth.Matern(hi, kind)).ll) / (LD(hi[k]) - LD(lo[k]))
        err = float(abs(num - t.grad[k]) / gs)
        print("kind %d g%d: formula %.15g, central difference %.15g, |diff| / max|g| %.3e (tolerance %.3e)"
              % (kind, k, float(t.grad[k]), float(num), err, tol))
        assert err <= tol, (kind, k, err, tol)


@pytest.fixture(scope="module")
def table(oracle):
    """Stand-in ratios and yardsticks of every case and kind, all eight orderings -- computed once."""
    out = {}
    for name in truth.MATERN_CASES:
        for kind in tm.KINDS:
            c = out[name, kind] = accuracy.live(oracle, tm.KIND_NAMES[kind], name)
            ratio, rs = accuracy.standin_ratios(c)
            print("STANDIN-MATERN %-13s %-8s " % (name, tm.KIND_NAMES[kind])
                  + "  ".join("%s %.2f" % kv for kv in list(ratio.items()) + list(rs.items()))
                  + "  | yardstick " + " ".join("%s %.1e" % kv for kv in c["noise"].items()))
    return out


def test_case_list_is_every_live_case():
    assert truth.MATERN_CASES == ("n1", "n2", "n63", "n64", "n65", "n257_d3", "n300_d17", "n515_d33", "n515_dense", "n384_cond1e6", "n1025_dense",
                                  "n1300_d6")
    assert all(truth.family_inputs(f, c)[0].shape[0] == truth.LIVE_CASES[c][0] for c in truth.MATERN_CASES
               for f in tm.KIND_NAMES.values())


def test_F_MATERN_is_what_the_rule_gives(table):
    """The project's rule (docs/ACCURACY.md, "The bound"): the next power of two at or above twice the largest stand-in /
    yardstick ratio over the case list, both kinds, all eight orderings -- measured here, on the CPU; F_SOLVE covers
    alpha and K^-1 likewise.  The ratios are those of the BLAS this runs on (docs/ACCURACY.md has the table of the build
    it was measured with)."""
    worst = max(max(accuracy.standin_ratios(c)[0].values()) for c in table.values())
    worst_solve = max(max(accuracy.standin_ratios(c)[1].values()) for c in table.values())
    rule = truth.factor_rule(worst)
    print("largest stand-in ratio %.2f -> F_MATERN by the rule %d (set: %d); alpha / K^-1 %.2f (F_SOLVE %d)"
          % (worst, rule, truth.F_MATERN, worst_solve, truth.F_SOLVE))
    assert truth.F_MATERN == rule, (worst, rule, truth.F_MATERN)
    assert 2 * worst_solve <= truth.F_SOLVE, (worst_solve, truth.F_SOLVE)


def test_yardsticks_under_the_cap(table):
    """No case has to be left out: every yardstick is far under truth.YARDSTICK_CAP, and the oracle on the data as given
    is no outlier among the permuted evaluations."""
    for (name, kind), c in table.items():
        accuracy.assert_yardstick_is_sane(c, (name, kind))


@pytest.mark.parametrize("kind", tm.KINDS)
def test_fp64_entry_formula_inside_the_bound(kind):
    """tests/truth_matern.py: entry_fp64 (the kernels' order of operations) against the longdouble kernel function on
    every case's K and k_test, entry by entry, inside k_entry_bound = (c0 + c1 (1 + a) (d + c2)) 2^-53, relative to the
    true entry.  The count, in u = 2^-53 (a correctly rounded operation 1 u; exp of libm / the device library 1 ulp = 2 u):
      d2  each term (x - y)^2: difference 1, square 2 + 1; the d-term sum of positive terms adds d - 1:         d + 2
      l2  exp(2 theta_0) on the host: 2;   s  one division: 1                                               => d + 5
      r   the square root halves the incoming error and adds its own rounding:                     (d + 5) / 2 + 1
      a   the constant RN(sqrt 3 | sqrt 5) and one multiply: 2                       => eps_a = (d + 11) / 2
      e   exp's argument error is amplified by a: a eps_a; its own error 2
      p   no cancellation (all terms positive): propagated eps_a dlog p / dlog a -- a / (1 + a) <= 1 for 3/2,
          (a + 2 a^2/3) / (1 + a + a^2/3) <= 2 for 5/2; own roundings: 3/2 one sum (1); 5/2 a a (1), RN(1/3) (1), its
          multiply (1), two sums of positive terms (the larger part's error + 1 each): 4
      kf  p e (1), sf2 (.) (1), sf2 = exp(2 theta_1) on the host (2): 4
    3/2: 2 + 1 + 4 + (a + 1) eps_a       = (7 + 1/2 (1 + a) (d + 11)) u
    5/2: 2 + 4 + 4 + (a + 2) eps_a      <= (10 + (1 + a) (d + 11)) u
    so (c0, c1, c2) = (7, 1/2, 11) and (10, 1, 11): truth_matern.K_BOUND.  (Entries below 1e-290, where fp64 has no full
    mantissa left, do not occur in the cases; asserted.)"""
    assert tm.K_BOUND == {tm.MATERN32: (7.0, 0.5, 11.0), tm.MATERN52: (10.0, 1.0, 11.0)}
    worst = 0.0
    for name in truth.MATERN_CASES:
        X, y, Xt, hp = truth.live_inputs(name)
        l2, sf2, _ = truth.hyper(hp)
        d = X.shape[1]
        for A in (X, Xt):
            true = truth.matern_kernel(truth.sqdist(A, X) / l2, sf2, kind)[0]
            got = tm.entry_fp64(tm.sqdist64(A, X), np.exp(2 * hp[0]), np.exp(2 * hp[1]), kind)[0]
            bound = tm.k_entry_bound(tm.a_of(A, X, hp, kind), d, kind)
            assert float(true.min()) > 1e-290
            rel = np.abs(got.astype(LD) - true) / true
            worst = max(worst, float(np.max(rel / bound)))
            assert np.all(rel <= bound), (name, kind, float(np.max(rel / bound)))
    print("kind %d: largest |fp64 entry - truth| / bound %.3f" % (kind, worst))


@pytest.mark.parametrize("kind", tm.KINDS)
def test_fp64_entry_extremes(kind):
    """s = 0 gives sf2 exactly and dk = 0; s = +inf and a finite a whose exp underflows give exactly 0 for both, no NaN
    (a > 1e154: a a overflows to inf while e = 0)."""
    sf2 = 1.37
    kf, dk = tm.entry_fp64(np.array([0.0, 1.0, 1e6, 1e300, np.inf]), 1.0, sf2, kind)
    assert kf[0] == sf2 and dk[0] == 0.0
    assert 0 < kf[1] < sf2 and dk[1] > 0
    assert np.all(kf[2:] == 0.0) and np.all(dk[2:] == 0.0)
    assert not np.any(np.isnan(kf)) and not np.any(np.isnan(dk))
