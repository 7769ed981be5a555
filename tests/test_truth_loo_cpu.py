"""CPU checks of everything tests/test_gpu_loo.py leans on (tests/truth_loo.py):

  1. the truth is itself tested: at n = 24 (d = 2; SE and ARD) mu_i and var_i against actually deleting point i and
     predicting it from the other 23 in longdouble (1e-15 relative), and the gradient against central differences of that
     brute-force objective -- the step rule of tests/test_truth_predict_grad_cpu.py: at h = 1e-5 the error relative to the
     largest component is at most 1e-8 and falls by 100 +- 10 % from h = 1e-4;
  2. the stand-in (the fused formulation in fp64, LAPACK / BLAS order) against the yardstick (the textbook route through the
     CPU oracle's potri / potrs): truth.factor_rule of the largest ratio is at most F_LOO[family], on every case of the GPU
     list; F_LOO is at least the family's existing factor;
  3. every yardstick is sane (no outlier on the data as given, under the existing 1e-9 cap);
  4. teeth: c_i without its alpha_i^2 / kappa_i term, and W_loo with one of its two outer products, each exceed the bound
     on at least one case.
The ratios are those of the BLAS this runs on."""
import numpy as np
import pytest

import truth
import truth_loo as tl
from conftest import HP_DEFAULT, synth

pytestmark = pytest.mark.skipif(not truth.EXTENDED, reason="numpy.longdouble is not an extended-precision type here")

LD = truth.LD
H_COARSE, H_FINE = LD("1e-4"), LD("1e-5")
SMALL = {"se": lambda hp: truth.SE(hp), "ard": lambda hp: truth.ARD(hp)}
SMALL_HP = {"se": list(HP_DEFAULT), "ard": [0.5, 1.2, 0.5, 0.5]}


def small(family, hp=None):
    X, y = synth(24, d=2, seed=3 * 24 + 2, scale=4.0)
    return X, y, SMALL[family](SMALL_HP[family] if hp is None else hp)


@pytest.mark.parametrize("family", ["se", "ard"])
def test_truth_is_leaving_one_out(family):
    X, y, cov = small(family)
    tt = tl.truth_of(truth.Truth(X, y, cov), y)
    mu, var, logp, ll = tl.brute(X, y, cov)
    for q, ref in (("mu", mu), ("var", var), ("logp", logp)):
        err = float(np.max(np.abs(tt[q] - ref) / np.abs(ref)))
        print("BRUTE %-3s %-4s largest relative difference %.2e" % (family, q, err))
        assert err <= 1e-15, (q, err)
    assert float(abs(tt["ll"] - ll) / abs(ll)) <= 1e-15


def brute_objective(family, X, y, theta):
    """-L_LOO by leaving one out at the fp64 point theta (a descriptor takes fp64 log-hyper-parameters as exact inputs; the
    difference quotient below divides by the exact distance of the two shifted points)."""
    return -tl.brute(X, y, SMALL[family]([float(v) for v in theta]))[3]


@pytest.mark.parametrize("family", ["se", "ard"])
def test_truth_gradient_is_the_derivative_of_leaving_one_out(family):
    X, y, cov = small(family)
    exact = tl.truth_of(truth.Truth(X, y, cov), y)["grad"]
    th0 = np.array(SMALL_HP[family], dtype=np.float64)
    e = {}
    for h in (H_COARSE, H_FINE):
        fd = np.empty(len(th0), dtype=LD)
        for j in range(len(th0)):
            hi, lo = th0.copy(), th0.copy()
            hi[j] += float(h)
            lo[j] -= float(h)
            fd[j] = (brute_objective(family, X, y, hi) - brute_objective(family, X, y, lo)) / (LD(hi[j]) - LD(lo[j]))
        e[h] = float(np.max(np.abs(fd - exact)) / np.max(np.abs(exact)))
    print("FD %-3s err/scale h=1e-4 %.3e  h=1e-5 %.3e  ratio %.1f" % (family, e[H_COARSE], e[H_FINE], e[H_COARSE] / e[H_FINE]))
    assert e[H_FINE] <= 1e-8, e
    assert 90.0 <= e[H_COARSE] / e[H_FINE] <= 110.0, e


@pytest.fixture(scope="module")
def table(oracle):
    """Stand-in ratios of every case of the GPU list -- computed once."""
    out = {}
    for family, name in tl.CASES:
        c = tl.case(oracle, family, name)
        r = out[family, name] = tl.ratios(c, tl.standin(c["cov"], c["X"], c["y"]))
        Q = tl.quantities(c["cov"])
        print("STANDIN-LOO %-12s %-13s " % (family, name) + "  ".join("%s %.2f" % (q, r[q]) for q in Q)
              + "  | yardstick " + " ".join("%.1e" % max(c["noise"][q], c["floor"][q]) for q in Q))
    return out


def test_case_list():
    assert tl.CASES == (("se", "n65"), ("se", "n128"), ("se", "n257_d3"), ("se", "n384_cond1e6"), ("matern32", "n65"),
                        ("matern52", "n300_d17"), ("ard", "n257_d3"), ("ard", "n300_d17"), ("matern52_ard", "n257_d3"),
                        ("se", "n1300_d6"),
                        ("se", "n1"), ("se", "n2"), ("se", "n63"), ("se", "n64"), ("matern32", "n63"), ("ard", "n1_d2"),
                        ("ard", "n2_d2"), ("ard", "n63_d2"), ("matern52_ard", "n63_d2"))
    assert set(tl.F_LOO) == {f for f, _ in tl.CASES}


def test_factors_hold_the_standin(table):
    """F_LOO[family] is the larger of the family's existing factor and truth.factor_rule of the largest stand-in ratio."""
    for family in tl.F_LOO:
        worst = max(max(r.values()) for (f, _), r in table.items() if f == family)
        rule = truth.factor_rule(worst)
        print("F_LOO %-12s largest stand-in ratio %.2f  factor_rule %d  existing %d  F_LOO %d"
              % (family, worst, rule, tl.EXISTING[family], tl.F_LOO[family]))
        assert rule <= tl.F_LOO[family], (family, worst, rule)
        assert tl.F_LOO[family] >= tl.EXISTING[family], family


def test_yardsticks_are_sane(table, oracle):
    for family, name in table:
        tl.assert_yardstick_is_sane(tl.case(oracle, family, name), (family, name))


@pytest.mark.parametrize("mutate", ["c_without_alpha", "one_outer_product"])
def test_mutations_are_caught(table, oracle, mutate):
    caught = []
    for family, name in tl.CASES:
        c = tl.case(oracle, family, name)
        r = tl.ratios(c, tl.standin(c["cov"], c["X"], c["y"], mutate))
        if max(r.values()) > tl.F_LOO[family]:
            caught.append((family, name, round(max(r.values()), 1)))
    print("MUTATION %s beyond the bound on:" % mutate, caught)
    assert caught, mutate
