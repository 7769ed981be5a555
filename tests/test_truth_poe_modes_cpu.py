"""CPU counterpart of tests/test_gpu_poe_modes.py: the stand-in of tests/truth_poe_modes.py (a CPU fp64 restatement of
exactly the library's formulation of the four combination rules) against the longdouble truth and the yardstick, on every
case of the GPU list.  It measures what sets the factor of the GPU bound -- the stand-in must stay at or below half of the
family's factor (the project's rule, truth.factor_rule) -- and shows that the bound has teeth: three mutated stand-ins
must each exceed it on at least one case.  Every figure is printed before it is asserted (run with -s); docs/ACCURACY.md
records them.  No GPU, no library call.
"""
import numpy as np
import pytest

import truth
import truth_poe_modes as tp

pytestmark = pytest.mark.skipif(not truth.EXTENDED, reason="numpy.longdouble is not an extended-precision type here")

case = tp.case


@pytest.mark.parametrize("name,nt", tp.CASE_LIST)
def test_standin_within_half_the_factor(oracle, name, nt):
    """The stand-in's error / max(yardstick, floor) per mode and quantity; twice the largest must not exceed the factor
    the GPU test uses for the family (the next power of two at or above it is what a factor of its own would be)."""
    c = case(oracle, name, nt)
    worst = 0.0
    for mode in tp.MODES:
        r = tp.ratios(c, c["yard"], mode, *tp.standin(c, mode))
        fl = tp.floors(c, mode)
        print("STANDIN-COMBINE %-16s nt%-3d %-4s mean %.2f var %.2f | yardstick mean %.1e var %.1e" % (
            name, nt, mode, r["mean"], r["var"], max(c["yard"][mode]["mean"], fl["mean"]),
            max(c["yard"][mode]["var"], fl["var"])))
        worst = max(worst, r["mean"], r["var"])
        # the truth is a latent distribution that respects the formulas' properties
        tm, tv = c["modes"][mode]
        assert np.all(tv > 0)
        if mode in ("bcm", "rbcm"):
            assert np.all(tv <= c["cov"].sf2 * (1 + 1e-15))
    F = tp.factor(c["cov"])
    print("STANDIN-COMBINE %-16s nt%-3d worst %.2f -> rule %d, factor in use %d" % (name, nt, worst,
                                                                                  truth.factor_rule(worst), F))
    assert truth.factor_rule(worst) <= F, (name, nt, worst, F)


def test_k1_truth_is_the_expert():
    """K = 1: poe, gpoe and bcm are the expert's own latent distribution in the truth too (longdouble rounding)."""
    c = tp.truth_case("se_1x257", 257)
    m, v = c["experts"][0]
    for mode in ("poe", "gpoe", "bcm"):
        tm, tv = c["modes"][mode]
        assert float(np.max(np.abs(tm - m))) <= 8 * truth.EPS_LD * float(np.max(np.abs(m)))
        assert float(np.max(np.abs(tv - v) / v)) <= 8 * truth.EPS_LD


@pytest.mark.parametrize("mutation", list(tp.MUTATIONS))
def test_mutations_exceed_the_bound(oracle, mutation):
    """beta without the 1/2 (rbcm), the prior term dropped (bcm, rbcm), sn2 left in the experts' rows (every mode): each
    must exceed F max(yardstick, floor) on at least one case of the list -- else the bound or the list is too loose."""
    caught, largest = [], 0.0
    for name, nt in tp.CASE_LIST:
        c = case(oracle, name, nt)
        F = tp.factor(c["cov"])
        for mode in tp.MODES:
            r = tp.ratios(c, c["yard"], mode, *tp.standin(c, mode, **tp.MUTATIONS[mutation]))
            big = max(r["mean"], r["var"])
            largest = max(largest, big)
            if not big <= F:
                caught.append((name, nt, mode))
    print("MUTATION %-20s exceeds the bound on %d of %d (case, mode) pairs; largest ratio %.3g" % (
        mutation, len(caught), 4 * len(tp.CASE_LIST), largest))
    assert caught, mutation
