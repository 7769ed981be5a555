"""CPU check of the ARD product-of-experts yardstick (tests/truth_ard_bcm.py): the stand-in table over its case list, and
that the project's factor rule asks for no more than the existing F_ARD -- what tests/test_gpu_ard_bcm.py leans on.
The ratios are those of the BLAS this runs on (docs/ACCURACY.md has the table of the build it was measured with)."""
import pytest

import truth
import truth_ard_bcm as tab

pytestmark = pytest.mark.skipif(not truth.EXTENDED, reason="numpy.longdouble is not an extended-precision type here")


def test_F_ARD_covers_the_bcm_standin(oracle):
    worst = 0.0
    for name in tab.CASES:
        c = tab.case(oracle, name)
        ratio = tab.standin_ratios(c)
        print("STANDIN-ARD-BCM %-12s " % name + "  ".join("%s %.2f" % kv for kv in ratio.items())
              + "  -> factor rule %d" % truth.factor_rule(max(ratio.values())))
        worst = max(worst, *ratio.values())
        for q in c["cov"].quantities:                 # the yardstick is sane (accuracy.assert_yardstick_is_sane's two rules)
            assert c["first"][q] <= c["cov"].F * max(c["rest"][q], c["floor"][q]), (name, q, c["first"][q], c["rest"][q])
            assert c["noise"][q] <= truth.YARDSTICK_CAP * c["floor"][q] / truth.U4, (name, q, c["noise"][q])
    print("largest stand-in ratio %.2f: factor rule %d, F_ARD %d" % (worst, truth.factor_rule(worst), truth.F_ARD))
    assert truth.factor_rule(worst) <= truth.F_ARD, (worst, truth.F_ARD)
