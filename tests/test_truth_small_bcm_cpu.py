"""CPU checks of everything tests/test_gpu_small.py leans on (tests/truth_small_bcm.py; tests/truth_loo.py on a grown handle):

  1. the table is the one the GPU tests run, and its two split rows are cugp_bcm_create_split's own split;
  2. per case the stand-in (truth.standin per expert through truth.poe, LAPACK / BLAS order) stays within the family's
     existing factor, and the yardstick is sane (accuracy.assert_yardstick_is_sane's two conditions);
  3. the combination rules and the input gradients of the product of experts on the mixed group (and 2+300): the
     stand-ins of tests/truth_poe_modes.py and tests/truth_predict_grad.py within the family's factor, yardsticks capped;
  4. a leave-one-out evaluation behind cugp_append: tests/truth_loo.py's fused formulation on the K^-1 and alpha that
     truth_append.standin_append's bordering leaves, within F_LOO of the family, on the small append cases;
  5. teeth: an expert that takes its row count from the lead expert (the first n_0 rows of its own data) leaves the bound on
     the mixed group.
The ratios are those of the BLAS this runs on."""
import numpy as np
import pytest

import accuracy
import truth
import truth_append as ta
import truth_loo as tl
import truth_poe_modes as tpm
import truth_predict_grad as tpg
import truth_small_bcm as tsb

pytestmark = pytest.mark.skipif(not truth.EXTENDED, reason="numpy.longdouble is not an extended-precision type here")

IDS = [tsb.case_id(c) for c in tsb.CASES]


def test_case_list():
    assert tsb.ROWS == {"1+1+3": (1, 1, 3), "63+63+64": (63, 63, 64), "1+2+63+64+65": (1, 2, 63, 64, 65), "2+130": (2, 130),
                        "2+300": (2, 300)}
    assert set(tsb.CASES) == {(f, r) for f in ("se", "matern52", "ard") for r in tsb.ROWS} | {("matern32_ard", tsb.MIXED)}
    assert set(tsb.MODES_CASES) == {(f, tsb.MIXED) for f in ("se", "matern52", "ard")}
    assert set(tsb.GRAD_CASES) == {(f, r) for f in ("se", "matern52", "ard") for r in (tsb.MIXED, "2+300")}
    assert tsb.HP_ARD == [0.5, 1.2, 0.5, 0.5] and tsb.HP["se"] == list(truth.HP_DEFAULT)
    for rname, (N, K) in tsb.SPLITS.items():
        assert tsb.parts_of(tsb.ROWS[rname]) == truth.bcm_rows(N, K)
    assert tsb.parts_of((1, 2, 63)) == [(0, 1), (1, 2), (3, 63)]


@pytest.mark.parametrize("family, rname", tsb.CASES, ids=IDS)
def test_standin_within_the_family_factor(oracle, family, rname):
    c = tsb.case(oracle, family, rname)
    r = tsb.standin_ratios(c)
    print("STANDIN-SMALL-BCM %-12s %-13s " % (family, rname) + "  ".join("%s %.2f" % kv for kv in r.items())
          + "  | yardstick " + " ".join("%s %.1e" % kv for kv in c["noise"].items()))
    accuracy.assert_yardstick_is_sane(c, (family, rname))
    assert max(r.values()) <= c["cov"].F, (r, c["cov"].F)


@pytest.mark.parametrize("family, rname", tsb.MODES_CASES, ids=[tsb.case_id(c) for c in tsb.MODES_CASES])
def test_modes_standin_within_the_family_factor(oracle, family, rname):
    c = tsb.modes_case(oracle, family, rname)
    for mode in tpm.MODES:
        r = tpm.ratios(c, c["yard"], mode, *tpm.standin(c, mode))
        fl = tpm.floors(c, mode)
        print("STANDIN-SMALL-MODES %-9s %-13s %-5s " % (family, rname, mode) + "  ".join("%s %.2f" % kv for kv in r.items()))
        assert max(r.values()) <= tpm.factor(c["cov"]), (mode, r)
        for q in ("mean", "var"):
            assert c["yard"][mode][q] <= truth.YARDSTICK_CAP * fl[q] / truth.U4, (mode, q)


@pytest.mark.parametrize("family, rname", tsb.GRAD_CASES, ids=[tsb.case_id(c) for c in tsb.GRAD_CASES])
def test_gradient_standin_within_the_family_factor(oracle, family, rname):
    c = tsb.grad_case(oracle, family, rname)
    for mode in tpg.BCM_MODES:
        r = tpg.bcm_ratios(c, mode, *tpg.bcm_standin(c, mode))
        m = c["modes"][mode]
        print("STANDIN-SMALL-GRAD %-9s %-13s %-9s " % (family, rname, mode) + "  ".join("%s %.2f" % kv for kv in r.items()))
        assert max(r.values()) <= tpg.factor(c["cov"]), (mode, r)
        for q in tpg.QUANTITIES:
            assert m["noise"][q] <= truth.YARDSTICK_CAP * m["floor"][q] / truth.U4, (mode, q)


SMALL_APPEND = [c for c in ta.CASES if truth.family_inputs(c[0], c[1])[0].shape[0] <= 65 and c[0] in tl.F_LOO]


@pytest.mark.parametrize("case", SMALL_APPEND, ids=[ta.case_id(c) for c in SMALL_APPEND])
def test_loo_behind_an_append_within_F_LOO(oracle, case):
    """cugp_loo on a handle that cugp_append has grown works from the bordered K^-1 and alpha."""
    family, name, n0, chunks = case
    c = tl.case(oracle, family, name)
    out = ta.standin_append(c["cov"], c["X"], c["y"], accuracy.live(oracle, family, name)["Xt"], n0, chunks)
    a, Ki = out[4], out[5]
    c64 = c["cov"].fp64()
    mu, var, logp = tl.point_quantities(np.diag(Ki).copy(), a, c["y"], truth.LL_CONST)
    ll = 0.0
    for v in logp:
        ll = ll + v
    W = tl.fused(Ki, a)
    g = np.array(c64.train(c["X"])[1](W) + (c64.sn2 * np.trace(W),))
    r = tl.ratios(c, (ll, g, mu, var, logp))
    print("STANDIN-APPEND-LOO %-34s " % ta.case_id(case) + "  ".join("%s %.2f" % kv for kv in r.items()))
    tl.assert_yardstick_is_sane(c, case)
    assert max(r.values()) <= tl.F_LOO[family], r


def test_small_append_cases():
    assert set(SMALL_APPEND) == {("se", "n2", 1, (1,)), ("se", "n65", 63, (1, 1)), ("matern32", "n2", 1, (1,)),
                                 ("ard", "n2_d2", 1, (1,)), ("ard", "n65_d2", 63, (1, 1)), ("matern52", "n65", 63, (1, 1)),
                                 ("se", "n64", 1, (62, 1))}


@pytest.mark.parametrize("family", ["se", "ard"])
def test_lead_experts_row_count_is_caught(oracle, family):
    """The mixed group with every expert evaluated on its first n_0 = 1 rows (a batched pass that takes n from the lead
    expert and not from the expert's own entry): LL and the gradient leave the bound by orders of magnitude."""
    c = tsb.case(oracle, family, tsb.MIXED)
    n0 = c["parts"][0][1]
    st = truth.poe(c["parts"], lambda Xk, yk: truth.standin(c["cov"], Xk[:n0], yk[:n0], c["Xt"]))(c["X"], c["y"])
    e = tsb.errors(c, *st)
    r = {q: e[q] / max(c["noise"][q], c["floor"][q]) for q in c["cov"].quantities}
    print("MUTATION-SMALL-BCM lead n %s: " % family + "  ".join("%s %.3g" % kv for kv in r.items()))
    assert r[c["cov"].quantities[0]] > 1e6 * c["cov"].F, r
