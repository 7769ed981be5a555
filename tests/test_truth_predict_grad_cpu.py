"""CPU checks of everything tests/test_gpu_predict_grad.py leans on (tests/truth_predict_grad.py):

  1. the truth's gradients against central differences of the truth's own longdouble prediction, the test inputs
     perturbed in longdouble: the only independent check of the derivative formulas;
  2. the stand-in (the library's formulation in fp64, LAPACK / BLAS order) stays at or below half the family's factor on
     every case of the GPU list, so truth.F, F_MATERN and F_ARD hold the gradients as they stand;
  3. every yardstick is sane (no outlier on the data as given, under the cap);
  4. the mutation "coordinate form" is caught on the shifted ARD case;
  5. the longdouble chain rule of the combination rules against central differences of truth_poe_modes.combine.
"""
import numpy as np
import pytest

import accuracy
import truth
import truth_poe_modes as tpm
import truth_predict_grad as tpg

pytestmark = pytest.mark.skipif(not truth.EXTENDED, reason="numpy.longdouble is not an extended-precision type here")

LD = truth.LD
H_COARSE, H_FINE = LD("1e-4"), LD("1e-5")


def central(f, x, h):
    """d f / d x[:, c] by central differences in longdouble; f maps [nt, d] -> a tuple of [nt] arrays -> a tuple of
    [nt, d]."""
    outs = None
    for c in range(x.shape[1]):
        hi, lo = x.copy(), x.copy()
        hi[:, c] += h
        lo[:, c] -= h
        fd = [(a - b) / (hi[:, c] - lo[:, c]) for a, b in zip(f(hi), f(lo))]
        if outs is None:
            outs = [np.empty(x.shape, dtype=LD) for _ in fd]
        for o, v in zip(outs, fd):
            o[:, c] = v
    return outs


def hold_h_rule(tag, exact, f, x):
    """At h = 1e-5 the error relative to the largest true entry is at most 1e-8, and it falls by 100 +- 10 % from h = 1e-4:
    pure O(h^2) truncation (a wrong formula leaves an error that does not move with h)."""
    e = {}
    for h in (H_COARSE, H_FINE):
        e[h] = [float(np.max(np.abs(n - t)) / np.max(np.abs(t))) for n, t in zip(central(f, x, h), exact)]
    for i, (coarse, fine) in enumerate(zip(e[H_COARSE], e[H_FINE])):
        print("FD %-26s quantity %d  err/scale h=1e-4 %.3e  h=1e-5 %.3e  ratio %.1f" % (tag, i, coarse, fine, coarse / fine))
        assert fine <= 1e-8, (tag, i, fine)
        assert 90.0 <= coarse / fine <= 110.0, (tag, i, coarse, fine)


@pytest.mark.parametrize("family,name", [("se", "n65"), ("matern32", "n65"), ("matern52", "n257_d3"), ("ard", "n257_d3")])
def test_truth_is_the_derivative_of_the_prediction(oracle, family, name):
    c = accuracy.live(oracle, family, name)
    t, Xt = c["t"], c["Xt"].astype(LD)
    exact = tpg.truth_gradients(t, c["Xt"])
    hold_h_rule(family + " " + name, exact, lambda x: tpg.truth_predict(t, x), Xt)
    # the latent variance has the same gradient: the noise term is a constant
    lat = central(lambda x: tpg.truth_predict(t, x, latent=True), Xt, H_FINE)[1]
    assert float(np.max(np.abs(lat - exact[1])) / np.max(np.abs(exact[1]))) <= 1e-8


@pytest.fixture(scope="module")
def table(oracle):
    """Stand-in ratios and yardsticks of every case of the GPU list -- computed once."""
    out = {}
    for family, name in tpg.CASE_LIST:
        c = tpg.case(oracle, family, name)
        r = out[family, name] = tpg.ratios(c, *tpg.standin(c["cov"], c["X"], c["y"], c["Xt"]))
        print("STANDIN-GRAD %-9s %-14s " % (family, name) + "  ".join("%s %.2f" % kv for kv in r.items())
              + "  | yardstick " + " ".join("%s %.1e" % (q, max(c["noise"][q], c["floor"][q])) for q in tpg.QUANTITIES)
              + "  scale " + " ".join("%.1e" % (c["floor"][q] / truth.U4) for q in tpg.QUANTITIES))
    return out


def test_case_list():
    assert tpg.CASES == {"se": ("n1", "n2", "n63", "n64", "n65", "n257_d3", "n300_d17", "n515_d33", "n384_cond1e6"),
                         "matern32": ("n1", "n2", "n63", "n64", "n65", "n257_d3"),
                         "matern52": ("n1", "n63", "n300_d17", "n384_cond1e6"),
                         "ard": ("n1_d2", "n2_d2", "n63_d2", "n64_d2", "n65_d2", "n257_d3", "n300_d17", "n257_d3_shift",
                                 "n384_cond1e6")}
    assert tpg.F_GRAD is None


def test_standin_stays_below_half_the_factors(table, oracle):
    """The existing factors hold the gradients: the stand-in, measured here on the CPU, is at or below F / 2 on every case
    (docs/ACCURACY.md has the table of the BLAS it was measured with)."""
    for (family, name), r in table.items():
        F = tpg.case(oracle, family, name)["cov"].F
        assert max(r.values()) <= F / 2, (family, name, r, F)
    worst = {f: max(max(r.values()) for (g, _), r in table.items() if g == f) for f in tpg.CASES}
    print("largest stand-in ratios per family:", {f: round(w, 2) for f, w in worst.items()})


def test_yardsticks_are_sane(table, oracle):
    for family, name in table:
        tpg.assert_yardstick_is_sane(tpg.case(oracle, family, name), (family, name))


def test_coordinate_form_is_caught(table, oracle):
    """x*_c sum(G a) - sum(G a x_c) is algebraically the same and cancels where |x| >> |x - x'|: on the shifted case it lies
    beyond the bound the GPU is held to."""
    c = tpg.case(oracle, "ard", "n257_d3_shift")
    r = tpg.ratios(c, *tpg.standin(c["cov"], c["X"], c["y"], c["Xt"], coordinate=True))
    print("MUTATION coordinate form on ard n257_d3_shift:", {q: round(v, 1) for q, v in r.items()},
          "against", table["ard", "n257_d3_shift"])
    assert max(r.values()) > truth.F_ARD, r


# ------------------------------------------------------------------ the chain rule of the combination rules
def synthetic_experts(K, nt, d, sf2, sn2, seed):
    """Smooth expert predictions of x in longdouble with their exact gradients: m_k = sin(a_k . x + b_k),
    var_f,k = sf2 (0.55 + 0.4 sin(c_k . x + e_k)) in (0, sf2).  -> f(x) -> (m [K][nt], v [K][nt]), g(x) -> (dm, dv)."""
    rng = np.random.default_rng(seed)
    a, cc = rng.uniform(-1, 1, (K, d)).astype(LD), rng.uniform(-1, 1, (K, d)).astype(LD)
    b, e = rng.uniform(-3, 3, K).astype(LD), rng.uniform(-3, 3, K).astype(LD)

    def f(x):
        return np.sin(x @ a.T + b).T, (sf2 * (LD("0.55") + LD("0.4") * np.sin(x @ cc.T + e))).T

    def g(x):
        dm = np.cos(x @ a.T + b).T[..., None] * a[:, None, :]
        dv = (sf2 * LD("0.4") * np.cos(x @ cc.T + e)).T[..., None] * cc[:, None, :]
        return dm, dv
    return f, g


@pytest.mark.parametrize("mode", tpg.BCM_MODES)
@pytest.mark.parametrize("K", (1, 3, 5))
def test_chain_rule_is_the_derivative_of_combine(K, mode):
    nt, d = 7, 3
    sf2, sn2 = LD("1.4918246976412703"), LD("0.1353352832366127")
    f, g = synthetic_experts(K, nt, d, sf2, sn2, 10 * K + len(mode))
    x = np.random.default_rng(4).uniform(-2, 2, (nt, d)).astype(LD)
    noise = sn2 if mode == "reference" else LD(0)
    rule = "poe" if mode == "reference" else mode

    def combined(xx):
        m, v = f(xx)
        return tpm.combine(m, v + noise, rule, sf2)
    m, v = f(x)
    exact = tpg.combine_grad(m, v + noise, *g(x), mode, sf2)
    hold_h_rule("combine %s K%d" % (mode, K), exact, combined, x)


@pytest.mark.parametrize("name", tpg.BCM_CASES)
def test_bcm_standin_stays_below_half_the_factors(oracle, name):
    """The product of experts at 200 points: the stand-in per expert through the fp64 chain rule against the experts'
    truths through the longdouble one, every mode and the reference product, at or below F / 2."""
    c = tpg.bcm_case(oracle, name)
    for mode in tpg.BCM_MODES:
        r = tpg.bcm_ratios(c, mode, *tpg.bcm_standin(c, mode))
        m = c["modes"][mode]
        print("STANDIN-GRAD-BCM %-15s %-9s " % (name, mode) + "  ".join("%s %.2f" % kv for kv in r.items())
              + "  | yardstick " + " ".join("%s %.1e" % (q, max(m["noise"][q], m["floor"][q])) for q in tpg.QUANTITIES))
        assert max(r.values()) <= c["cov"].F / 2, (name, mode, r)
        for q in tpg.QUANTITIES:
            assert m["noise"][q] <= truth.YARDSTICK_CAP * m["floor"][q] / truth.U4, (name, mode, q)
