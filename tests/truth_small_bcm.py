"""Products of experts whose experts lie below, at and around one 64-row build tile -- TEST INFRASTRUCTURE, CPU, a plain
module beside tests/truth.py, tests/accuracy.py, tests/truth_poe_modes.py and tests/truth_predict_grad.py.

Every case is a list of EXPLICIT expert sizes over one data set of d = 2 (bcm_create pads all experts of a model to the
largest when their 128-tile counts differ by at most one, and runs them as one batched group):

    1+1+3            cugp_bcm_create_split's split of N = 5 into K = 3: every expert a handful of rows
    63+63+64         the split of N = 190: below and at the build tile
    1+2+63+64+65     one group padded to 65 rows: an expert's own n far from its neighbours', most of each matrix padding
    2+130            the small expert padded into a second 128-tile that holds nothing but padding
    2+300            tile counts that differ by two: no common padded size, experts of different padded sizes in one model

  truth      every expert's truth.Truth (longdouble), combined by truth.poe in expert order: truth.bcm_truth's procedure on
             explicit rows
  yardstick  truth.noise_level of the family's own fp64 evaluator (cov.evaluator: the CPU oracle; ARD on the scaled copy, as
             tests/truth_ard_bcm.py) per expert, combined by truth.poe, the rows permuted inside their own expert
  stand-in   truth.standin per expert through truth.poe (truth.standin_bcm on explicit rows); its ratios
             (tests/test_truth_small_bcm_cpu.py, docs/ACCURACY.md) ask for no factor beyond the families' existing ones
  bound      F_family max(yardstick, floor) with truth.F, F_MATERN, F_ARD as they stand
  modes      `modes_case`: the combination rules of tests/truth_poe_modes.py on the experts' latent predictions;
  gradients  `grad_case`: tests/truth_predict_grad.py's product of experts (bcm_case_at) on the same experts
"""
import numpy as np

import truth
import truth_ard_matern as tam  # noqa: F401  (adds "matern32_ard" to truth.FAMILIES)
import truth_poe_modes as tpm
import truth_predict_grad as tpg
from conftest import HP_DEFAULT, synth

D = 2
SCALE = 4.0
ROWS = {
    "1+1+3": (1, 1, 3),
    "63+63+64": (63, 63, 64),
    "1+2+63+64+65": (1, 2, 63, 64, 65),
    "2+130": (2, 130),
    "2+300": (2, 300),
}
SPLITS = {"1+1+3": (5, 3), "63+63+64": (190, 3)}        # the two that are cugp_bcm_create_split's own split of (N, K)
MIXED = "1+2+63+64+65"
HP_ARD = list(truth.ARD_CASES["n65_d2"][2]) + list(truth.ARD_CASES["n65_d2"][3:5])     # n65_d2's parameters
HP = {"se": list(HP_DEFAULT), "matern52": list(HP_DEFAULT), "ard": HP_ARD, "matern32_ard": HP_ARD}
# (family, rows): every table row for se, matern52 and ard; matern32_ard on the mixed group alone
CASES = tuple((f, r) for f in ("se", "matern52", "ard") for r in ROWS) + (("matern32_ard", MIXED),)
MODES_CASES = tuple((f, MIXED) for f in ("se", "matern52", "ard"))                    # the five combination rules
GRAD_CASES = tuple((f, r) for f in ("se", "matern52", "ard") for r in (MIXED, "2+300"))     # cugp_bcm_predict_grad
GROUPED_ROWS = (MIXED, "2+130")                          # one batched group each: held against the experts one by one


def parts_of(rows):
    """-> [(offset, rows)] of consecutive experts."""
    off = np.concatenate([[0], np.cumsum(rows)[:-1]])
    return [(int(o), int(r)) for o, r in zip(off, rows)]


def case_id(case):
    return "%s-%s" % case


def inputs(family, rname):
    """-> (X, y, Xt, cov, parts): synth(N, d = 2, seed = N + K, box 4.0), 64 test points in the same box, row 5 of them a
    training row (truth.points), the family's descriptor."""
    rows = ROWS[rname]
    N, K = sum(rows), len(rows)
    X, y = synth(N, d=D, seed=N + K, scale=SCALE)
    return X, y, np.ascontiguousarray(truth.points(X, D, SCALE)), truth.FAMILIES[family][1](HP[family]), parts_of(rows)


_CASES = {}


def expert_truths(family, rname):
    """The experts' truth.Truth, once per process (they do not depend on the test points)."""
    key = ("truths", family, rname)
    if key not in _CASES:
        X, y, _, cov, parts = inputs(family, rname)
        _CASES[key] = [truth.Truth(X[o: o + r], y[o: o + r], cov, keep=False) for o, r in parts]
    return _CASES[key]


def case(oracle, family, rname):
    """Truth, yardsticks (with the as-given and the permuted parts) and floors of LL, gradient, means and variances."""
    key = (family, rname)
    if key not in _CASES:
        X, y, Xt, cov, parts = inputs(family, rname)
        ts = iter(expert_truths(family, rname))

        def expert(Xk, yk):
            t = next(ts)
            return (t.ll, t.grad) + t.predict(Xt)
        tb = dict(zip(("ll", "grad", "mean", "var"), truth.poe(parts, expert)(X, y)))
        Xe, ev = cov.evaluator(oracle, X, Xt)
        noise, first, rest = truth.noise_level(cov, truth.poe(parts, ev), Xe, y, tb["ll"], tb["grad"], tb["mean"], tb["var"],
                                               parts=parts)
        _CASES[key] = dict(X=X, y=y, Xt=Xt, cov=cov, parts=parts, K=len(parts), tb=tb, noise=noise, first=first, rest=rest,
                           floor=truth.floors(cov, truth.scales(cov, tb["ll"], tb["grad"], tb["mean"])))
    return _CASES[key]


def errors(c, ll, grad, mean, var):
    tb = c["tb"]
    return truth.errors(c["cov"], ll, grad, mean, var, tb["ll"], tb["grad"], tb["mean"], tb["var"])


def errors_pred(c, mean, var):
    return truth.errors_pred(mean, var, c["tb"]["mean"], c["tb"]["var"])


def standin_ratios(c):
    """Stand-in error / max(noise, floor) per quantity of the family."""
    st = truth.poe(c["parts"], lambda Xk, yk: truth.standin(c["cov"], Xk, yk, c["Xt"]))(c["X"], c["y"])
    e = errors(c, *st)
    return {q: e[q] / max(c["noise"][q], c["floor"][q]) for q in c["cov"].quantities}


def modes_case(oracle, family, rname):
    """tests/truth_poe_modes.py's case (truth_case + yardsticks) on explicit rows."""
    key = ("modes", family, rname)
    if key not in _CASES:
        X, y, Xt, cov, parts = inputs(family, rname)
        ex = [tpm.latent(t, Xt) for t in expert_truths(family, rname)]
        m, v = np.array([e[0] for e in ex], dtype=truth.LD), np.array([e[1] for e in ex], dtype=truth.LD)
        c = dict(X=X, y=y, Xt=Xt, cov=cov, K=len(parts), parts=parts, experts=ex,
                 modes={mode: tpm.combine(m, v, mode, cov.sf2) for mode in tpm.MODES})
        c["yard"] = tpm.yardsticks(oracle, c)
        _CASES[key] = c
    return _CASES[key]


def grad_case(oracle, family, rname):
    """tests/truth_predict_grad.py's product-of-experts case on explicit rows."""
    key = ("grad", family, rname)
    if key not in _CASES:
        X, y, Xt, cov, parts = inputs(family, rname)
        _CASES[key] = tpg.bcm_case_at(oracle, X, y, Xt, cov, parts, expert_truths(family, rname))
    return _CASES[key]
