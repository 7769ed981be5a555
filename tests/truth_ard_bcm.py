"""The cases and the yardstick of the ARD product-of-experts tests -- TEST INFRASTRUCTURE, CPU, a plain module beside
tests/truth.py and tests/accuracy.py.

An ARD BCM is K ARD experts over the reference's row split with ONE shared theta = [log l_1 .. log l_d, log sf, log sn].
  truth      truth.bcm_truth with the truth.ARD descriptor (longdouble, expert by expert)
  yardstick  truth.noise_level of the CPU oracle's isotropic evaluation of every expert on the scaled copy X / l at
             [0, theta_d, theta_{d+1}] (truth.ARD.evaluator's trick), combined by truth.poe in expert order, the rows
             permuted inside their own expert.  The oracle's g0 there is the sum of the g_c (truth.errors_ll_grad
             compares it with the sum of the true ones), and every g_c is held to that yardstick.
  stand-in   truth.standin_bcm; its ratios (tests/test_truth_ard_bcm_cpu.py, docs/ACCURACY.md) ask for no factor beyond
             the existing truth.F_ARD.
"""
import numpy as np

import truth
from conftest import synth

# name -> (N, K, d, theta_l, theta_f, theta_n, box half-width of synth)
CASES = {
    "3x65_d2": (195, 3, 2, [0.5, 1.2], 0.5, 0.5, 4.0),                                  # one row over a 64 build tile
    "3x300_d17": (900, 3, 17, np.linspace(0.7, 1.9, 17).tolist(), 0.3, -0.8, 1.8),      # two feature chunks
    "5x261p2_d3": (1307, 5, 3, [0.9, 0.3, 1.6], 0.2, -1.0, 4.0),                        # uneven split, last expert 263 rows
}


def inputs(name):
    """-> (X, y, Xt, cov, K): synth(N, d, seed=N + K, scale), truth.points in the same box, the ARD descriptor."""
    N, K, d, th, tf, tn, scale = CASES[name]
    X, y = synth(N, d=d, seed=N + K, scale=scale)
    return X, y, np.ascontiguousarray(truth.points(X, d, scale)), truth.ARD(list(th) + [tf, tn]), K


def case_at(oracle, cov, X, y, parts, Xt):
    """Truth, yardsticks and floors of an ARD BCM whose experts hold the rows `parts` [(offset, rows)] of (X, y), at the
    test points Xt.  The yardstick: truth.noise_level of the oracle's product of experts on the scaled data."""
    def expert(Xk, yk):
        t = truth.Truth(Xk, yk, cov, keep=False)
        return (t.ll, t.grad) + t.predict(Xt)
    tb = dict(zip(("ll", "grad", "mean", "var"), truth.poe(parts, expert)(X, y)))
    evaluate = truth.poe(parts, truth.oracle_evaluator(oracle, [0.0] + cov.hp[-2:], cov.scaled(Xt)))
    noise, first, rest = truth.noise_level(cov, evaluate, cov.scaled(X), y, tb["ll"], tb["grad"], tb["mean"], tb["var"],
                                           parts=parts)
    return dict(X=X, y=y, Xt=Xt, cov=cov, parts=parts, tb=tb, noise=noise, first=first, rest=rest,
                floor=truth.floors(cov, truth.scales(cov, tb["ll"], tb["grad"], tb["mean"])))


_CASES = {}


def case(oracle, name):
    """A case of CASES, computed once per process whichever test asks."""
    if name not in _CASES:
        X, y, Xt, cov, K = inputs(name)
        _CASES[name] = case_at(oracle, cov, X, y, truth.bcm_rows(len(y), K), Xt)    # (bcm_truth's split)
    return _CASES[name]


def bcm_errors(c, ll, grad, mean, var):
    """Errors of one fp64 evaluation of the case against its truth, per quantity of truth.QUANTITIES_ARD."""
    tb = c["tb"]
    return truth.errors(c["cov"], ll, grad, mean, var, tb["ll"], tb["grad"], tb["mean"], tb["var"])


def standin_ratios(c):
    """Stand-in (truth.standin, expert by expert as truth.standin_bcm) error / max(noise, floor) per quantity: the
    case's row in docs/ACCURACY.md."""
    st = truth.poe(c["parts"], lambda Xk, yk: truth.standin(c["cov"], Xk, yk, c["Xt"]))(c["X"], c["y"])
    e = bcm_errors(c, *st)
    return {q: e[q] / max(c["noise"][q], c["floor"][q]) for q in c["cov"].quantities}
