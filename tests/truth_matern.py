"""The Matern 3/2 and 5/2 kernels' per-entry fp64 arithmetic and its rounding bound -- TEST INFRASTRUCTURE, CPU, numpy
only.  The Matern truth, yardstick, stand-in and F_MATERN are those of tests/truth.py (the descriptor truth.Matern).

`entry_fp64` restates the kernels' per-entry arithmetic (kernels.hip: matern_entry) operation by operation in fp64
numpy; `k_entry_bound` is the rounding count it and the GPU's K entries are held to.  `standin_objective` drives the
CPU optimiser the library's is compared with.
"""
import numpy as np

import truth
from truth import C2, KIND_NAMES, KINDS, MATERN32, MATERN52, U  # noqa: F401  (the kinds are used through this module)


def sqdist64(A, B):
    """|a_i - b_j|^2 in fp64, one feature at a time in index order, no FMA: sqdist_4x4's sequence."""
    S = np.zeros((A.shape[0], B.shape[0]))
    for k in range(A.shape[1]):
        D = A[:, k][:, None] - B[:, k][None, :]
        S = S + D * D
    return S


SQRT3, SQRT5, THIRD = 1.7320508075688772, 2.23606797749979, 0.3333333333333333     # the kernels' fp64 constants


def entry_fp64(d2, l2, sf2, kind):
    """matern_entry of kernels.hip in fp64 numpy, one rounding per line as there: -> (kf, dk).  div_by is a correctly
    rounded quotient, numpy's sqrt is correctly rounded, every product and sum is its own ufunc call (no FMA)."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        s = d2 / l2
        a = (SQRT3 if kind == MATERN32 else SQRT5) * np.sqrt(s)
        e = np.exp(-a)
        p1 = 1.0 + a
        if kind == MATERN32:
            p, q = p1, a * a
        else:
            t = (a * a) * THIRD
            p, q = p1 + t, t * p1
        dead = e == 0.0
        return np.where(dead, 0.0, sf2 * (p * e)), np.where(dead, 0.0, sf2 * (q * e))


# The K-entry bound, relative to the true Kf entry, in units of u = 2^-53 (a correctly rounded operation: 1 u; exp of
# libm / the device library: 1 ulp = 2 u), counted along matern_entry:
#   d2   each term (x - y)^2: difference 1 u, square 2 u + 1 u; the d-term sum of positive terms adds d - 1       d + 2
#   l2   exp(2 theta_0) on the host                                                                                    2
#   s    one (correctly rounded) division                                                                              1
#   r    the square root halves the incoming (d + 5) u and adds its own rounding                         (d + 5) / 2 + 1
#   a    the constant RN(sqrt 3 | sqrt 5) and one multiply                                                             2
#        => eps_a = (d + 11) / 2 u
#   e    exp's argument error is amplified by a: a eps_a; its own error                                                2
#   p    no cancellation (all terms positive): propagated eps_a dlog p / dlog a, which is a / (1 + a) <= 1 for 3/2 and
#        (a + 2 a^2/3) / (1 + a + a^2/3) <= 2 for 5/2; own roundings: 3/2 one sum (1); 5/2 a a (1), the constant RN(1/3)
#        (1), its multiply (1), then two sums of positive terms (max of the parts' + 1 each: 3 + 1 = 4)            1 | 4
#   kf   p e (1), sf2 (...) (1), sf2 = exp(2 theta_1) on the host (2)                                                  4
# Sum: 3/2: (7 + (a + 1) (d + 11) / 2) u;  5/2: (10 + (a + 2) (d + 11) / 2) u <= (10 + (1 + a) (d + 11)) u.
# Form (c0 + c1 (1 + a) (d + c2)) u:
K_BOUND = {MATERN32: (7.0, 0.5, 11.0), MATERN52: (10.0, 1.0, 11.0)}


def k_entry_bound(a, d, kind):
    """Relative bound on an fp64 Kf entry at a = sqrt(3 | 5) r (array or scalar) with d features."""
    c0, c1, c2 = K_BOUND[kind]
    return (c0 + c1 * (1.0 + np.asarray(a, dtype=np.float64)) * (d + c2)) * U


def a_of(A, B, hp, kind):
    """a = sqrt(3 | 5) |x - x'| / l in fp64, for k_entry_bound."""
    return np.sqrt(C2[kind] * sqdist64(np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64))
                   / np.exp(2 * hp[0]))


def standin_objective(X, y, kind):
    """theta -> (-LL, gradient) of the fp64 stand-in: the objective cugp_cg_minimize is driven by in the optimiser test."""
    def fn(th):
        try:
            ll, g, _, _ = truth.standin(truth.Matern(th, kind), X, y, X[:1])
        except np.linalg.LinAlgError:
            return float("nan"), np.full(3, np.nan)
        return -ll, g
    return fn
