"""Rational quadratic covariance, ARD and with one tied length scale (GPML covRQard / covRQiso; include/cugp.h:
cugp_create_rq) -- TEST INFRASTRUCTURE, CPU, numpy only; a plain module beside tests/truth.py, tests/accuracy.py and the
truth_* modules, which it imports and leaves as they are.

    ARD   theta = [log l_1 .. log l_d, log alpha, log sf, log sn]          (nh = d + 3)
    tied  theta = [log l, log alpha, log sf, log sn], every w_c = exp(-theta_0)   (nh = 4)
    w_c = exp(-theta_c),  u_c = (x_c - x'_c) w_c,  s = sum_c u_c^2,  alpha = exp(theta_alpha),  u = s / (2 alpha),  L = log1p(u)
    Kf = sf2 exp(-alpha L)      H = Kf / (1 + u)      A = Kf alpha (u / (1 + u) - L)
    dK/dtheta_c = H u_c^2,   dK/dtheta_alpha = A,   dk/dx*_c = -H (x*_c - x_c) w_c^2
    g_c = 1/2 sum W o H o u_c^2,   g_alpha = 1/2 sum W o A,   tied: g_0 = g_l1 + .. + g_ld in index order

  descriptor  RQ(hp, tied=False): the interface of truth_ard_matern.ARDMatern (train, k, grad_factors, evaluator, fp64), the
              formulas in textbook form in the descriptor's dtype; `train` returns terms(W) = (g_l.., g_alpha, sum W o Kf).
              truth.errors_ll_grad takes the extra term as it stands: "gc" is the worst of the length AND the alpha components.
  yardstick   K formed in fp64 numpy, handed to the oracle's chol_and_det / K_inverse / Kinvy.
  per entry   `entry_fp64` restates cov_device.h's rq_entry rounding by rounding; `k_entry_bound` is the derived count that
              it and the GPU's K entries are held to.
  families    "rq_ard" and "rq" are added to truth.FAMILIES when this module is imported.
  factor      F_RQ by the project's rule from the stand-in on the CPU (tests/test_truth_rq_cpu.py; docs/ACCURACY.md).
"""
import math

import numpy as np

import accuracy
import truth
import truth_ard_matern as tam
from truth import LD, U

# The project's rule: the next power of two at or above twice the largest stand-in / yardstick ratio over RQ_CASES,
# TIED_CASES and the eight orderings.  STANDIN_WORST is that ratio as measured on the CPU before the first GPU run (the
# predictive mean of rq_ard n257_d3; the table is in docs/ACCURACY.md); test_truth_rq_cpu.py holds F_RQ to the rule at
# that figure and the live stand-in to F_RQ.
STANDIN_WORST = 16.15
F_RQ = 64


def shape_f(u):
    """u / (1 + u) - log1p(u) in u's dtype without the cancellation for small u: the series sum_{k >= 2} (-1)^(k+1)
    (1 - 1/k) u^k below 2^-7 (14 terms: the remainder is under 2^-105 of the leading term), the plain difference above."""
    u = np.asarray(u)
    T = u.dtype.type
    small = u < T(2.0 ** -7)
    us = np.where(small, u, T(0))
    ser = np.zeros_like(u)
    for k in range(15, 1, -1):                                  # Horner from the highest term down
        ser = ser * us + T((-1) ** (k + 1)) * (T(1) - T(1) / T(k))
    ser = ser * us * us
    ub = np.where(small, T(1), u)
    return np.where(small, ser, ub / (T(1) + ub) - np.log1p(ub))


def parts(S, sf2, alpha):
    """(Kf, H, A) from the weighted squared distance S, in its dtype: the textbook form."""
    T = S.dtype.type
    u = S / (T(2) * alpha)
    Kf = sf2 * np.exp(-alpha * np.log1p(u))
    return Kf, Kf / (T(1) + u), Kf * alpha * shape_f(u)


class RQ:
    """Rational quadratic at theta = [log l_1 .. log l_d, log alpha, log sf, log sn], or with tied=True at [log l, log
    alpha, log sf, log sn] (all d weights equal; d is the data's); differences are weighted before they are squared."""
    quantities = truth.QUANTITIES_ARD

    @property
    def F(self):
        return F_RQ

    def __init__(self, hp, tied=False, dtype=LD, mutate=None):
        self.hp, self.tied, self.dtype, self.mutate = [float(h) for h in hp], bool(tied), dtype, mutate
        assert not tied or len(self.hp) == 4
        th = np.asarray(self.hp[:-3], dtype=np.float64)
        self.wl = np.exp(-th.astype(dtype))
        self.alpha = np.exp(dtype(self.hp[-3]))
        self.sf2, self.sn2 = np.exp(2 * dtype(self.hp[-2])), np.exp(2 * dtype(self.hp[-1]))

    def weights(self, d):
        if self.tied:
            return np.full(d, self.wl[0], dtype=self.dtype)
        assert d == len(self.wl)
        return self.wl

    @property
    def w(self):
        """the weights of an ARD descriptor (a tied one needs the data's d: weights(d))"""
        assert not self.tied
        return self.wl

    def fp64(self):
        return RQ(self.hp, self.tied, np.float64, self.mutate)

    def _parts(self, S):
        T = self.dtype
        if self.mutate == "u_s_over_alpha":
            S = S * T(2)                                   # u := s / alpha
        Kf, H, A = parts(S, self.sf2, self.alpha)
        if self.mutate == "kf_for_h":
            H = Kf
        if self.mutate == "a_without_ratio":
            A = -Kf * self.alpha * np.log1p(S / (T(2) * self.alpha))
        return Kf, H, A

    def train(self, X):
        """-> (Kf, terms); terms(W) = (g_l .., g_alpha, sum W o Kf)."""
        w = self.weights(X.shape[1])
        Kf, H, A = self._parts(truth.wsqdist(X, X, w))

        def terms(W):
            WH = W * H
            g = [None] * len(w)

            def per_dim(c, D2):
                g[c] = (WH * D2).sum() / 2
            truth.wsqdist(X, X, w, per_dim)               # the dimensions a second time, W o H fixed
            if self.tied:
                g0 = g[0]
                for c in range(1, len(w)):
                    g0 = g0 + g[c]
                g = [g0]
            return tuple(g) + ((W * A).sum() / 2, (W * Kf).sum())
        return Kf, terms

    def k(self, A, B):
        return self._parts(truth.wsqdist(A, B, self.weights(np.asarray(A).shape[1])))[0]

    def grad_factors(self, Xt, X):
        """-> (G [nt, n], s [d]) of dk/dx*_c = -G (x*_c - x_c) s_c."""
        T = self.dtype
        w = self.weights(np.asarray(X).shape[1])
        return self._parts(truth.wsqdist(np.asarray(Xt, dtype=T), np.asarray(X, dtype=T), w))[1], w * w

    def evaluator(self, oracle, X, Xt, solve=False):
        """truth_ard_matern.ARDMatern.evaluator's construction: K in fp64 numpy through the oracle's factorisation, inverse
        and solve (the reference's order of operations)."""
        c = self.fp64()

        def evaluate(Xp, yp):
            n = len(yp)
            Kf, terms = c.train(Xp)
            K = Kf + c.sn2 * np.eye(n)
            quad, logdet = oracle.chol_and_det(K, yp)
            ll = -0.5 * (quad + logdet + n * truth.LL_CONST)
            Ki = oracle.K_inverse(K)
            a = oracle.Kinvy(K, yp)
            W = Ki - np.outer(a, a)
            g = np.array(terms(W) + (c.sn2 * np.trace(W),))
            Ks = c.k(Xt, Xp)
            out = (ll, g, Ks @ a, c.sf2 + c.sn2 - ((Ks @ Ki) * Ks).sum(1))
            return out + (a, Ki) if solve else out
        return X, evaluate


# ---------------------------------------------------------------------------------------- the cases
# truth.ARD_CASES' data and length scales with these theta_alpha; n257_d3_shift at 12 is the SE limit, the cancellation in
# A and |x| >> |x - x'| at once.  1300 rows is left out: the hand-over blocks are N^3 code the family does not touch.
THETA_ALPHA = {"n1_d2": 0.4, "n2_d2": 0.4, "n63_d2": 0.4, "n64_d2": 0.4, "n65_d2": 0.4, "n257_d3": -0.7,
               "n257_d3_shift": 12.0, "n300_d17": 2.0, "n515_d33": -0.7, "n515_dense": 0.4, "n384_cond1e6": 0.4,
               "n1025_dense": 2.0}
RQ_CASES = tuple(THETA_ALPHA)
TIED_CASES = ("n65", "n257_d3", "n300_d17", "n384_cond1e6")          # truth.LIVE_CASES' data, theta = [l, 0.4, f, n]
TIED_THETA_ALPHA = 0.4
JOINT_CASES_RQ = ("n65_d2", "n257_d3", "n1025_dense")


def rq_ard_inputs(name):
    X, y, Xt, hp = truth.ard_inputs(name)
    return X, y, Xt, hp[:-2] + [THETA_ALPHA[name]] + hp[-2:]


def rq_tied_inputs(name):
    X, y, Xt, hp = truth.live_inputs(name)
    return X, y, Xt, [hp[0], TIED_THETA_ALPHA, hp[1], hp[2]]


truth.FAMILIES.setdefault("rq_ard", (rq_ard_inputs, lambda hp: RQ(hp), lambda name: truth.ARD_CASES[name][5]))
truth.FAMILIES.setdefault("rq", (rq_tied_inputs, lambda hp: RQ(hp, tied=True), lambda name: truth.LIVE_CASES[name][3]))
ALL_CASES = tuple(("rq_ard", n) for n in RQ_CASES) + tuple(("rq", n) for n in TIED_CASES)


def inputs(family, name):
    return truth.family_inputs(family, name)


def live(oracle, family, name):
    """accuracy.live of the case: truth, predictions, yardsticks (alpha and K^-1 included) and floors, once per process."""
    return accuracy.live(oracle, family, name)


def standin_orderings(c):
    """Stand-in error / max(noise, floor) per quantity of the family: the largest over the data as given and the seven row
    permutations of truth.permutations (LL, gradient, means and variances do not depend on the order of the rows)."""
    cov, t = c["cov"], c["t"]
    worst = {q: 0.0 for q in cov.quantities}
    for idx in truth.permutations(len(c["y"])):
        st = truth.standin(cov, np.ascontiguousarray(c["X"][idx]), np.ascontiguousarray(c["y"][idx]), c["Xt"])
        e = truth.errors(cov, *st[:4], t.ll, t.grad, c["tm"], c["tv"])
        for q in cov.quantities:
            worst[q] = max(worst[q], e[q] / max(c["noise"][q], c["floor"][q]))
    return worst


# ---------------------------------------------------------------------------------------- per-entry arithmetic
def host_shape(theta_alpha):
    """(alpha, h2a) as the library's host code forms them: alpha = exp(theta_alpha) by the C library, h2a = RN(0.5 / alpha)."""
    try:
        alpha = math.exp(float(theta_alpha))
    except OverflowError:                                  # (C's exp returns +inf; Python raises)
        alpha = math.inf
    return alpha, 0.5 / alpha


def entry_fp64(s, sf2, alpha, h2a):
    """cov_device.h's rq_entry in fp64 numpy, one rounding per line as there: -> (kf, hh, da)."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        s = np.asarray(s, dtype=np.float64)
        u = s * h2a
        L = np.log1p(u)
        e = np.exp(-(alpha * L))
        kf = sf2 * e
        r = 1.0 / (1.0 + u)
        hh = kf * r
        da = kf * (alpha * (u * r - L))
        return kf, hh, da


def k_entry_bound(u, alpha, d):
    """Bounds on rq_entry's fp64 outputs at the true u = s / (2 alpha), in units of the true values:
    -> (|dKf| / Kf, |dH| / H, |dA| / (Kf alpha)).

    Counted in u_r = 2^-53 along rq_entry, every operation correctly rounded (1 u_r) except exp and log1p, for which the
    device library and the host's libm are ASSUMED to deliver 1 ulp = 2 u_r (the Matern bound's assumption, truth_matern.py):
      u_c   the difference 1, w_c = exp(-theta_c) on the host 2, their product 1                                     4
      s     each term u_c^2: 2 * 4 + 1; the d-term sum of positive terms adds d - 1                              d + 8
      h2a   alpha = exp(theta_alpha) on the host 2, the division 1                                                    3
      u     = RN(s h2a)                                                                          eps_u = d + 8 + 3 + 1 = d + 12
      L     log1p's condition number u / ((1 + u) log1p(u)) <= 1, its own 2                           eps_L = d + 14
      t     = RN(alpha L): alpha 2, the product 1                                                     eps_t = d + 17
      e     = exp(-t): the argument's ABSOLUTE error t eps_t becomes relative, exp's own 2            alpha L (d + 17) + 2
      kf    sf2 = exp(2 theta_f) on the host 2, the product 1                  eps_kf = 5 + alpha L (d + 17)
      r     q = RN(1 + u): eps_u u / (1 + u) + 1 <= d + 13; the division 1                            eps_r = d + 14
      hh    = RN(kf r)                                                         eps_hh = eps_kf + d + 15
      p     = RN(u r): eps_u + eps_r + 1 = 2 d + 27, of a value u / (1 + u) <= u
      f     = RN(p - L), f -> u / (1 + u) - log1p(u) in [-u^2 / 2, 0]: ABSOLUTE error (2 d + 27) u + (d + 14) L + |f|
            <= (3 d + 41) u + |f| since L <= u  (the errors p and L inherit from u cancel to second order; the count does
            not use that)
      da    = RN(kf RN(alpha f)): alpha 2, two products 2, kf eps_kf:   |dA| <= Kf alpha ((3 d + 41) u + |f| (eps_kf + 5))
    The bound grows with alpha L (the exponent's absolute error) and with d (the distance's)."""
    u = np.asarray(u, dtype=np.float64)
    aL = float(alpha) * np.log1p(u)
    eps_kf = 5.0 + aL * (d + 17.0)
    f = np.abs(np.asarray(shape_f(u.astype(LD)), dtype=np.float64))
    return eps_kf * U, (eps_kf + d + 15.0) * U, ((3.0 * d + 41.0) * u + f * (eps_kf + 5.0)) * U


def true_u(A, B, cov):
    """u = s / (2 alpha) of the descriptor in fp64 (for k_entry_bound)."""
    w = cov.weights(np.asarray(A).shape[1])
    S = truth.wsqdist(np.asarray(A, dtype=np.float64).astype(LD), np.asarray(B, dtype=np.float64).astype(LD), w)
    return np.asarray(S / (2 * cov.alpha), dtype=np.float64)


def entry_excess(Kf, A, B, cov):
    """Largest |Kf - truth| / (truth * bound) over the entries of an fp64 Kf = k(A, B) without noise."""
    c = RQ(cov.hp, cov.tied)
    t = c.k(np.asarray(A, dtype=np.float64).astype(LD), np.asarray(B, dtype=np.float64).astype(LD))
    err = np.abs(np.asarray(Kf).astype(LD) - t)
    bnd = t * k_entry_bound(true_u(A, B, c), float(c.alpha), np.asarray(A).shape[1])[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, LD(0), err / bnd)
    return float(np.max(r))


def entries_fp64(A, B, cov):
    """(kf, hh, da) of entry_fp64 on the kernels' weighted distance (truth_ard_matern.wsqdist64) with the host's scalars."""
    c64 = cov.fp64()
    d = np.asarray(A).shape[1]
    w = np.array([math.exp(-cov.hp[0 if cov.tied else c]) for c in range(d)])
    alpha, h2a = host_shape(cov.hp[-3])
    s = tam.wsqdist64(np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64), w)
    return entry_fp64(s, math.exp(2 * c64.hp[-2]), alpha, h2a)


# ---------------------------------------------------------------------------------------- leave-one-out
def loo_case(oracle, family, name):
    """tests/truth_loo.py's case for this family: its truth (truth_loo.truth_of goes through the descriptor's `train`), its
    floors and errors; the yardstick is its textbook route (GPML 5.10-5.13 in fp64 on the oracle's potri / potrs, over the
    eight orderings) with this family's explicit derivative matrices, which truth_loo.dK_list picks by class.  The bound is
    the family's own factor, as truth_loo.F_LOO takes a family's existing one."""
    import truth_loo as tl
    c = live(oracle, family, name)
    cov, X, y = c["cov"], c["X"], c["y"]
    tt = tl.truth_of(c["t"], y)
    c64 = cov.fp64()
    n = len(y)

    def textbook(Xp, yp):
        w = c64.weights(Xp.shape[1])
        Kf, H, A = c64._parts(truth.wsqdist(Xp, Xp, w))
        lead = [None] * len(w)

        def per_dim(j, D2):
            lead[j] = H * D2
        truth.wsqdist(Xp, Xp, w, per_dim)
        if c64.tied:
            tot = lead[0]
            for j in range(1, len(w)):
                tot = tot + lead[j]
            lead = [tot]
        dKs = lead + [A, 2 * Kf, 2 * c64.sn2 * np.eye(n)]
        K = Kf + c64.sn2 * np.eye(n)
        Ki = np.asarray(oracle.K_inverse(K))
        a = np.asarray(oracle.Kinvy(K, yp))
        kap = np.diag(Ki).copy()
        mu, var, logp = tl.point_quantities(kap, a, yp, truth.LL_CONST)
        ll = 0.0
        for v in logp:
            ll = ll + v
        g = []
        for dK in dKs:
            Z = Ki @ dK
            g.append(-np.sum((a * (Z @ a) - 0.5 * (1 + a * a / kap) * np.sum(Z * Ki.T, axis=1)) / kap))
        return ll, np.array(g), mu, var, logp

    X64, y64 = np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64)

    def one(idx):
        ll, g, mu, var, logp = textbook(np.ascontiguousarray(X64[idx]), np.ascontiguousarray(y64[idx]))
        inv = np.empty(n, dtype=np.int64)
        inv[idx] = np.arange(n)
        return tl.errors(cov, tt, ll, g, mu[inv], var[inv], logp[inv])
    E = list(truth._pool().map(one, truth.permutations(n)))
    Q = tl.quantities(cov)
    return dict(X=X, y=y, cov=cov, t=c["t"], tt=tt, noise={q: max(e[q] for e in E) for q in Q},
                first={q: E[0][q] for q in Q}, rest={q: max(e[q] for e in E[1:]) for q in Q},
                floor=tl.floors(cov, tt), family=family)


def loo_hold(rep, c, ll, grad, mu, var, logp, tag=""):
    import truth_loo as tl
    e = tl.errors(c["cov"], c["tt"], ll, grad, mu, var, logp)
    for q in tl.quantities(c["cov"]):
        rep.add(tag + q, e[q], c["noise"][q], c["floor"][q], c["cov"].F)
