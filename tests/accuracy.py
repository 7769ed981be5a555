"""The accuracy harness of the GPU tests and of their CPU counterparts -- TEST INFRASTRUCTURE; a plain module beside
tests/truth.py.  For every covariance family (a descriptor of truth.py) and checked quantity q

    err_gpu(q) <= F * max(noise(q), floor(q))

  err    LL relative to |LL|; each gradient component relative to max|g|; the largest absolute error of the means, of
         the variances, of the joint covariance; alpha and 64 rows of K^-1 relative to the largest entry
  noise  what the CPU oracle's reference-order fp64 arithmetic delivers on the same input (truth.noise_level, through
         the family's evaluator): its largest error against the truth over the data as given and 7 row permutations.
         The joint covariance is held to the variances' yardstick (its diagonal IS the variances, and every entry is
         the same expression k(s, t) - w_s . w_t); alpha and K^-1 to the oracle's own potrs / potri
  floor  4 ulp of the quantity's scale (|LL|, max|g|, max|mean|, sf2 + sn2; the largest entry for alpha, K^-1)
  F      the descriptor's (truth.F, F_ARD, F_MATERN; F_SOLVE for alpha and K^-1), set from a stand-in measured on the
         CPU (LAPACK / BLAS order), never from the GPU's errors: docs/ACCURACY.md holds the tables.

`Report` prints every figure before it asserts; `live` computes truth, yardsticks and floors of a live case once per
process, whichever test modules ask; `hold_live_case` and `hold_fixture_case` are the bodies every family's accuracy
tests share -- a family brings its descriptor, its case list and a factory for its handle.
"""
import numpy as np

import truth

LD = truth.LD
U4 = truth.U4


class Report:
    """Collects (quantity, error, yardstick) of one case, prints each, asserts all at the end.  F: the factor of the
    covariance `cov` unless a row names its own."""

    def __init__(self, case, cov=None):
        self.case, self.cov, self.bad = case, cov, []

    def add(self, q, err, noise, floor, F=None):
        F = self.cov.F if F is None else F
        yard = max(noise, floor)
        ratio = float(err) / yard
        print("ACC %-22s %-18s err %.3e  noise %.3e  floor %.3e  ratio %6.2f" % (self.case, q, float(err), noise, floor, ratio))
        if not ratio <= F:                           # NaN fails
            self.bad.append((q, float(err), yard, ratio, F))

    def add_all(self, tag, e, noise, fl, F=None):
        """Every quantity of the family that `e` holds, under its own name."""
        for q in self.cov.quantities:
            if q in e:
                self.add(tag + q, e[q], noise[q], fl[q], F)

    def check(self):
        assert not self.bad, "%s: (quantity, error, yardstick, ratio, F) beyond F yardsticks: %s" % (self.case, self.bad)


# ------------------------------------------------------------------ the cases, computed once
_CASES = {}


def case_at(oracle, cov, X, y, Xt, t, rows=None):
    """Predictions of the truth t at Xt, the yardsticks there (with `rows` also for alpha and K^-1) and the floors."""
    tm, tv = t.predict(Xt)
    out = truth.yardstick(oracle, cov, X, y, Xt, t, tm, tv, rows)
    c = dict(X=X, y=y, Xt=Xt, cov=cov, t=t, tm=tm, tv=tv, noise=out[0], first=out[1], rest=out[2],
             floor=truth.floors(cov, truth.scales(cov, t.ll, t.grad, tm)))
    if rows is not None:
        c.update(rows=rows, solve=out[3])
    return c


def live(oracle, family, name):
    """Inputs, truth, predictions at the 64 points, yardsticks (alpha and K^-1 included) and floors of a live case of
    a family of truth.FAMILIES."""
    if (family, name) not in _CASES:
        X, y, Xt, cov = truth.family_inputs(family, name)
        _CASES[family, name] = case_at(oracle, cov, X, y, Xt, truth.Truth(X, y, cov), truth.solve_rows(len(y)))
    return _CASES[family, name]


def wide(oracle, family, name, nt):
    """The same at nt test points (truth.wide_inputs), on the live case's truth: it does not depend on them."""
    X, y, Xt, cov = truth.wide_inputs(name, nt, family)
    c = case_at(oracle, cov, X, y, Xt, live(oracle, family, name)["t"])
    c["tcov"] = c["t"].joint(Xt, with_noise=False)[1]
    return c


def standin_ratios(c):
    """Stand-in error / max(noise, floor) of a case of `live`, per quantity of the family and for alpha and K^-1: its
    row of the stand-in table in docs/ACCURACY.md (of the BLAS this runs on)."""
    if "standin" not in c:
        st = truth.standin(c["cov"], c["X"], c["y"], c["Xt"], solve=True)
        e = truth.errors(c["cov"], *st[:4], c["t"].ll, c["t"].grad, c["tm"], c["tv"])
        es = truth.solve_errors(st[4], st[5], c["t"], c["rows"])
        c["standin"] = ({q: e[q] / max(c["noise"][q], c["floor"][q]) for q in c["cov"].quantities},
                        {q: es[q] / max(c["solve"][q], U4) for q in truth.SOLVE_QUANTITIES})
    return c["standin"]


def assert_yardstick_is_sane(c, tag, quantities=None):
    """The oracle's error on the data as given is no outlier among the 7 permuted evaluations (within F of the largest
    of them, floored like the bound), and no yardstick exceeds YARDSTICK_CAP of its scale: a broken truth or oracle
    cannot silently loosen the GPU test."""
    for q in quantities or c["cov"].quantities:
        assert c["first"][q] <= c["cov"].F * max(c["rest"][q], c["floor"][q]), (tag, q, c["first"][q], c["rest"][q])
        scale = c["floor"][q] / U4                # 1 for LL and gradient (relative errors), else the quantity's scale
        assert c["noise"][q] <= truth.YARDSTICK_CAP * scale, (tag, q, c["noise"][q], scale)


def wide_standin_ratios(tag, c):
    """Stand-in error / max(noise, floor) of the means, the variances and the joint covariance (the worse of with and
    without noise; the variances' yardstick and the cov floor, as the GPU tests hold it) of a case of `wide`."""
    cov, noise, fl = c["cov"], c["noise"], c["floor"]
    _, _, mean, var, lat = truth.standin(cov, c["X"], c["y"], c["Xt"], joint=True)
    cn = lat + float(cov.sn2) * np.eye(len(lat))
    e = truth.joint_errors(mean, var, cn, lat, c["tm"], c["tv"], c["tcov"], cov.sn2)
    r = dict(mean=e["mean"] / max(noise["mean"], fl["mean"]), var=e["var"] / max(noise["var"], fl["var"]),
             cov=max(e["cov_noise"], e["cov_latent"]) / max(noise["var"], fl["cov"]))
    print("STANDIN-WIDE %-28s " % tag + "  ".join("%s %.2f" % kv for kv in r.items())
          + "  | yardstick " + " ".join("%s %.1e" % (q, max(noise[q], fl[q])) for q in ("mean", "var")))
    return r


# ------------------------------------------------------------------ the shared bodies of the GPU tests
def hold_live_case(rep, c, make_handle, overlaps=(True,), joint=False, fresh=None):
    """A live case `c` on the GPU: the LL-only path on a fresh handle (forward substitution inside the factorisation;
    `fresh(g)` sees that handle first), then on a fresh handle per overlap setting -- set before its first evaluation:
    a handle that has evaluated this point answers from what it holds, whatever the setting says by then --
    loglik_grad, K^-1 exactly symmetric, alpha and 64 rows of K^-1, prediction at the 64 test points (one of them a
    training row); with `joint` the joint covariance with and without noise on the last handle.
    make_handle(overlap=None) -> a handle of the family with its hyper-parameters set."""
    X, y, Xt, t, noise, fl = c["X"], c["y"], c["Xt"], c["t"], c["noise"], c["floor"]
    g = make_handle()
    if fresh is not None:
        fresh(g)
    ll_only = g.compute_loglikelihood(X, y)                       # first call on a fresh handle: nothing to reuse
    rep.add("ll_only", abs(LD(ll_only) - t.ll) / abs(t.ll), noise["ll"], fl["ll"])
    g.close()
    for overlap in overlaps:
        g = make_handle(overlap)
        tag = "" if overlap else "nooverlap_"
        ll, gr = g.loglik_grad(X, y)
        assert gr.shape == t.grad.shape
        rep.add_all(tag, truth.errors_ll_grad(c["cov"], ll, gr, t.ll, t.grad), noise, fl)
        Ki = g.get_K_inverse()
        assert np.array_equal(Ki, Ki.T)
        es = truth.solve_errors(g.get_alpha(), Ki, t, c["rows"])
        for q in truth.SOLVE_QUANTITIES:
            rep.add(tag + q, es[q], c["solve"][q], U4, truth.F_SOLVE)
        m, v = g.compute_test_means_and_variances(X, y, Xt)
        rep.add_all(tag, truth.errors_pred(m, v, c["tm"], c["tv"]), noise, fl)
        if not overlap:
            g.close()
    if joint:
        for with_noise in (True, False):
            tmj, tcov = t.joint(Xt, with_noise)
            mj, cov = g.compute_test_joint(X, y, Xt, with_noise=with_noise)
            tag = "joint_noise_" if with_noise else "joint_latent_"
            rep.add(tag + "mean", np.max(np.abs(mj.astype(LD) - tmj)), noise["mean"], fl["mean"])
            rep.add(tag + "cov", np.max(np.abs(cov.astype(LD) - tcov)), noise["var"], fl["cov"])
    g.close()
    rep.check()


def hold_fixture_case(rep, f, X, y, Xt, cov, make_handle):
    """A committed fixture f (tests/golden/make_truth.py: load) on the GPU: the LL-only path on a fresh handle, then
    loglik_grad and the prediction at the 64 test points on another."""
    fl = truth.floors(cov, truth.scales(cov, f["ll"], f["grad"], f["mean"]))
    g = make_handle()
    ll_only = g.compute_loglikelihood(X, y)
    rep.add("ll_only", abs(LD(ll_only) - f["ll"]) / abs(f["ll"]), f["noise"]["ll"], fl["ll"])
    g.close()
    g = make_handle()
    ll, gr = g.loglik_grad(X, y)
    m, v = g.compute_test_means_and_variances(X, y, Xt)
    g.close()
    rep.add_all("", truth.errors(cov, ll, gr, m, v, f["ll"], f["grad"], f["mean"], f["var"]), f["noise"], fl)
    rep.check()
