"""GPU accuracy: the HIP path held to fp64 ROUNDING against an extended-precision truth (tests/truth.py), not to the
1e-8 / 1e-6 of the parity suite.  For every case and checked quantity q

    err_gpu(q) <= F * max(noise(q), floor(q))

  err    LL relative to |LL|; each gradient component relative to max|g|; the largest absolute error of the means, of
         the variances, of the joint covariance; alpha and 64 rows of K^-1 relative to the largest entry
  noise  what the CPU oracle's reference-order fp64 arithmetic delivers on the same input: its largest error against
         the truth over the data as given and 7 row permutations (live, or from tests/golden/truth/<case>.json).  The
         joint covariance is held to the variances' yardstick (its diagonal IS the variances, and every entry is the
         same expression k(s, t) - w_s . w_t); alpha and K^-1 to the oracle's own potrs / potri
  floor  4 ulp of the quantity's scale (|LL|, max|g|, max|mean|, sf2 + sn2; the largest entry for alpha, K^-1)
  F      8 (32 for alpha and K^-1), set from a stand-in measured on the CPU (LAPACK / BLAS order), never from the
         GPU's errors: docs/ACCURACY.md holds the table, and the GPU's measured ratios beside it.

Every figure is printed before it is asserted ("ACC <case> <quantity> err yardstick ratio"; run with -s to keep them).
The factor itself is held to Higham's componentwise bound on sampled rows (test_factor_residual).
One process, one device; nothing outside the tree is read.
"""
import sys

import numpy as np
import pytest

import truth
from conftest import GOLDEN, synth

sys.path.insert(0, GOLDEN)
import make_truth  # noqa: E402

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not truth.EXTENDED, reason="numpy.longdouble is not an extended-precision type here")]

LD = truth.LD
U4 = 4 * 2.0 ** -52


@pytest.fixture(scope="module")
def gp_mod():
    import cugp_amd.gp as gp
    return gp


class Report:
    """Collects (quantity, error, yardstick) of one case, prints each, asserts all at the end."""

    def __init__(self, case):
        self.case, self.bad = case, []

    def add(self, q, err, noise, floor, F=truth.F):
        yard = max(noise, floor)
        ratio = float(err) / yard
        print("ACC %-14s %-18s err %.3e  noise %.3e  floor %.3e  ratio %6.2f" % (self.case, q, float(err), noise, floor, ratio))
        if not ratio <= F:                           # NaN fails
            self.bad.append((q, float(err), yard, ratio, F))

    def check(self):
        assert not self.bad, "%s: (quantity, error, yardstick, ratio, F) beyond F yardsticks: %s" % (self.case, self.bad)


def add_six(rep, tag, e, noise, fl):
    for q in truth.QUANTITIES:
        if q in e:
            rep.add(tag + q, e[q], noise[q], fl[q])


# ------------------------------------------------------------------ live cases
_CASE = {}


def live(oracle, name):
    """Inputs, truth and yardsticks of a live case, computed once per module."""
    if name not in _CASE:
        X, y, Xt, hp = truth.live_inputs(name)
        t = truth.Truth(X, y, hp)
        tm, tv = t.predict(Xt)
        noise, _, _ = truth.noise_level(oracle, X, y, hp, Xt, t.ll, t.grad, tm, tv)
        rows = truth.solve_rows(len(y))
        solve = truth.noise_level_solve(oracle, X, y, hp, t, rows)
        _CASE[name] = dict(X=X, y=y, Xt=Xt, hp=hp, t=t, tm=tm, tv=tv, noise=noise, solve=solve, rows=rows,
                           floor=truth.floors(truth.scales(hp, t.ll, t.grad, tm)))
    return _CASE[name]


@pytest.mark.parametrize("name", list(truth.LIVE_CASES))
def test_live_case(gp_mod, oracle, name):
    """loglik_grad, the LL-only path (forward substitution inside the factorisation), prediction at 64 test points (one
    of them a training row), alpha, 64 rows of K^-1, and on the three smallest and two largest cases the joint
    covariance with and without noise.  n1025_dense also on a handle of its own with the inverse streams off."""
    c = live(oracle, name)
    X, y, Xt, hp, t = c["X"], c["y"], c["Xt"], c["hp"], c["t"]
    n, d = X.shape
    rep = Report(name)

    g = gp_mod.Covsum(n, d)
    g.set_loghyperparam(hp)
    ll_only = g.compute_loglikelihood(X, y)                       # first call on a fresh handle: nothing to reuse
    rep.add("ll_only", abs(LD(ll_only) - t.ll) / abs(t.ll), c["noise"]["ll"], c["floor"]["ll"])
    g.close()

    # a fresh handle per overlap setting, set before its first evaluation: a handle that has evaluated this point
    # answers from what it holds, whatever the setting says by then
    for overlap in ((False, True) if name == "n1025_dense" else (True,)):
        g = gp_mod.Covsum(n, d)
        g.set_overlap(overlap)
        g.set_loghyperparam(hp)
        tag = "" if overlap else "nooverlap_"
        ll, gr = g.loglik_grad(X, y)
        add_six(rep, tag, truth.errors_ll_grad(ll, gr, t.ll, t.grad), c["noise"], c["floor"])
        Ki = g.get_K_inverse()
        assert np.array_equal(Ki, Ki.T)
        es = truth.solve_errors(g.get_alpha(), Ki, t, c["rows"])
        for q in truth.SOLVE_QUANTITIES:
            rep.add(tag + q, es[q], c["solve"][q], U4, truth.F_SOLVE)
        m, v = g.compute_test_means_and_variances(X, y, Xt)
        add_six(rep, tag, truth.errors_pred(m, v, c["tm"], c["tv"]), c["noise"], c["floor"])
        if not overlap:
            g.close()
    if name in truth.JOINT_CASES:
        for with_noise in (True, False):
            tmj, tcov = t.joint(Xt, with_noise)
            mj, cov = g.compute_test_joint(X, y, Xt, with_noise=with_noise)
            tag = "joint_noise_" if with_noise else "joint_latent_"
            rep.add(tag + "mean", np.max(np.abs(mj.astype(LD) - tmj)), c["noise"]["mean"], c["floor"]["mean"])
            rep.add(tag + "cov", np.max(np.abs(cov.astype(LD) - tcov)), c["noise"]["var"], c["floor"]["cov"])
    g.close()
    rep.check()


# ------------------------------------------------------------------ fixture cases
def fixture_yardsticks(f):
    fl = truth.floors(truth.scales(f["hp"], f["ll"], f["grad"], f["mean"]))
    return f["noise"], fl


@pytest.mark.parametrize("name", ["n2049", "n4200"])
def test_fixture_case(gp_mod, name):
    """17 tiles and 33 tiles (the largest size of the classic schedule) against the committed truth."""
    f = make_truth.load(name)
    X, y, Xt, hp, _ = make_truth.inputs(name)
    noise, fl = fixture_yardsticks(f)
    rep = Report(name)
    g = gp_mod.Covsum(*X.shape)
    g.set_loghyperparam(hp)
    ll_only = g.compute_loglikelihood(X, y)
    rep.add("ll_only", abs(LD(ll_only) - f["ll"]) / abs(f["ll"]), noise["ll"], fl["ll"])
    g.close()
    g = gp_mod.Covsum(*X.shape)
    g.set_loghyperparam(hp)
    ll, gr = g.loglik_grad(X, y)
    m, v = g.compute_test_means_and_variances(X, y, Xt)
    g.close()
    add_six(rep, "", truth.errors(ll, gr, m, v, f["ll"], f["grad"], f["mean"], f["var"]), noise, fl)
    rep.check()


def test_fixture_bcm(gp_mod):
    """Three 1500-row experts of the si24000 data at HP_BCM, factored as one group: summed LL and gradient
    (cugp_bcm_loglik_grad) and the product-of-experts prediction (cugp_bcm_predict)."""
    f = make_truth.load("bcm3x1500")
    X, y, Xt, hp, experts = make_truth.inputs("bcm3x1500")
    noise, fl = fixture_yardsticks(f)
    rep = Report("bcm3x1500")
    b = gp_mod.BCM.split(X, y, experts)
    assert b.rows == [r for _, r in truth.bcm_rows(len(y), experts)]
    b.set_BCM_log_hyperparam(hp)
    ll, gr, _ = b.loglik_grad()
    m, v = b.compute_BCM_test_means_and_var(Xt)
    b.close()
    add_six(rep, "", truth.errors(ll, gr, m, v, f["ll"], f["grad"], f["mean"], f["var"]), noise, fl)
    rep.check()


# ------------------------------------------------------------------ the factor
(PANEL, NEAR, PANEL_MIN_NT, SUBPANEL) = (8, 9, 10, 17)             # kernels.h TUNE_*, as tests/test_gpu_launch_paths.py
SCHED = {PANEL_MIN_NT: 1, PANEL: 4, NEAR: 12, SUBPANEL: 2}
TILE = 128
EXTRA_ULPS = truth.POTRF_EXTRA_ULPS        # gamma_(n + 15) where Higham has gamma_(n + 1): see test_factor_residual


@pytest.mark.parametrize("n,cfg", [(515, {}), (1300, {}), (1500, SCHED), (2049, {}), (4200, {}), (6100, {}),
                                   (6100, {SUBPANEL: 2})],
                         ids=["515", "1300", "1500-two-speed-P4-near12-S2", "2049", "4200", "6100", "6100-S2"])
def test_factor_residual(gp_mod, n, cfg):
    """The factor fetched after an evaluation, on 64 fixed-seed rows plus the rows at every 128-tile boundary +- 1,
    componentwise against the library's own K (compute_K_train: the device exp is not part of it):

        |K - L L^T|_ij <= gamma_(n+15) (|L||L^T|)_ij,      gamma_k = k u / (1 - k u), u = 2^-53

    Derived, not measured.  Higham, Accuracy and Stability, Thm 10.3: gamma_(n+1) |L||L^T| for ANY order of the sums,
    given square roots and divisions within one ulp.  The diagonal micro tiles (panel_factor) instead eliminate in
    LDL^T form with y ~ d^-1/2 from v_rsq_f64 and one third-order step (truncation 3e-24, then 5 rounded operations:
    |y sqrt(d) - 1| <= 4u, so d y^2 = 1 + e_y, |e_y| <= 9u): l_ic = fl(m_ic y_c), and the update term is
    fma(fl(l_ic y_c), m_jc, .) = l_ic l_jc (1 + d1) / (1 + d2) -- two rounding factors per term beyond the textbook
    product, none from y; the closing term is m_ic = l_ic l_cc / ((1 + e_y)(1 + d3)(1 + d4)): 11 more.  With the fma the
    textbook product rounding is absent, but it is kept: index n + 1 + 2 + 11 + 1 spare = n + 15 (EXTRA_ULPS).

    The theorem also assumes that the rows below a block are solved by substitution, while k_trsm_inv64 multiplies them
    by explicit inverses of the block's two 64 x 64 halves (X0 = A0 T00^T, Z1 = A1 - X0 L10^T, X1 = Z1 T11^T), whose
    residual grows with |L_BB^-T||L_BB^T| of the block.  No allowance is made for that: the bound above is asserted as
    it stands, so a panel solve that loses more than the substitution's constant leaves for it shows up here.
    (Measured: the largest residual is 0.01 .. 0.27 of the bound.)

    L's strict upper triangle is exactly zero and its diagonal positive, as cugp_get_cholesky documents (upper zeroed;
    the padding never leaves the device)."""
    X, y = synth(n, d=3, seed=n, scale=8.0)
    g = gp_mod.Covsum(n, 3)
    g.set_data(X, y)
    for k, v in cfg.items():
        g.set_tuning(k, v)
    g.set_loghyperparam(truth.HP_A)
    K = g.compute_K_train()
    g.loglik_grad()
    L = g.get_cholesky()
    g.close()
    assert L.shape == (n, n) and np.all(np.isfinite(L))
    assert not np.any(np.triu(L, 1)), "strict upper triangle of the fetched factor is not zero"
    assert np.all(np.diag(L) > 0)
    edges = [r for b in range(TILE, n, TILE) for r in (b - 1, b, b + 1) if r < n]
    rows = sorted(set(np.random.default_rng(n).choice(n, 64, replace=False).tolist() + edges + [0, n - 1]))
    res, bnd = truth.potrf_residual_rows(K, L, rows)
    worst = max(float(np.max(r / (truth.gamma(n + EXTRA_ULPS) * b))) for r, b in zip(res, bnd))
    print("ACC factor n=%d %s: %d rows, largest residual / (gamma_(n+%d) |L||L^T|) %.4f" % (n, cfg, len(rows), EXTRA_ULPS, worst))
    assert worst <= 1.0, (n, cfg, worst)
