"""GPU accuracy: the HIP path held to fp64 ROUNDING against an extended-precision truth (tests/truth.py), not to the
1e-8 / 1e-6 of the parity suite.  For every case and checked quantity q (tests/accuracy.py holds the shared harness)

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

import accuracy
import truth
from accuracy import Report
from conftest import GOLDEN, synth

sys.path.insert(0, GOLDEN)
import make_truth  # noqa: E402

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not truth.EXTENDED, reason="numpy.longdouble is not an extended-precision type here")]


@pytest.fixture(scope="module")
def gp_mod():
    import cugp_amd.gp as gp
    return gp


def handle(gp_mod, X, cov, overlap=None):
    g = gp_mod.Covsum(*X.shape)
    if overlap is not None:
        g.set_overlap(overlap)
    g.set_loghyperparam(cov.hp)
    return g


# ------------------------------------------------------------------ live cases
@pytest.mark.parametrize("name", list(truth.LIVE_CASES))
def test_live_case(gp_mod, oracle, name):
    """loglik_grad, the LL-only path (forward substitution inside the factorisation), prediction at 64 test points (one
    of them a training row), alpha, 64 rows of K^-1, and on the three smallest and two largest cases the joint
    covariance with and without noise.  n1025_dense also on a handle of its own with the inverse streams off."""
    c = accuracy.live(oracle, "se", name)
    accuracy.hold_live_case(Report(name, c["cov"]), c, lambda overlap=None: handle(gp_mod, c["X"], c["cov"], overlap),
                            overlaps=(False, True) if name == "n1025_dense" else (True,), joint=name in truth.JOINT_CASES)


# ------------------------------------------------------------------ fixture cases
@pytest.mark.parametrize("name", ["n2049", "n4200"])
def test_fixture_case(gp_mod, name):
    """17 tiles and 33 tiles (the largest size of the classic schedule) against the committed truth."""
    X, y, Xt, cov, _ = make_truth.inputs(name)
    accuracy.hold_fixture_case(Report(name, cov), make_truth.load(name), X, y, Xt, cov, lambda: handle(gp_mod, X, cov))


def test_fixture_bcm(gp_mod):
    """Three 1500-row experts of the si24000 data at HP_BCM, factored as one group: summed LL and gradient
    (cugp_bcm_loglik_grad) and the product-of-experts prediction (cugp_bcm_predict)."""
    f = make_truth.load("bcm3x1500")
    X, y, Xt, cov, experts = make_truth.inputs("bcm3x1500")
    fl = truth.floors(cov, truth.scales(cov, f["ll"], f["grad"], f["mean"]))
    rep = Report("bcm3x1500", cov)
    b = gp_mod.BCM.split(X, y, experts)
    assert b.rows == [r for _, r in truth.bcm_rows(len(y), experts)]
    b.set_BCM_log_hyperparam(cov.hp)
    ll, gr, _ = b.loglik_grad()
    m, v = b.compute_BCM_test_means_and_var(Xt)
    b.close()
    rep.add_all("", truth.errors(cov, ll, gr, m, v, f["ll"], f["grad"], f["mean"], f["var"]), f["noise"], fl)
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
