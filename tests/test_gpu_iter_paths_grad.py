"""Input gradients of the posterior sample paths on the GPU (cugp_iter_paths_grad, SamplePaths.grad)
against numpy.longdouble, with the truths of test_gpu_iter_xgrad (cross, case, handle) and test_gpu_iter_paths (draws), u = 2^-53.

Data term, out_cia = -s_a sum_j G_ij (x_ia - x_ja) V_cj.  Bound  s_a sum_j (gamma_m + E^G_ij) |G_ij| |V_cj| |x_ia - x_ja|,  E^G as
in test_gpu_iter_xgrad; m along k_cov_xgrad_cols: the difference (1), G times it (1), the MFMA's product with V (1), one
addition per entry, 8 entries of each of ceil(n / 32) stages, the ranges (split - 1), and in the finish s_a from the host's
exp (5; 1 / l^2: 3) and its product (1), the sign exact: m = 3 + 8 ceil(n / 32) + split - 1 + 6.
Feature term, out_cia = -amp sum_k sin(p_ik) o_ka W_ck, o = omega / l.  The phase carries k_rff_apply's (d + 7) u S_ik (sin has
slope <= 1), the device library's sin 4 ulp <= 8 u |sin|, the scaled frequency 4 u (the scale 3, its product 1) and sin times
it 1 u: per term  amp |o_ka| |W_ck| ((d + 7) u S_ik + 13 u |sin p_ik|);  the sum, as for the feature product (the MFMA's product,
m additions, fewer ranges than stages, amp from the host 3 and its product 1):  gamma_{m + stages + 6} amp sum_k |sin| |o| |W|.
Both terms: the two bounds at the device's own V plus u (|truth| + bounds) for the one addition.

Shifted data (X + 1e6, Xt + 1e6, n = 257, d = 3, nt = 17, s = 17) holds the same bound: the difference is formed first.  On the
CPU, in fp64 numpy, the coordinate form x_ia sum_j (G_ij V_cj) - sum_j (G_ij V_cj x_ja) on those inputs reaches 2.1e+04 times this
bound; the difference-first fp64 sums reach 0.041 of it.

Largest error / bound on one MI355X: see docs/ACCURACY.md, "Gradients of the sample paths"."""
import numpy as np
import pytest

import test_gpu_iter as ti
import test_gpu_iter_paths as tp
import test_gpu_iter_xgrad as xg
import truth
from conftest import synth
from cugp_amd import gp

pytestmark = pytest.mark.gpu
LD, U, gamma = truth.LD, truth.U, truth.gamma


def data_chain(n, split):
    return 3 + 8 * -(-n // 32) + split - 1 + 6


def data_term(F, B, V, m):
    """-> (truth, bound) [s, nt, d] from xg.cross's F = G (x* - x) s_a and B = E^G |F|, for columns V [s, n]"""
    Vl = V.astype(LD)
    return -np.einsum("ija,cj->cia", F, Vl), np.einsum("ija,cj->cia", gamma(m) * np.abs(F) + B, np.abs(Vl))


def feature_term(hp, ard, Xq, c, Om, b, W):
    """-> (truth, bound) [s, nq, d], longdouble"""
    d, m = Om.shape[1], len(b)
    ell = np.exp(np.asarray(hp[:d] if ard else [hp[0]] * d, dtype=LD))
    Xc, Ot, Wl = Xq.astype(LD) - c.astype(LD), Om.astype(LD) / ell, W.astype(LD)
    Sn = np.sin(Xc @ Ot.T + b.astype(LD))
    S = np.abs(Xc) @ np.abs(Ot).T + np.abs(b)
    amp = np.sqrt(2 * np.exp(2 * LD(hp[-2])) / m)
    per = (d + 7) * U * S + 13 * U * np.abs(Sn) + gamma(m + -(-m // 32) + 6) * np.abs(Sn)
    return -amp * np.einsum("ik,ka,ck->cia", Sn, Ot, Wl), amp * np.einsum("ik,ka,ck->cia", per, np.abs(Ot), np.abs(Wl))


def update_paths(g, V):
    """SamplePaths that carry V alone (part="update" looks at nothing else)"""
    return gp.SamplePaths(g, np.zeros((1, g.d)), np.zeros(1), np.zeros((len(V), 1)), V, None, None)


DATA = sorted({("se", n, 17, 17, 3, 0) for n in (1, 31, 32, 33, 65, 257)} | {("se", 65, nt, 17, 3, 0) for nt in (1, 15, 16, 64, 65, 70)}
              | {("se", 65, 17, s, 3, 0) for s in (1, 16, 17, 64)} | {("se", 65, 17, 17, d, 0) for d in (1, 3, 4, 5, 16, 17, 33)}
              | {("se", 257, 17, 17, 3, sp) for sp in (1, 2, 3)}
              | {(f, 65, 17, 17, 17, 0) for f in ("se_ard", "matern32", "matern52", "matern32_ard", "matern52_ard", "rq", "rq_ard")})


@pytest.mark.parametrize("family,n,nt,s,d,split", DATA)
def test_data_term_against_longdouble(family, n, nt, s, d, split):
    X, Xt, F, B = xg.cross(family, n, d, nt)
    V = ti.vectors(s, n, seed=3)
    got = gp.IterativeGP.plan(nt, n, 1, split)["split"]
    assert split == 0 or got == split
    want, bound = data_term(F, B, V, data_chain(n, got))
    out = update_paths(xg.handle(family, n, d, X, split), V).grad(Xt, "update")
    ti.hold(out, want, bound, "paths grad, data term %s" % ((family, n, nt, s, d, split),))


FEATURES = sorted({("se", m, 3, 0) for m in (1, 31, 32, 33, 100)} | {(f, 33, d, 0) for f in ("se", "matern52_ard") for d in (1, 16, 17)}
                  | {("se", 100, 3, sp) for sp in (1, 3)} | {("rq_ard", 33, 3, 0)})


@pytest.mark.parametrize("family,m,d,split", FEATURES)
def test_feature_term_against_longdouble(family, m, d, split):
    hp = ti.case(family, 65, d)[2]
    Om, b, W, _ = tp.draws(family, d, m, 17, 65)
    Xq, c = synth(65, d=d, seed=11, scale=4.0 if d <= 3 else 1.8)[0], np.linspace(-0.5, 0.5, d)
    out = gp.SamplePaths(ti.handle(family, 65, d, split), Om, b, W, np.zeros((17, 65)), c, None).grad(Xq, "prior")
    want, bound = feature_term(hp, family.endswith("ard"), Xq, c, Om, b, W)
    ti.hold(out, want, bound, "paths grad, feature term %s" % ((family, m, d, split),))


@pytest.mark.parametrize("family", ["se", "rq_ard"])
def test_both_terms_of_real_paths(family):
    n, nt, m, s = 150, 70, 33, 3
    hp = ti.case(family, n, 3)[2]
    X, Xt, F, B = xg.cross(family, n, 3, nt)
    Om, b, W, Eps = tp.draws(family, 3, m, s, n)
    paths = ti.handle(family, n, 3).sample_paths(s, Omega=Om, b=b, W=W, Eps=Eps, tol=ti.TOL, max_iter=4 * n, check_every=7)
    assert np.all(paths.info[:, 2] == 1)
    wd, bd = data_term(F, B, paths.V, data_chain(n, 1))
    wf, bf = feature_term(hp, family.endswith("ard"), Xt, paths.origin, Om, b, W)
    ti.hold(paths.grad(Xt), wf + wd, bd + bf + U * (np.abs(wf + wd) + bd + bf), "paths grad, both terms " + family)


def test_shifted_data_keeps_the_bound():
    X, Xt, F, B = xg.cross("se", 257, 3, 17, 1e6)
    V = ti.vectors(17, 257, seed=3)
    want, bound = data_term(F, B, V, data_chain(257, 1))
    ti.hold(update_paths(xg.handle("se", 257, 3, X), V).grad(Xt, "update"), want, bound, "paths grad, shifted by 1e6")


def test_bits():
    X, Xt, _, _ = xg.cross("matern52_ard", 65, 3, 70)
    Om, b, W, _ = tp.draws("matern52_ard", 3, 100, 17, 65)
    V, g = ti.vectors(17, 65, seed=3), xg.handle("matern52_ard", 65, 3, X)
    paths = gp.SamplePaths(g, Om, b, W, V, g._origin, None)
    out = paths.grad(Xt)
    assert np.array_equal(out, paths.grad(Xt))
    for c in (0, 5, 16):
        assert np.array_equal(out[c], gp.SamplePaths(g, Om, b, W[c:c + 1], V[c:c + 1], g._origin, None).grad(Xt)[0]), c
    pick = np.arange(2, 70, 4)                         # 17 of the 70 points, each with other neighbours and another place in its block
    assert np.array_equal(out[:, pick], paths.grad(Xt[pick]))


def test_one_column_agrees_with_input_grad():
    """The same sums in another order (k_cov_xgrad: per lane, then the fk groups): within the two paths' bounds together."""
    X, Xt, F, B = xg.cross("rq_ard", 257, 3, 17)
    V, g = ti.vectors(2, 257, seed=3)[:1], xg.handle("rq_ard", 257, 3, X)
    bound = data_term(F, B, V, data_chain(257, 1))[1][0] + xg.forms(F, B, V, xg.chain(257, 1))[1]
    ti.hold(update_paths(g, V).grad(Xt, "update")[0], g.input_grad(Xt, V).astype(LD), bound, "paths grad beside input_grad")
