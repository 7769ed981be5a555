"""The nearest-neighbour (Vecchia) GP on the GPU (gp.NeighborGP, cugp_nn_*) against truth.py's longdouble Truth:
    l_i = Truth(block_i).ll - Truth(neighbours_i).ll,  the gradient formed the same way,  the prediction from the definition.
Bound: F_NN max(yardstick, 4 ulp |truth|), the yardstick being the error of the SAME definition evaluated in numpy fp64
(truth.standin in place of Truth) against its longdouble value: it carries each block's conditioning.

F_NN: the smallest power of two at or above twice the largest GPU error / yardstick ratio over CASES (docs/ACCURACY.md,
"Neighbour GP", holds the ratios).  Measured on an MI355X: the largest ratio is 9.49 (LL of rq_ard n261 m15 d1; the
gradient's largest is 0.93, the mean's 0.89, the variance's 0.64), twice that 19.0."""
import functools

import numpy as np
import pytest

import truth
import truth_ard_matern as tam
import truth_rq
from conftest import synth
from cugp_amd import gp

RATIO_WORST = 9.49
F_NN = 32

HP = [0.9, 0.2, -1.0]             # moderate length scale in synth's box of half-width 4


def _lengths(d):
    return np.linspace(0.7, 1.3, d).tolist()


# family -> (kernel=, ard=, d -> theta, theta -> descriptor)
FAMILIES = {
    "se": ("se", False, lambda d: HP, truth.SE),
    "matern32": ("matern32", False, lambda d: HP, lambda hp: truth.Matern(hp, truth.MATERN32)),
    "matern52": ("matern52", False, lambda d: HP, lambda hp: truth.Matern(hp, truth.MATERN52)),
    "ard": ("se", True, lambda d: _lengths(d) + HP[1:], truth.ARD),
    "matern32_ard": ("matern32_ard", False, lambda d: _lengths(d) + HP[1:], lambda hp: tam.ARDMatern(hp, truth.MATERN32)),
    "matern52_ard": ("matern52_ard", False, lambda d: _lengths(d) + HP[1:], lambda hp: tam.ARDMatern(hp, truth.MATERN52)),
    "rq_ard": ("rq_ard", False, lambda d: _lengths(d) + [0.4] + HP[1:], truth_rq.RQ),
    "rq": ("rq", False, lambda d: [HP[0], 0.4] + HP[1:], lambda hp: truth_rq.RQ(hp, tied=True)),
}
# (n, m, d): both sides of each padded block size and packing; n = 1: no neighbour; n = m + 1: every block still growing; 70 at
# m = 63: a growing block beside full ones; 261: several workgroup partials and a ragged last workgroup at every packing;
# d = 17: one feature beyond a chunk
SHAPES = [(1, 1, 1), (2, 1, 3), (16, 15, 17), (17, 16, 1), (32, 31, 3), (33, 32, 17), (64, 63, 1), (70, 63, 3),
          (261, 1, 17), (261, 15, 1), (261, 16, 3), (261, 31, 17), (261, 32, 1), (261, 63, 3)]
EXACT = [(16, 15, 3), (33, 32, 3), (64, 63, 3)]          # idx_i = 0 .. i - 1: the exact GP of all rows
CASES = [(f, n, m, d, False) for f in ("se", "rq_ard") for n, m, d in SHAPES]
CASES += [(f, 261, 16, 3, False) for f in FAMILIES if f not in ("se", "rq_ard")]
CASES += [(f, n, m, d, True) for f in ("se", "rq_ard") for n, m, d in EXACT]
NT = 5


def _ev_truth(cov):
    def ev(X, y, Xt):
        t = truth.Truth(X, y, cov, keep=False)
        return (t.ll, t.grad) + tuple(t.predict(Xt))
    return ev


def _ev_fp64(cov):
    return lambda X, y, Xt: truth.standin(cov, X, y, Xt)


def reference(ev, X, y, idx, Xt, idx_t):
    """(LL, g, mean, var) of the definition, every block and neighbour block through ev(X, y, Xt) -> (ll, grad, mean, var)."""
    ll, g = 0, 0
    for i in range(len(y)):
        nb = [j for j in idx[i] if j >= 0]
        lb, gb = ev(X[nb + [i]], y[nb + [i]], X[:1])[:2]
        ln, gn = ev(X[nb], y[nb], X[:1])[:2] if nb else (0, 0)
        ll, g = ll + (lb - ln), g + (gb - gn)
    pred = [ev(X[[j for j in idx_t[t] if j >= 0]], y[[j for j in idx_t[t] if j >= 0]], Xt[t:t + 1])[2:] for t in range(len(Xt))]
    return ll, g, np.array([p[0][0] for p in pred]), np.array([p[1][0] for p in pred])


@functools.lru_cache(maxsize=None)
def inputs(family, n, m, d, exact):
    """the data, the index rows and the fp64 restatement of a case (which raises where a block is not positive definite)"""
    kernel, ard, theta, descriptor = FAMILIES[family]
    X, y = synth(n, d=d, seed=3 * n + d + m, scale=4.0)
    hp = theta(d)
    cov = descriptor(hp)
    idx = gp.nn_neighbors(X, m)
    if exact:
        idx = np.array([[j if j < i else -1 for j in range(m)] for i in range(n)], dtype=np.int32)
    Xt = synth(NT, d=d, seed=7, scale=4.0)[0]
    idx_t = gp.nn_neighbors(X, m, Xt)
    fp = reference(_ev_fp64(cov), X, y, idx, Xt, idx_t)
    return dict(kernel=kernel, ard=ard, cov=cov, X=X, y=y, hp=hp, idx=idx, Xt=Xt, idx_t=idx_t, fp64=fp)


@functools.lru_cache(maxsize=None)
def case(family, n, m, d, exact):
    """the inputs with the longdouble truth, the yardstick and the 4 ulp floors of (LL, g, mean, var), computed once"""
    c = dict(inputs(family, n, m, d, exact))
    cov, X, y = c["cov"], c["X"], c["y"]
    tr = reference(_ev_truth(cov), X, y, c["idx"], c["Xt"], c["idx_t"])
    if exact:
        t = truth.Truth(X, y, cov, keep=False)
        assert abs(t.ll - tr[0]) <= 1e-15 * abs(t.ll) and np.max(np.abs(t.grad - tr[1])) <= 1e-15 * np.max(np.abs(t.grad))
        tr = (t.ll, t.grad) + tr[2:]
    scale = (abs(tr[0]), np.max(np.abs(tr[1])), np.max(np.abs(tr[2])), cov.sf2 + cov.sn2)
    c.update(truth=tr, yard=tuple(float(e) for e in errors(c["fp64"], tr)), floor=tuple(float(truth.U4 * s) for s in scale))
    return c


def errors(got, tr):
    """the largest absolute error of LL, the gradient, the means, the variances (differences in longdouble)"""
    return tuple(np.max(np.abs(np.asarray(a).astype(truth.LD) - b)) for a, b in zip(got, tr))


def model(c, m):
    g = gp.NeighborGP(len(c["y"]), m, c["X"].shape[1], kernel=c["kernel"], ard=c["ard"])
    g.set_data(c["X"], c["y"])
    g.set_neighbors(c["idx"])
    g.set_loghyper(c["hp"])
    return g


@pytest.mark.parametrize("family,n,m,d,exact", CASES)
def test_fp64_restatement_is_finite_and_positive_definite(family, n, m, d, exact):
    fp = inputs(family, n, m, d, exact)["fp64"]
    assert all(np.all(np.isfinite(np.asarray(v, dtype=np.float64))) for v in fp) and np.all(fp[3] > 0)


@pytest.mark.gpu
@pytest.mark.parametrize("family,n,m,d,exact", CASES)
def test_accuracy(family, n, m, d, exact):
    """LL, g, mean and var within F_NN max(yardstick, 4 ulp |truth|); exact: of the exact GP of all rows."""
    c = case(family, n, m, d, exact)
    g = model(c, m)
    ll, gr = g.loglik_grad()
    mean, var = g.predict(c["Xt"], c["idx_t"])
    g.close()
    err = errors((ll, gr, mean, var), c["truth"])
    ratios = [float(e) / max(yd, fl) for e, yd, fl in zip(err, c["yard"], c["floor"])]
    print("nn ratios %s n%d m%d d%d exact%d: ll %.3g g %.3g mean %.3g var %.3g" % ((family, n, m, d, exact) + tuple(ratios)))
    assert max(ratios) <= F_NN, ratios


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["se", "rq_ard", "rq"])
@pytest.mark.parametrize("m", [15, 31, 63])
def test_bits(family, m):
    """Two calls give equal bits; loglik's value has loglik_grad's; a row's prediction does not depend on the other rows."""
    c = case(family, 261, 16, 3, False) if family == "rq" else case(family, 261, m, [1, 17, 3][m // 31], False)
    m = 16 if family == "rq" else m
    g = model(c, m)
    a, b = g.loglik_grad(), g.loglik_grad()
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and g.loglik() == a[0]
    p5 = g.predict(c["Xt"], c["idx_t"])
    for t in (0, NT - 1):
        p1 = g.predict(c["Xt"][t:t + 1], c["idx_t"][t:t + 1])
        assert p1[0][0] == p5[0][t] and p1[1][0] == p5[1][t]
    lat = g.predict(c["Xt"], c["idx_t"], with_noise=False)
    assert np.array_equal(lat[0], p5[0]) and np.all(lat[1] < p5[1])
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("m", [15, 63])
def test_failure_gives_nan_and_the_handle_recovers(m):
    """A duplicated training point with sn2 = exp(-800) (= 0) and a NaN label each give NaN with CUGP_OK; the next healthy
    theta or data gives a fresh handle's bits."""
    c = case("se", 261, m, [1, 17, 3][m // 31], False)
    fresh = model(c, m)
    want = fresh.loglik_grad()
    wantp = fresh.predict(c["Xt"], c["idx_t"])
    fresh.close()
    g = model(c, m)
    X, y = c["X"].copy(), c["y"].copy()
    X[c["idx"][200, 0]] = X[200]                                       # row 200 and its nearest neighbour are one point
    g.set_data(X, c["y"])
    g.set_loghyper(c["hp"][:-1] + [-800.0])
    ll, gr = g.loglik_grad()
    assert np.isnan(ll) and np.all(np.isnan(gr)) and np.isnan(g.loglik())
    y[17] = np.nan
    g.set_data(c["X"], y)
    g.set_loghyper(c["hp"])
    ll, gr = g.loglik_grad()
    assert np.isnan(ll) and np.all(np.isnan(gr))
    g.set_data(c["X"], c["y"])
    got = g.loglik_grad()
    gotp = g.predict(c["Xt"], c["idx_t"])
    g.close()
    assert got[0] == want[0] and np.array_equal(got[1], want[1])
    assert np.array_equal(gotp[0], wantp[0]) and np.array_equal(gotp[1], wantp[1])


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["se", "rq_ard"])
def test_cg_solve_descends(family):
    c = case(family, 261, 16, 3, False)
    g = model(c, 16)
    f0 = -g.loglik()
    tr = g.cg_solve(10)
    end = -g.loglik()
    g.close()
    f = tr[:, -1]
    assert len(f) >= 2 and f[0] == f0 and np.all(np.diff(f) <= 0) and f[-1] < f[0] and end == f[-1]
