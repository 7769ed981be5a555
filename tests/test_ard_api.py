"""The ARD interface (one length scale per input dimension) without a GPU: the eight new entry points are exported and
bound with their argument counts, every argument error comes back as CUGP_ERR_INVALID before any device call (a null or
a dummy handle is never dereferenced), and the CG loop over nh entries is the 3-entry loop bit for bit."""
import ctypes as C

import numpy as np
import pytest

import cugp_amd.gp as gp
from conftest import HP_BCM
from cugp_amd import capi

NEW = [("cugp_create_ard", 4), ("cugp_num_hyper", 2), ("cugp_set_loghyper_ard", 3), ("cugp_get_loghyper_ard", 3),
       ("cugp_loglik_grad_ard", 4), ("cugp_loglik_grad_fetch_ard", 4), ("cugp_cg_minimize_n", 8),
       ("cugp_cg_solve_ard", 5)]


@pytest.mark.parametrize("name, nargs", NEW)
def test_exported_and_bound(name, nargs):
    assert name in capi.SIGNATURES
    assert len(capi.SIGNATURES[name][1]) == nargs
    fn = getattr(capi.lib(), name)
    assert fn.restype is C.c_int and len(fn.argtypes) == nargs


def test_python_methods_exist():
    import inspect
    assert "ard" in inspect.signature(gp.Covsum.__init__).parameters
    assert callable(gp.cg_minimize_n)
    for m in ("get_param_dim", "set_loghyperparam", "get_loghyperparam", "loglik_grad", "fetch",
              "compute_gradient_loghyperparam", "cg_solve"):
        assert callable(getattr(gp.Covsum, m))


DUMMY = C.c_void_p(0x1000)     # never dereferenced: the checks come first


@pytest.mark.parametrize("handle", [None, DUMMY], ids=["null", "dummy"])
def test_argument_errors(handle):
    L = capi.lib()
    v, ll, nh = np.zeros(5), C.c_double(), C.c_int()
    p = capi.ptr(v)
    INV = capi.CUGP_ERR_INVALID
    out = C.c_void_p()
    assert L.cugp_create_ard(0, 3, 0, C.byref(out)) == INV and L.cugp_create_ard(10, 0, 0, C.byref(out)) == INV
    assert L.cugp_create_ard(10, 3, 0, None) == INV
    assert L.cugp_num_hyper(None, C.byref(nh)) == INV and L.cugp_num_hyper(handle, None) == INV
    assert L.cugp_set_loghyper_ard(None, p, 5) == INV and L.cugp_set_loghyper_ard(handle, None, 5) == INV
    assert L.cugp_set_loghyper_ard(handle, p, 2) == INV and L.cugp_set_loghyper_ard(handle, p, -1) == INV
    assert b"cugp_set_loghyper_ard" in L.cugp_last_error()
    assert L.cugp_get_loghyper_ard(None, p, 5) == INV and L.cugp_get_loghyper_ard(handle, None, 5) == INV
    assert L.cugp_get_loghyper_ard(handle, p, 0) == INV
    assert L.cugp_loglik_grad_ard(None, C.byref(ll), p, 5) == INV
    assert L.cugp_loglik_grad_ard(handle, None, p, 5) == INV and L.cugp_loglik_grad_ard(handle, C.byref(ll), None, 5) == INV
    assert L.cugp_loglik_grad_ard(handle, C.byref(ll), p, 1) == INV
    assert b"cugp_loglik_grad_ard" in L.cugp_last_error()
    assert L.cugp_loglik_grad_fetch_ard(None, C.byref(ll), p, 5) == INV
    assert L.cugp_loglik_grad_fetch_ard(handle, C.byref(ll), p, 2) == INV
    assert L.cugp_cg_solve_ard(None, 10, None, 0, None) == INV
    cb = capi.OBJECTIVE_N(lambda *a: None)
    assert L.cugp_cg_minimize_n(cb, None, None, 5, 10, None, 0, None) == INV
    assert L.cugp_cg_minimize_n(cb, None, p, 0, 10, None, 0, None) == INV
    assert L.cugp_cg_minimize_n(cb, None, p, 5, -1, None, 0, None) == INV
    assert L.cugp_cg_minimize_n(C.cast(None, capi.OBJECTIVE_N), None, p, 5, 10, None, 0, None) == INV


def _oracle_objective(oracle, X, y):
    def fn(th):
        return -oracle.loglik(X, y, th), oracle.grad(X, y, th)
    return fn


def test_cg_minimize_n_is_cg_minimize_for_three(oracle, si128):
    """nh = 3: theta and the whole trace equal cugp_cg_minimize's bit for bit (and hence the oracle's)."""
    X, y = si128
    fn = _oracle_objective(oracle, X, y)
    th3, tr3 = gp.cg_minimize(fn, HP_BCM, 60)
    thn, trn = gp.cg_minimize_n(fn, HP_BCM, 60)
    assert trn.shape == tr3.shape and np.array_equal(trn, tr3) and np.array_equal(thn, th3)
    tho, tro = oracle.cg_minimize(fn, HP_BCM, 60)
    assert np.array_equal(trn, tro) and np.array_equal(thn, tho)


def test_cg_minimize_n_padding_invariance(oracle, si128):
    """An nh = 5 objective that is the 3-entry one in its first three entries and constant in the last two (gradient
    exactly 0.0 there) takes the 3-entry trajectory bit for bit in those entries and never moves the other two: adding
    exact zeros in index order changes no bit, so this pins the order of the sums."""
    X, y = si128
    fn = _oracle_objective(oracle, X, y)

    def fn5(th):
        f, g = fn(th[:3])
        return f, np.concatenate([g, [0.0, 0.0]])
    start = np.array(list(HP_BCM) + [0.7, -1.3])
    th3, tr3 = gp.cg_minimize(fn, HP_BCM, 60)
    th5, tr5 = gp.cg_minimize_n(fn5, start, 60)
    assert tr5.shape == (tr3.shape[0], 6)
    assert np.array_equal(tr5[:, :3], tr3[:, :3]) and np.array_equal(tr5[:, 5], tr3[:, 3])
    assert np.all(tr5[:, 3] == 0.7) and np.all(tr5[:, 4] == -1.3)
    assert np.array_equal(th5[:3], th3) and th5[3] == 0.7 and th5[4] == -1.3


def test_cg_minimize_n_nan_bisects():
    """nh = 6: a probe that returns NaN halves the step instead of aborting; the probe after the NaN one is the midpoint."""
    c = np.array([0.5, -1.0, 0.0, 2.0, -0.5, 1.5])
    k = np.array([1.0, 2.0, 0.5, 1.5, 0.75, 1.25])
    count = [0]

    def fn(th):
        count[0] += 1
        if count[0] == 2:
            return float("nan"), np.array([np.nan] + [0.0] * 5)
        return float(np.sum(k * (th - c) ** 2)), 2 * k * (th - c)
    start = np.array([-3.0, 2.0, 1.0, 0.0, 1.0, -1.0])
    th, tr = gp.cg_minimize_n(fn, start, 60)
    assert tr.shape[1] == 7
    assert np.isnan(tr[1, 6]) and np.isfinite(tr[2, 6])
    assert np.allclose(tr[2, :6] - start, 0.5 * (tr[1, :6] - start), rtol=1e-12, atol=1e-15)
    assert np.isfinite(tr[-1, 6]) and np.allclose(th, c, atol=1e-4)
