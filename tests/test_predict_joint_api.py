"""Joint predictive covariance and posterior draws (cugp_predict_cov, cugp_predict_sample) without a GPU: both symbols
are exported and bound with their argument counts, and every argument error comes back as CUGP_ERR_INVALID before any
device call (a null or a dummy handle is never dereferenced)."""
import ctypes as C
import math

import numpy as np
import pytest

from cugp_amd import capi


@pytest.mark.parametrize("name, nargs", [("cugp_predict_cov", 6), ("cugp_predict_sample", 8)])
def test_exported_and_bound(name, nargs):
    assert name in capi.SIGNATURES
    assert len(capi.SIGNATURES[name][1]) == nargs
    fn = getattr(capi.lib(), name)
    assert fn.restype is C.c_int and len(fn.argtypes) == nargs


def _p(a):
    return capi.ptr(a) if a is not None else None


DUMMY = C.c_void_p(0x1000)     # never dereferenced: the checks come first


@pytest.mark.parametrize("handle", [None, DUMMY], ids=["null", "dummy"])
def test_predict_cov_argument_errors(handle):
    L = capi.lib()
    Xt, m, cov = np.zeros((4, 3)), np.empty(4), np.empty((4, 4))
    cases = [(None, Xt, 4, cov),                    # null handle
             (handle, None, 4, cov),                # null Xt
             (handle, Xt, 4, None),                 # null cov
             (handle, Xt, 0, cov),                  # nt <= 0
             (handle, Xt, -2, cov)]
    for h, x, nt, c in cases:
        for noise in (0, 1):
            assert L.cugp_predict_cov(h, _p(x), nt, noise, _p(m), _p(c)) == capi.CUGP_ERR_INVALID, (x is None, nt)
    assert b"cugp_predict_cov" in L.cugp_last_error()


@pytest.mark.parametrize("handle", [None, DUMMY], ids=["null", "dummy"])
def test_predict_sample_argument_errors(handle):
    L = capi.lib()
    Xt, Z, out = np.zeros((4, 3)), np.zeros((2, 4)), np.empty((2, 4))
    ok = dict(h=handle, x=Xt, nt=4, jit=0.0, ns=2, z=Z, o=out)
    bad = [dict(h=None), dict(x=None), dict(z=None), dict(o=None), dict(nt=0), dict(nt=-1), dict(ns=0), dict(ns=-5),
           dict(jit=-1e-12), dict(jit=-1.0), dict(jit=math.nan), dict(jit=math.inf), dict(jit=-math.inf)]
    for b in bad:
        a = dict(ok, **b)
        for noise in (0, 1):
            rc = L.cugp_predict_sample(a["h"], _p(a["x"]), a["nt"], noise, a["jit"], a["ns"], _p(a["z"]), _p(a["o"]))
            assert rc == capi.CUGP_ERR_INVALID, b
    assert b"cugp_predict_sample" in L.cugp_last_error()


def test_python_methods_exist():
    import cugp_amd.gp as gp
    assert callable(gp.Covsum.compute_test_joint) and callable(gp.Covsum.sample_posterior)
