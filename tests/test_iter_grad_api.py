"""The matrix-free gradient's interface without a GPU: cugp_iter_grad_forms and cugp_iter_loglik_grad are declared with their
estimator stated, exported and bound; every refusal comes back as CUGP_ERR_INVALID with the call's name before the handle is
read or a device looked for; the Rademacher probes are a function of the generator."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cugp_amd.gp as gp
from conftest import ROOT
from cugp_amd import capi

_dp, _vp = C.POINTER(C.c_double), C.c_void_p
CALLS = {
    "cugp_iter_grad_forms": [_vp, _dp, _dp, C.c_int, _dp],
    "cugp_iter_loglik_grad": [_vp, _dp, C.c_int, C.c_double, C.c_int, C.c_int, _dp, _dp, _dp],
}


@pytest.mark.parametrize("name", sorted(CALLS))
def test_declared_exported_and_bound(name):
    with open(os.path.join(ROOT, "include", "cugp.h")) as f:
        text = f.read()
    assert re.search(r"\bint\s+%s\s*\(" % name, re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    doc = " ".join(text.split())
    for words in ("Hutchinson", "deterministic function of (X, y, theta, Z", "g_h = 1/2 [ (1/t) sum_p u_p' (dK/dtheta_h) z_p"):
        assert words in doc, words
    assert capi.SIGNATURES[name] == (C.c_int, CALLS[name])
    fn = getattr(capi.lib(), name)
    assert fn.restype is C.c_int and list(fn.argtypes) == CALLS[name]


def test_refusals_come_before_the_device():
    """The handle is a zeroed block: it is not read before the arguments beside it have passed, and reads as 'no data set'."""
    L = capi.lib()
    buf, h, null = np.zeros(8), C.cast(C.create_string_buffer(1 << 14), _vp), _vp()
    p = capi.ptr(buf)

    def refused(rc, call):
        return rc == capi.CUGP_ERR_INVALID and call.encode() in L.cugp_last_error()
    for args in ((null, p, p, 1, p), (h, None, p, 1, p), (h, p, None, 1, p), (h, p, p, 1, None), (h, p, p, 0, p), (h, p, p, 1, p)):
        assert refused(L.cugp_iter_grad_forms(*args), "cugp_iter_grad_forms"), args
    ok = (1e-8, 10, 5)
    for args in ((null, p, 1) + ok + (p, p, p), (h, None, 1) + ok + (p, p, p), (h, p, 1) + ok + (None, p, p),
                 (h, p, 0) + ok + (p, p, p), (h, p, 1, 0.0, 10, 5, p, p, p), (h, p, 1, float("nan"), 10, 5, p, p, p),
                 (h, p, 1, float("inf"), 10, 5, p, p, p), (h, p, 1, 1e-8, 0, 5, p, p, p), (h, p, 1, 1e-8, 10, 0, p, p, p),
                 (h, p, 1) + ok + (p, None, None)):
        assert refused(L.cugp_iter_loglik_grad(*args), "cugp_iter_loglik_grad"), args


def test_rademacher_probes_follow_the_generator():
    a, b = gp.rademacher(np.random.default_rng(11), 7, 33), gp.rademacher(np.random.default_rng(11), 7, 33)
    assert a.shape == (7, 33) and a.dtype == np.float64 and np.array_equal(a, b) and np.all(np.abs(a) == 1.0)
    assert not np.array_equal(a, gp.rademacher(np.random.default_rng(12), 7, 33)) and abs(a.mean()) < 0.5
    with pytest.raises(ValueError):
        gp.rademacher(np.random.default_rng(11), 0, 33)
