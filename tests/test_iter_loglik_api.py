"""The Lanczos-quadrature interface without a GPU: cugp_iter_loglik and cugp_iter_precond_sample are declared with the estimator,
the truncation rule and the refusals stated, exported and bound; every refusal comes back as CUGP_ERR_INVALID with the call's
name before the handle is read or a device looked for."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from cugp_amd import capi

_dp, _vp = C.POINTER(C.c_double), C.c_void_p
CALLS = {
    "cugp_iter_loglik": [_vp, _dp, _dp, C.c_int, C.c_double, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp],
    "cugp_iter_precond_sample": [_vp, _dp, _dp, C.c_int, _dp],
}


@pytest.mark.parametrize("name", sorted(CALLS))
def test_declared_exported_and_bound(name):
    with open(os.path.join(ROOT, "include", "cugp.h")) as f:
        text = f.read()
    assert re.search(r"\bint\s+%s\s*\(" % name, re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    doc = " ".join(text.split())
    for words in ("logdet = log|M| + (1/t) sum_p quad_p", "Truncation rule", "cugp_iter_loglik in the mixed mode",
                  "out [t][n] = L G1 + sn G2"):
        assert words in doc, words
    assert capi.SIGNATURES[name] == (C.c_int, CALLS[name])
    fn = getattr(capi.lib(), name)
    assert fn.restype is C.c_int and list(fn.argtypes) == CALLS[name]


def test_refusals_come_before_the_device():
    """The handle is a zeroed block: it is not read before the arguments beside it have passed, and reads as 'no data set'
    (cugp_iter_precond_sample: as 'no preconditioner asked for')."""
    L = capi.lib()
    buf, h, null = np.zeros(8), C.cast(C.create_string_buffer(1 << 14), _vp), _vp()
    p = capi.ptr(buf)

    def refused(rc, call):
        return rc == capi.CUGP_ERR_INVALID and call.encode() in L.cugp_last_error()
    ok, outs = (1e-8, 10, 5), (p, p, p, p, p, p)
    for args in ((null, p, p, 1) + ok + outs, (h, None, p, 1) + ok + outs, (h, p, p, 1) + ok + (None, p, p, p, p, p),
                 (h, p, p, 0) + ok + outs, (h, p, p, 1, 0.0, 10, 5) + outs, (h, p, p, 1, float("nan"), 10, 5) + outs,
                 (h, p, p, 1, 1e-8, 0, 5) + outs, (h, p, p, 1, 1e-8, 10, 0) + outs, (h, p, p, 1, 1e-8, 16385, 5) + outs,
                 (h, p, None, 1) + ok + (p, None, None, None, None, None)):
        assert refused(L.cugp_iter_loglik(*args), "cugp_iter_loglik"), args
    for args in ((null, p, p, 1, p), (h, None, p, 1, p), (h, p, None, 1, p), (h, p, p, 1, None), (h, p, p, 0, p), (h, p, p, 1, p)):
        assert refused(L.cugp_iter_precond_sample(*args), "cugp_iter_precond_sample"), args
