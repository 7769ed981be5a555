"""The variance cache's interface without a GPU: the four cugp_iter_varcache_* / cugp_iter_predict_cached calls are declared with
the bound, the ending rule and the refusals stated, exported and bound; every refusal comes back as CUGP_ERR_INVALID with the
call's name before the handle is read or a device looked for; predict(var="cached") without a cache raises."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from cugp_amd import capi, gp

_dp, _ip, _vp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_void_p
CALLS = {
    "cugp_iter_varcache_build": [_vp, _dp, C.c_int, C.c_int, _ip],
    "cugp_iter_varcache_info": [_vp, _ip],
    "cugp_iter_varcache_get": [_vp, _dp, _dp, _dp],
    "cugp_iter_predict_cached": [_vp, _dp, C.c_int, C.c_int, _dp, _dp],
}


@pytest.mark.parametrize("name", sorted(CALLS))
def test_declared_exported_and_bound(name):
    with open(os.path.join(ROOT, "include", "cugp.h")) as f:
        text = f.read()
    assert re.search(r"\bint\s+%s\s*\(" % name, re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    doc = " ".join(text.split())
    for words in ("var_k(x*) = sf2 + sn2 - |R' k*|^2", "never below the exact variance", "the device decides where the basis ends",
                  name + " :"):
        assert words in doc, words
    assert capi.SIGNATURES[name] == (C.c_int, CALLS[name])
    fn = getattr(capi.lib(), name)
    assert fn.restype is C.c_int and list(fn.argtypes) == CALLS[name]


def test_refusals_come_before_the_device():
    """The handle is a zeroed block (n = 0, no cache): it is not read before the arguments beside it have passed."""
    L = capi.lib()
    buf, h, null = np.zeros(8), C.cast(C.create_string_buffer(1 << 14), _vp), _vp()
    p, ip = capi.ptr(buf), (C.c_int * 4)()
    refusals = {
        "cugp_iter_varcache_build": [(null, p, 1, 1, ip), (h, None, 1, 1, ip), (h, p, 1, 1, None), (h, p, 0, 1, ip), (h, p, 17, 1, ip),
                                     (h, p, 1, 0, ip), (h, p, 1, 513, ip), (h, p, 1, 1, ip)],         # the last: rank above n = 0
        "cugp_iter_varcache_info": [(null, ip), (h, None)],
        "cugp_iter_varcache_get": [(null, p, p, p), (h, p, p, p), (h, None, None, None)],             # no cache
        "cugp_iter_predict_cached": [(null, p, 1, 1, p, p), (h, None, 1, 1, p, p), (h, p, 1, 1, p, None), (h, p, 0, 1, None, p),
                                     (h, p, 2147482624, 1, None, p), (h, p, 1, 1, None, p)],           # the last: no cache
    }
    for call, cases in refusals.items():
        for args in cases:
            assert getattr(L, call)(*args) == capi.CUGP_ERR_INVALID and call.encode() in L.cugp_last_error(), (call, args)
    assert L.cugp_iter_varcache_info(h, ip) == 0 and list(ip) == [0, 0, 0, 0]


def test_predict_cached_without_a_cache_raises():
    g = gp.IterativeGP.__new__(gp.IterativeGP)                 # no device: the zeroed block again, behind the Python layer
    g.n, g.d, g._keep = 4, 2, C.create_string_buffer(1 << 14)
    g._h = C.cast(g._keep, _vp)
    try:
        with pytest.raises(capi.CugpError) as e:
            g.predict(np.zeros((3, 2)), var="cached")
        assert e.value.code == capi.CUGP_ERR_INVALID and "cugp_iter_predict_cached" in str(e.value)
        with pytest.raises(ValueError):
            g.predict(np.zeros((3, 2)), var="exact")
        with pytest.raises(ValueError):
            g.variance_cache(2)                                # the default start block needs rng
    finally:
        g._h = _vp()                                           # nothing for close() to destroy
