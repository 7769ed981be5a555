"""The test-input gradients' interface without a GPU: the two calls are declared, documented, exported and bound with their
exact argument types; their refusals that need no handle come before any device; IterativeGP.input_grad / predict_grad hand
their arguments on, put None where a quantity was not asked for and check shapes on the host."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import cugp_amd.gp as gp
from conftest import ROOT
from cugp_amd import capi

_dp, _vp = C.POINTER(C.c_double), C.c_void_p
CALLS = {
    "cugp_iter_input_grad": [_vp, _dp, C.c_int, _dp, C.c_int, _dp],
    "cugp_iter_predict_grad": [_vp, _dp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, C.c_double, C.c_int, C.c_int, _dp],
}


@pytest.mark.parametrize("name", sorted(CALLS))
def test_declared_documented_exported_and_bound(name):
    with open(os.path.join(ROOT, "include", "cugp.h")) as f:
        text = f.read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(" % name, code) and any(name in c for c in re.findall(r"/\*.*?\*/", text, re.S))
    assert capi.SIGNATURES[name] == (C.c_int, CALLS[name])
    fn = getattr(capi.lib(), name)
    assert fn.restype is C.c_int and list(fn.argtypes) == CALLS[name]


def test_refusals_come_before_the_device():
    L = capi.lib()
    p, null = capi.ptr(np.zeros(8)), _vp()
    for rc in (L.cugp_iter_input_grad(null, p, 1, p, 1, p), L.cugp_iter_input_grad(null, None, 1, p, 1, p)):
        assert rc == capi.CUGP_ERR_INVALID and b"cugp_iter_input_grad" in L.cugp_last_error()
    assert L.cugp_iter_predict_grad(null, p, 1, 1, p, p, p, p, 1e-8, 10, 5, None) == capi.CUGP_ERR_INVALID
    assert b"cugp_iter_predict_grad" in L.cugp_last_error()


def test_plumbing_through_gp(monkeypatch):
    seen = []
    monkeypatch.setattr(capi, "lib", lambda: type("L", (), {"__getattr__": lambda s, n: lambda *a: seen.append((n,) + a[1:]) or 0})())
    g = gp.IterativeGP.__new__(gp.IterativeGP)
    g.n, g.d, g._h = 4, 2, _vp()
    assert list(inspect.signature(g.predict_grad).parameters) == ["Xt", "with_noise", "want_var", "want_var_grad", "tol", "max_iter",
                                                                  "check_every"]
    assert list(inspect.signature(g.input_grad).parameters) == ["Xt", "W"]
    Xt = np.ones((3, 2))
    assert g.input_grad(Xt, np.ones(4)).shape == (3, 2) and g.input_grad(Xt, np.ones((3, 4))).shape == (3, 2)
    assert [(s[0], s[2], s[4]) for s in seen] == [("cugp_iter_input_grad", 3, 1), ("cugp_iter_input_grad", 3, 3)]
    for W in (np.ones((2, 4)), np.ones((3, 5)), np.ones((0, 4))):
        with pytest.raises(ValueError):
            g.input_grad(Xt, W)
    del seen[:]
    m, v, dm, dv, info = g.predict_grad(Xt, with_noise=False, tol=1e-6, max_iter=7, check_every=3)
    assert (m.shape, v.shape, dm.shape, dv.shape, info.shape) == ((3,), (3,), (3, 2), (3, 2), (3, 4))
    assert seen[0][0] == "cugp_iter_predict_grad" and seen[0][2:4] == (3, 0) and seen[0][8:11] == (1e-6, 7, 3)
    m, v, dm, dv, info = g.predict_grad(Xt, want_var=False)
    assert v is None and dv.shape == (3, 2) and info.shape == (3, 4) and seen[1][5] is None and seen[1][3] == 1
    m, v, dm, dv, info = g.predict_grad(Xt, want_var=False, want_var_grad=False)
    assert v is None and dv is None and info is None and dm.shape == (3, 2) and seen[2][7] is None and seen[2][11] is None
