"""The sample paths' input gradients without a GPU: cugp_iter_paths_grad is declared, documented, exported and bound with its
exact argument types; its refusals that need no handle come before any device, each with its own message; SamplePaths.grad
hands its arguments on -- [s, nt, d], 64 paths a call, a NULL for the term that `part` leaves out."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cugp_amd.gp as gp
from conftest import ROOT
from cugp_amd import capi

_dp, _vp = C.POINTER(C.c_double), C.c_void_p
NAME = "cugp_iter_paths_grad"
ARGS = [_vp, _dp, C.c_int, _dp, _dp, C.c_int, _dp, _dp, C.c_int, _dp, _dp]


def test_declared_documented_exported_and_bound():
    with open(os.path.join(ROOT, "include", "cugp.h")) as f:
        text = f.read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(" % NAME, code) and any(NAME in c for c in re.findall(r"/\*.*?\*/", text, re.S))
    assert capi.SIGNATURES[NAME] == (C.c_int, ARGS)
    fn = getattr(capi.lib(), NAME)
    assert fn.restype is C.c_int and list(fn.argtypes) == ARGS


@pytest.mark.parametrize("w,v,s,nt,why", [(1, 1, 3, 2, b"null argument"), (0, 0, 3, 2, b"both NULL"), (1, 1, 0, 2, b"s must"),
                                          (1, 0, 65, 2, b"s must"), (0, 1, 3, 0, b"nt must")])
def test_refusals_come_before_the_device(w, v, s, nt, why):
    L, p = capi.lib(), capi.ptr(np.zeros(8))
    assert L.cugp_iter_paths_grad(_vp(), p, nt, p, p, 1, p if w else None, p if v else None, s, None, p) == capi.CUGP_ERR_INVALID
    assert NAME.encode() in L.cugp_last_error() and why in L.cugp_last_error()


def test_plumbing_through_gp(monkeypatch):
    seen = []
    monkeypatch.setattr(capi, "lib", lambda: type("L", (), {"__getattr__": lambda s, n: lambda *a: seen.append((n,) + a[1:]) or 0})())
    g = gp.IterativeGP.__new__(gp.IterativeGP)
    g.n, g.d, g._h = 4, 2, _vp()
    paths = gp.SamplePaths(g, np.ones((5, 2)), np.ones(5), np.ones((70, 5)), np.ones((70, 4)), None, None)
    for part, nulls in (("both", (False, False)), ("prior", (False, True)), ("update", (True, False))):
        del seen[:]
        assert paths.grad(np.ones((6, 2)), part).shape == (70, 6, 2)
        # (name, Xt, nt, Omega, b, m, W, V, s, origin, out): 64 + 6 paths
        assert [(c[0], c[2], c[5], c[8], c[9]) for c in seen] == [(NAME, 6, 5, 64, None), (NAME, 6, 5, 6, None)]
        assert all((c[6] is None, c[7] is None) == nulls for c in seen)
    with pytest.raises(ValueError):
        paths.grad(np.ones((6, 2)), "mean")
