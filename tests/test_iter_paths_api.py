"""The pathwise draws' interface without a GPU: the three calls are declared, documented, exported and bound with their exact
argument types; their refusals that need no handle come before any device; IterativeGP.features_apply / sample_paths hand
their arguments on, draw only what the caller did not give and check shapes on the host; spectral_frequencies draws from the
families' spectral densities (E cos(omega . r) = k(r) / sf2 at unit length scale)."""
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
    "cugp_iter_features_apply": [_vp, _dp, C.c_int, _dp, _dp, C.c_int, _dp, C.c_int, _dp, _dp],
    "cugp_iter_paths_fit": [_vp, _dp, _dp, C.c_int, _dp, _dp, C.c_int, _dp, C.c_double, C.c_int, C.c_int, _dp, _dp],
    "cugp_iter_paths_eval": [_vp, _dp, C.c_int, _dp, _dp, C.c_int, _dp, _dp, C.c_int, _dp, _dp],
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
    for name, args in (("cugp_iter_features_apply", (null, p, 1, p, p, 1, p, 1, None, p)),
                       ("cugp_iter_paths_fit", (null, p, p, 1, p, None, 1, None, 1e-8, 10, 5, p, None)),
                       ("cugp_iter_paths_eval", (null, p, 1, p, p, 1, p, p, 1, None, p))):
        assert getattr(L, name)(*args) == capi.CUGP_ERR_INVALID and name.encode() in L.cugp_last_error()


def test_plumbing_through_gp(monkeypatch):
    seen = []
    monkeypatch.setattr(capi, "lib", lambda: type("L", (), {"__getattr__": lambda s, n: lambda *a: seen.append((n,) + a[1:]) or 0})())
    g = gp.IterativeGP.__new__(gp.IterativeGP)
    g.n, g.d, g.nh, g._h, g._kind, g._origin = 4, 2, 3, _vp(), capi.CUGP_KERNEL_SE, np.array([0.5, -0.5])
    assert list(inspect.signature(g.features_apply).parameters) == ["Xq", "Omega", "b", "W", "origin"]
    assert list(inspect.signature(g.sample_paths).parameters) == ["s", "features", "rng", "Omega", "b", "W", "Eps", "origin", "tol",
                                                                  "max_iter", "check_every"]
    Om, b, W = np.ones((5, 2)), np.ones(5), np.ones((3, 5))
    assert g.features_apply(None, Om, b, W).shape == (3, 4) and g.features_apply(np.ones((7, 2)), Om, b, W[0], [0, 1]).shape == (1, 7)
    assert [(s[0], s[1], s[2], s[5], s[7], s[8] is None) for s in seen] == [("cugp_iter_features_apply", None, 4, 5, 3, True),
                                                                           ("cugp_iter_features_apply", seen[1][1], 7, 5, 1, False)]
    for bad in ((np.ones((5, 3)), b, W), (Om, np.ones(4), W), (Om, b, np.ones((65, 5))), (Om, b, np.ones((3, 4))), (Om[:0], b[:0], W[:, :0])):
        with pytest.raises(ValueError):
            g.features_apply(None, *bad)
    del seen[:]
    with pytest.raises(ValueError):
        g.sample_paths(2, Omega=Om, b=b)                                   # W would have to be drawn: no rng
    paths = g.sample_paths(3, Omega=Om, b=b, W=W, tol=1e-6, max_iter=7, check_every=3)
    assert seen[0][0] == "cugp_iter_paths_fit" and seen[0][3] == 5 and seen[0][5] is None and seen[0][6] == 3 and seen[0][8:11] == (1e-6, 7, 3)
    assert paths.V.shape == (3, 4) and paths.info.shape == (3, 4) and np.array_equal(paths.origin, g._origin)
    assert paths(np.ones((6, 2))).shape == (3, 6) and seen[1][0] == "cugp_iter_paths_eval" and seen[1][2] == 6 and seen[1][8] == 3
    del seen[:]
    paths = g.sample_paths(70, features=9, rng=np.random.default_rng(0))    # everything drawn, the noise too; 64 + 6 paths
    assert [(s[0], s[3], s[6], s[5] is None) for s in seen] == [("cugp_iter_paths_fit", 9, 64, False), ("cugp_iter_paths_fit", 9, 6, False)]
    assert paths.Omega.shape == (9, 2) and paths.W.shape == (70, 9) and np.all((paths.b >= 0) & (paths.b < 2 * np.pi))
    assert paths(np.ones((6, 2))).shape == (70, 6) and [s[8] for s in seen[2:]] == [64, 6]


@pytest.mark.parametrize("kernel,alpha,k", [
    ("se", None, lambda r: np.exp(-r * r / 2)), ("matern32", None, lambda r: (1 + 3 ** .5 * r) * np.exp(-3 ** .5 * r)),
    ("matern52_ard", None, lambda r: (1 + 5 ** .5 * r + 5 * r * r / 3) * np.exp(-5 ** .5 * r)),
    ("rq", 0.8, lambda r: (1 + r * r / 1.6) ** -0.8)])
def test_spectral_frequencies_against_the_closed_forms(kernel, alpha, k):
    """|cos| <= 1: the mean of m = 2^16 of them lies within 6 / sqrt(m) of its expectation k(r) / sf2 at six standard errors."""
    m, r = 1 << 16, np.array([0.3, -0.7, 1.1])
    Om = gp.spectral_frequencies(kernel, 3, m, np.random.default_rng(0), alpha)
    err = abs(np.cos(Om @ r).mean() - k(np.sqrt(r @ r)))
    print(kernel, "error", err)
    assert Om.shape == (m, 3) and err <= 6 / np.sqrt(m)
    if alpha is not None:
        with pytest.raises(ValueError):
            gp.spectral_frequencies(kernel, 3, 4, np.random.default_rng(0))
