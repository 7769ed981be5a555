"""The mixed mode's interface without a GPU: the three calls are declared, documented, exported and bound; the refusals that
need no handle come before any device (cugp_iter_apply32 without data or theta needs a handle: test_gpu_iter_mixed.py);
IterativeGP's own argument checks; and the numpy.float32 restatement of k_cov_apply32's arithmetic stays within F_MIX of
the longdouble truth on the GPU test's cases -- the figure F_MIX was set from."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cugp_amd.gp as gp
import mixed_ref as mr
from conftest import ROOT
from cugp_amd import capi

_dp, _ip, _vp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_void_p
CALLS = {
    "cugp_iter_set_precision": [_vp, C.c_int, C.c_double],
    "cugp_iter_apply32": [_vp, _dp, C.c_int, _dp],
    "cugp_iter_solve_stats": [_vp, _ip],
}


@pytest.mark.parametrize("name", sorted(CALLS))
def test_declared_documented_exported_and_bound(name):
    with open(os.path.join(ROOT, "include", "cugp.h")) as f:
        text = f.read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(" % name, code) and any(name[5:] in c or name in c for c in re.findall(r"/\*.*?\*/", text, re.S))
    assert re.search(r"#define\s+CUGP_ITER_FP64\s+0\b", code) and re.search(r"#define\s+CUGP_ITER_MIXED\s+1\b", code)
    assert capi.SIGNATURES[name] == (C.c_int, CALLS[name]) and (capi.CUGP_ITER_FP64, capi.CUGP_ITER_MIXED) == (0, 1)
    fn = getattr(capi.lib(), name)
    assert fn.restype is C.c_int and list(fn.argtypes) == CALLS[name]


def test_refusals_come_before_the_device():
    L = capi.lib()
    buf, ibuf, null = np.zeros(8), (C.c_int * 4)(), _vp()
    p = capi.ptr(buf)

    def refused(rc, call, word=""):
        return rc == capi.CUGP_ERR_INVALID and call.encode() in L.cugp_last_error() and word.encode() in L.cugp_last_error()
    for mode in (-1, 2):
        assert refused(L.cugp_iter_set_precision(null, mode, 0.0), "cugp_iter_set_precision", "mode")
    for drop in (-0.5, 1.0, 2.0, float("nan"), float("inf")):
        assert refused(L.cugp_iter_set_precision(null, 1, drop), "cugp_iter_set_precision", "cycle_drop"), drop
    assert refused(L.cugp_iter_set_precision(null, 1, 0.5), "cugp_iter_set_precision", "null")
    assert refused(L.cugp_iter_apply32(null, p, 1, p), "cugp_iter_apply32")
    assert refused(L.cugp_iter_solve_stats(null, ibuf), "cugp_iter_solve_stats")


def test_plumbing_through_gp(monkeypatch):
    """IterativeGP hands the mode, the default cycle_drop (0) and the fp32 product's call on, and refuses other strings."""
    seen = []
    monkeypatch.setattr(capi, "lib", lambda: type("L", (), {"__getattr__": lambda s, n: lambda *a: seen.append((n,) + a[1:]) or 0})())
    g = gp.IterativeGP.__new__(gp.IterativeGP)
    g.n, g.d, g._h = 4, 1, _vp()
    g.set_precision("mixed"), g.set_precision("fp64", cycle_drop=0.25)
    assert seen == [("cugp_iter_set_precision", 1, 0.0), ("cugp_iter_set_precision", 0, 0.25)]
    g.apply(np.ones((2, 4)), precision="fp32"), g.apply(np.ones((2, 4))), g.solve_stats()
    assert [s[0] for s in seen[2:]] == ["cugp_iter_apply32", "cugp_iter_apply", "cugp_iter_solve_stats"] and seen[2][2] == 2
    for call in (lambda: g.set_precision("fp32"), lambda: g.apply(np.ones((1, 4)), precision="mixed")):
        with pytest.raises(ValueError):
            call()


@pytest.mark.parametrize("family,n,d,t,split", mr.PRODUCT)
def test_restatement_within_f_mix(family, n, d, t, split):
    X, _, hp, K, M = mr.case(family, n, d)
    V = mr.vectors(t, n)
    ratio = float(np.max(np.abs(mr.restate32(family, X, hp, V) - V.astype(mr.LD) @ K.T) / mr.yardstick(M, V)))
    print("ratio %.3g" % ratio)
    assert ratio <= mr.F_MIX / 2                       # (F_MIX: twice the next power of two above the largest ratio)
