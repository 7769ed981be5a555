"""The preconditioner's interface without a GPU: the cugp_iter_*precond* calls are declared, exported and bound, every
refusal comes back as CUGP_ERR_INVALID with the call's name before a device is looked for, and cugp_iter_precond_plan's
row ranges cover [0, n) exactly once."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cugp_amd.gp as gp
from conftest import ROOT
from cugp_amd import capi

_dp, _ip, _vp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_void_p
CALLS = {
    "cugp_iter_set_precond": [_vp, C.c_int],
    "cugp_iter_precond_info": [_vp, _ip],
    "cugp_iter_get_precond": [_vp, _dp, _ip],
    "cugp_iter_precond_apply": [_vp, _dp, C.c_int, _dp],
    "cugp_iter_precond_plan": [C.c_int, C.c_int, _ip],
}


@pytest.mark.parametrize("name", sorted(CALLS))
def test_declared_exported_and_bound(name):
    with open(os.path.join(ROOT, "include", "cugp.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(" % name, text) and re.search(r"#define\s+CUGP_ITER_MAX_RANK\s+512\b", text)
    assert capi.SIGNATURES[name] == (C.c_int, CALLS[name]) and capi.CUGP_ITER_MAX_RANK == 512
    fn = getattr(capi.lib(), name)
    assert fn.restype is C.c_int and list(fn.argtypes) == CALLS[name]


def test_refusals_come_before_the_device():
    L = capi.lib()
    buf, ibuf, null = np.zeros(8), (C.c_int * 4)(), _vp()
    p = capi.ptr(buf)

    def refused(rc, call):
        return rc == capi.CUGP_ERR_INVALID and call.encode() in L.cugp_last_error()
    assert refused(L.cugp_iter_set_precond(null, 1), "cugp_iter_set_precond")
    assert refused(L.cugp_iter_precond_info(null, ibuf), "cugp_iter_precond_info")
    assert refused(L.cugp_iter_get_precond(null, p, ibuf), "cugp_iter_get_precond")
    assert refused(L.cugp_iter_precond_apply(null, p, 1, p), "cugp_iter_precond_apply")
    for n, rank in ((0, 0), (capi.CUGP_ITER_MAX_N + 1, 1), (5, -1), (5, 6), (1000, 513)):
        assert refused(L.cugp_iter_precond_plan(n, rank, ibuf), "cugp_iter_precond_plan"), (n, rank)
    assert refused(L.cugp_iter_precond_plan(5, 1, None), "cugp_iter_precond_plan")


@pytest.mark.parametrize("n,rank", [(n, r) for n in (1, 511, 512, 513, 10 ** 5, 10 ** 6) for r in (0, 1, 64, 65, 512) if r <= n])
def test_plan_replay(n, rank):
    """Every row in exactly one range, ranges ascending and none empty; the rank pads to 64 and does not move the ranges."""
    p = gp.IterativeGP.precond_plan(n, rank)
    assert p["rp"] == -(-rank // 64) * 64 and p["per"] % 16 == 0 and p["steps"] * 4 == p["per"] and 1 <= p["blocks"] <= 512
    assert (p["per"], p["blocks"]) == tuple(gp.IterativeGP.precond_plan(n, 0)[k] for k in ("per", "blocks"))
    seen = np.zeros(n, dtype=int)
    for b in range(p["blocks"]):
        lo, hi = b * p["per"], min((b + 1) * p["per"], n)
        assert lo < hi
        seen[lo:hi] += 1
    assert np.all(seen == 1)
