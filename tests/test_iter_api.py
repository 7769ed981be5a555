"""The matrix-free exact GP's interface without a GPU: the cugp_iter_* calls are declared, exported and bound; every refusal
comes back as CUGP_ERR_INVALID with the call's name before a device is looked for; and cugp_iter_apply_plan, replayed on
the CPU, covers every column exactly once in ascending ranges."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cugp_amd.gp as gp
from conftest import ROOT
from cugp_amd import capi

_dp, _ip, _vp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_void_p
SOLVER = [C.c_double, C.c_int, C.c_int]
CALLS = {
    "cugp_iter_create": [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_vp)],
    "cugp_iter_destroy": [_vp],
    "cugp_iter_num_hyper": [_vp, _ip],
    "cugp_iter_set_data": [_vp, _dp, _dp],
    "cugp_iter_set_loghyper": [_vp, _dp, C.c_int],
    "cugp_iter_set_split": [_vp, C.c_int],
    "cugp_iter_apply": [_vp, _dp, C.c_int, _dp],
    "cugp_iter_apply_cross": [_vp, _dp, C.c_int, _dp, C.c_int, _dp],
    "cugp_iter_solve": [_vp, _dp, C.c_int] + SOLVER + [_dp, _dp],
    "cugp_iter_fit": [_vp] + SOLVER + [_dp],
    "cugp_iter_get_alpha": [_vp, _dp],
    "cugp_iter_predict": [_vp, _dp, C.c_int, _dp, _dp] + SOLVER + [_dp],
    "cugp_iter_apply_plan": [C.c_int, C.c_int, C.c_int, _ip],
    "cugp_iter_apply_plan_split": [C.c_int, C.c_int, C.c_int, C.c_int, _ip],
}
INV = capi.CUGP_ERR_INVALID
JT, ROWS, SLOTS = 32, 64, 512          # kernels.h: ITER_JT, ITER_ROWS, ITER_SLOTS


@pytest.mark.parametrize("name", sorted(CALLS))
def test_declared_exported_and_bound(name):
    with open(os.path.join(ROOT, "include", "cugp.h")) as f:
        assert re.search(r"\bint\s+%s\s*\(" % name, re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S))
    assert capi.SIGNATURES[name] == (C.c_int, CALLS[name])
    fn = getattr(capi.lib(), name)
    assert fn.restype is C.c_int and list(fn.argtypes) == CALLS[name]


def refused(rc, call):
    return rc == INV and call.encode() in capi.lib().cugp_last_error()


def test_refusals_come_before_the_device():
    """On a machine without a GPU a call that looked for one first would answer CUGP_ERR_NODEVICE."""
    L = capi.lib()
    h, buf, ibuf = _vp(), np.zeros(8), (C.c_int * 4)()
    p = capi.ptr(buf)
    for args in ((0, 2, 0, 0, 0), (5, 0, 0, 0, 0), (5, 2, -1, 0, 0), (5, 2, 0, 4, 0), (5, 2, 0, -1, 0), (5, 2, 0, 0, 2),
                 (capi.CUGP_ITER_MAX_N + 1, 2, 0, 0, 0)):
        assert refused(L.cugp_iter_create(*args, C.byref(h)), "cugp_iter_create") and not h.value, args
    assert refused(L.cugp_iter_create(5, 2, 0, 0, 0, None), "cugp_iter_create")
    assert L.cugp_iter_destroy(None) == capi.CUGP_OK
    null = _vp()
    assert refused(L.cugp_iter_num_hyper(null, ibuf), "cugp_iter_num_hyper")
    assert refused(L.cugp_iter_set_data(null, p, p), "cugp_iter_set_data")
    assert refused(L.cugp_iter_set_loghyper(null, p, 3), "cugp_iter_set_loghyper")
    assert refused(L.cugp_iter_set_split(null, 1), "cugp_iter_set_split")
    assert refused(L.cugp_iter_apply(null, p, 1, p), "cugp_iter_apply")
    assert refused(L.cugp_iter_apply_cross(null, p, 1, p, 1, p), "cugp_iter_apply_cross")
    assert refused(L.cugp_iter_solve(null, p, 1, 1e-8, 10, 1, p, None), "cugp_iter_solve")
    assert refused(L.cugp_iter_fit(null, 1e-8, 10, 1, None), "cugp_iter_fit")
    assert refused(L.cugp_iter_get_alpha(null, p), "cugp_iter_get_alpha")
    assert refused(L.cugp_iter_predict(null, p, 1, p, p, 1e-8, 10, 1, None), "cugp_iter_predict")
    for args in ((0, 5, 1), (5, 0, 1), (5, 5, 0)):
        assert refused(L.cugp_iter_apply_plan(*args, ibuf), "cugp_iter_apply_plan"), args
    assert refused(L.cugp_iter_apply_plan(5, 5, 1, None), "cugp_iter_apply_plan")
    assert refused(L.cugp_iter_apply_plan_split(5, 5, 1, -1, ibuf), "cugp_iter_apply_plan_split")
    assert refused(L.cugp_iter_apply_plan_split(5, 5, 1, 65536, ibuf), "cugp_iter_apply_plan_split")
    with pytest.raises(ValueError):
        gp.IterativeGP(5, 2, kernel="cubic")
    cnt = C.c_int()
    if not (L.cugp_device_count(C.byref(cnt)) == capi.CUGP_OK and cnt.value > 0):
        assert L.cugp_iter_create(5, 2, 0, capi.CUGP_KERNEL_RQ, 1, C.byref(h)) == capi.CUGP_ERR_NODEVICE and not h.value


@pytest.mark.parametrize("na", [1, 64, 65, 1000, 32767, 32768, 100000])
@pytest.mark.parametrize("nb", [1, 31, 32, 33, 257, 8192, 100000])
@pytest.mark.parametrize("force", [0, 1, 2, 3, 7, 65535])
def test_plan_replay(na, nb, force):
    """Every j in exactly one range, ranges ascending and none empty; S = 1 where the row blocks alone fill the device; a
    forced S is taken up to one range per stage; t does not enter (a column's bits cannot depend on its neighbours)."""
    plans = [gp.IterativeGP.plan(na, nb, t, force) for t in (1, 17, 64, 200)]
    p = plans[0]
    assert all(q == p for q in plans)
    assert p["stages"] == -(-nb // JT) and p["row_blocks"] == -(-na // ROWS) and 1 <= p["split"] <= p["stages"]
    seen = np.zeros(nb, dtype=int)
    for s in range(p["split"]):
        lo, hi = s * p["per"] * JT, min((s + 1) * p["per"] * JT, nb)
        assert lo < hi
        seen[lo:hi] += 1
    assert np.all(seen == 1)
    if force == 0 and p["row_blocks"] >= SLOTS:
        assert p["split"] == 1
    if force == 0 and p["split"] > 1:
        assert p["per"] >= 8 and p["row_blocks"] * (p["split"] - 1) < SLOTS
    if force:
        assert p["split"] == -(-p["stages"] // -(-p["stages"] // min(force, p["stages"])))
    if force == 0:
        out = (C.c_int * 4)()
        assert capi.lib().cugp_iter_apply_plan(na, nb, 5, out) == p["split"] and list(out) == list(p.values())
