"""The nearest-neighbour (Vecchia) GP's interface without a GPU: the cugp_nn_* calls are declared, exported and bound with
the header's signatures; every refusal comes back as CUGP_ERR_INVALID with the call's name before the handle is read or a
device looked for; gp.nn_neighbors against a plain double loop."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from cugp_amd import capi, gp

_dp, _ip, _vp, _i = C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_void_p, C.c_int
CALLS = {
    "cugp_nn_create": [_i, _i, _i, _i, _i, _i, C.POINTER(_vp)],
    "cugp_nn_destroy": [_vp],
    "cugp_nn_num_hyper": [_vp, _ip],
    "cugp_nn_check_neighbors": [_ip, _i, _i, _i, _i],
    "cugp_nn_set_data": [_vp, _dp, _dp],
    "cugp_nn_set_neighbors": [_vp, _ip],
    "cugp_nn_set_loghyper": [_vp, _dp, _i],
    "cugp_nn_loglik": [_vp, _dp],
    "cugp_nn_loglik_grad": [_vp, _dp, _dp, _i],
    "cugp_nn_predict": [_vp, _dp, _i, _ip, _i, _dp, _dp],
    "cugp_nn_cg_solve": [_vp, _i, _dp, _i, _ip],
}


@pytest.mark.parametrize("name", sorted(CALLS))
def test_declared_exported_and_bound(name):
    with open(os.path.join(ROOT, "include", "cugp.h")) as f:
        text = f.read()
    assert re.search(r"\bint\s+%s\s*\(" % name, re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    assert capi.SIGNATURES[name] == (_i, CALLS[name])
    fn = getattr(capi.lib(), name)
    assert fn.restype is _i and list(fn.argtypes) == CALLS[name]


def _ints(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, a.ctypes.data_as(_ip)


def test_refusals_come_before_the_device():
    """The handle is a zeroed block: it is not read before the arguments beside it have passed, and reads as 'no data set'."""
    L = capi.lib()
    buf, h, null, out = np.zeros(8), C.cast(C.create_string_buffer(1 << 12), _vp), _vp(), _vp()
    p, (_, ip) = capi.ptr(buf), _ints(np.zeros(8))
    calls = [("cugp_nn_create", a) for a in ((4, 64, 2, 0, 0, 0, C.byref(out)), (4, 0, 2, 0, 0, 0, C.byref(out)),
                                              (0, 3, 2, 0, 0, 0, C.byref(out)), (4, 3, 0, 0, 0, 0, C.byref(out)),
                                              (4, 3, 2, -1, 0, 0, C.byref(out)), (4, 3, 2, 0, 4, 0, C.byref(out)),
                                              (4, 3, 2, 0, 0, 2, C.byref(out)), (4, 3, 2, 0, 0, 0, None))]
    calls += [("cugp_nn_num_hyper", (null, ip)), ("cugp_nn_num_hyper", (h, None)),
              ("cugp_nn_set_data", (null, p, p)), ("cugp_nn_set_data", (h, None, p)), ("cugp_nn_set_data", (h, p, None)),
              ("cugp_nn_set_data", (h, p, p)), ("cugp_nn_set_neighbors", (null, ip)), ("cugp_nn_set_neighbors", (h, None)),
              ("cugp_nn_set_neighbors", (h, ip)), ("cugp_nn_set_loghyper", (null, p, 3)), ("cugp_nn_set_loghyper", (h, None, 3)),
              ("cugp_nn_set_loghyper", (h, p, 3)), ("cugp_nn_loglik", (null, p)), ("cugp_nn_loglik", (h, None)),
              ("cugp_nn_loglik", (h, p)), ("cugp_nn_loglik_grad", (null, p, p, 3)), ("cugp_nn_loglik_grad", (h, p, None, 3)),
              ("cugp_nn_loglik_grad", (h, p, p, 3)), ("cugp_nn_predict", (null, p, 1, ip, 1, p, p)),
              ("cugp_nn_predict", (h, None, 1, ip, 1, p, p)), ("cugp_nn_predict", (h, p, 1, None, 1, p, p)),
              ("cugp_nn_predict", (h, p, 0, ip, 1, p, p)), ("cugp_nn_predict", (h, p, 1, ip, 2, p, p)),
              ("cugp_nn_predict", (h, p, 1, ip, 1, None, p)), ("cugp_nn_predict", (h, p, 1, ip, 1, p, p)),
              ("cugp_nn_cg_solve", (null, 5, p, 1, ip)), ("cugp_nn_cg_solve", (h, 0, p, 1, ip)), ("cugp_nn_cg_solve", (h, 5, p, 1, ip))]
    for name, args in calls:
        assert getattr(L, name)(*args) == capi.CUGP_ERR_INVALID and name.encode() in L.cugp_last_error(), (name, args)


@pytest.mark.parametrize("rows,training,ok", [
    ([[-1, -1], [0, -1], [1, 0], [0, 2]], 1, True),
    ([[-1, -1], [1, -1], [1, 0], [0, 2]], 1, False),        # row 1 names itself: an index >= i
    ([[-1, -1], [0, -1], [1, 1], [0, 2]], 1, False),        # twice in a row
    ([[-1, -1], [0, -1], [1, -2], [0, 2]], 1, False),       # below -1
    ([[3, 0], [2, -1]], 0, True),                           # test rows: any training rows
    ([[4, 0], [2, -1]], 0, False),                          # beyond n = 4
    ([[3, 3], [2, -1]], 0, False),
])
def test_check_neighbors(rows, training, ok):
    L = capi.lib()
    a, ip = _ints(rows)
    rc = L.cugp_nn_check_neighbors(ip, len(a), 2, 4, training)
    assert rc == (capi.CUGP_OK if ok else capi.CUGP_ERR_INVALID)
    for bad in ((None, 2, 2, 4, 1), (ip, 0, 2, 4, 1), (ip, 2, 64, 4, 1), (ip, 2, 0, 4, 1), (ip, 2, 2, 0, 1), (ip, 2, 2, 4, 2)):
        assert L.cugp_nn_check_neighbors(*bad) == capi.CUGP_ERR_INVALID and b"cugp_nn_check_neighbors" in L.cugp_last_error()


@pytest.mark.parametrize("weights", [None, [1.0, 0.25]])
def test_nn_neighbors_against_a_double_loop(weights):
    """n = 40, m = 5, d = 2 on a small integer grid (many exact ties; rows 7 and 8 are one point): ties go to the smaller
    index, each row's neighbours come in order of distance, -1 behind them; with Xt the m nearest training rows."""
    rng = np.random.default_rng(5)
    X = rng.integers(0, 6, (40, 2)).astype(np.float64)
    X[8] = X[7]
    Xt = np.vstack([rng.integers(0, 6, (6, 2)).astype(np.float64), X[7:8]])
    w = np.ones(2) if weights is None else np.asarray(weights)

    def loop(Q, earlier):
        out = np.full((len(Q), 5), -1, dtype=np.int32)
        for i in range(len(Q)):
            cand = []
            for j in range(i if earlier else len(X)):
                cand.append((sum(((Q[i, c] - X[j, c]) * w[c]) ** 2 for c in range(2)), j))
            cand.sort()
            for s, (_, j) in enumerate(cand[:5]):
                out[i, s] = j
        return out
    got = gp.nn_neighbors(X, 5, weights=weights)
    assert got.dtype == np.int32 and np.array_equal(got, loop(X, True))
    assert np.array_equal(gp.nn_neighbors(X, 5, Xt, weights=weights), loop(Xt, False))
    a, ip = _ints(got)
    assert capi.lib().cugp_nn_check_neighbors(ip, 40, 5, 40, 1) == capi.CUGP_OK
