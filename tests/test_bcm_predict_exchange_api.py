"""cugp_bcm_predict_allgather (product-of-experts prediction across ranks, csrc/comm.cpp) without a GPU: the symbol is
exported and bound, and the argument errors every rank detects alike come back before any device or collective is
touched."""
import ctypes as C

import numpy as np

from cugp_amd import capi


def test_predict_allgather_exported_and_bound():
    assert "cugp_bcm_predict_allgather" in capi.SIGNATURES
    fn = capi.lib().cugp_bcm_predict_allgather
    assert fn.restype is C.c_int and len(fn.argtypes) == 8


def test_predict_allgather_argument_errors_without_a_device():
    L = capi.lib()
    Xt = np.zeros((4, 3))
    m, v = np.empty(4), np.empty(4)
    # no communicator
    assert L.cugp_bcm_predict_allgather(None, None, 1, 1, capi.ptr(Xt), 4, capi.ptr(m), capi.ptr(v)) == capi.CUGP_ERR_INVALID
    # a world of one without an id: creating it touches no device
    c = C.c_void_p()
    assert L.cugp_comm_create(None, 0, 0, 1, 0, C.byref(c)) == capi.CUGP_OK
    try:
        for per, nexp, nt, mp, vp in [(1, 1, 0, m, v),          # nt = 0
                                      (1, 1, -3, m, v),
                                      (1, 1, 4, None, v),       # null outputs
                                      (1, 1, 4, m, None),
                                      (0, 1, 4, m, v),          # per out of range
                                      (1, 0, 4, m, v),          # nexperts out of range
                                      (1, 2, 4, m, v)]:         # per * world < nexperts
            rc = L.cugp_bcm_predict_allgather(None, c, per, nexp, capi.ptr(Xt), nt,
                                              capi.ptr(mp) if mp is not None else None,
                                              capi.ptr(vp) if vp is not None else None)
            assert rc == capi.CUGP_ERR_INVALID, (per, nexp, nt)
        assert b"bad argument" in L.cugp_last_error()
    finally:
        L.cugp_comm_destroy(c)
