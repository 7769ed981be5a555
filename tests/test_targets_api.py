"""The multi-target interface (m target vectors over one factorisation) without a GPU: the six entry points are exported
and bound with the header's argument counts, the Python methods exist, every argument error comes back as
CUGP_ERR_INVALID with the call's name before any device call (a null or a dummy handle is never dereferenced), and good
arguments without a device give CUGP_ERR_NODEVICE, never a value."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cugp_amd.gp as gp
from conftest import ROOT
from cugp_amd import capi

NEW = [("cugp_set_targets", 3), ("cugp_num_targets", 2), ("cugp_loglik_grad_targets", 5), ("cugp_predict_targets", 5),
       ("cugp_get_alpha_targets", 2), ("cugp_cg_solve_targets", 5)]
INV = capi.CUGP_ERR_INVALID
DUMMY = C.c_void_p(0x1000)     # never dereferenced: the checks come first


@pytest.mark.parametrize("name, nargs", NEW)
def test_exported_and_bound(name, nargs):
    assert name in capi.SIGNATURES
    assert len(capi.SIGNATURES[name][1]) == nargs
    fn = getattr(capi.lib(), name)
    assert fn.restype is C.c_int and len(fn.argtypes) == nargs


@pytest.mark.parametrize("name, nargs", NEW)
def test_header_declares_the_same_argument_count(name, nargs):
    with open(os.path.join(ROOT, "include", "cugp.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, text)
    assert decl, name
    assert len(decl.group(1).split(",")) == nargs


def test_python_methods_exist():
    for name in ("set_targets", "loglik_grad_targets", "predict_targets", "get_alpha_targets", "cg_solve_targets"):
        assert callable(getattr(gp.Covsum, name)), name
    assert isinstance(gp.Covsum.num_targets, property)


def refused(rc, call):
    return rc == INV and call.encode() in capi.lib().cugp_last_error()


@pytest.mark.parametrize("handle", [None, DUMMY], ids=["null", "dummy"])
def test_argument_errors(handle):
    L = capi.lib()
    Y, Xt, out = np.zeros((2, 10)), np.zeros((4, 3)), np.zeros(64)
    ll, m, ne = C.c_double(7.0), C.c_int(7), C.c_int(7)
    # a null handle, whatever else is given
    assert refused(L.cugp_set_targets(None, capi.ptr(Y), 2), "cugp_set_targets")
    assert refused(L.cugp_num_targets(None, C.byref(m)), "cugp_num_targets")
    assert refused(L.cugp_loglik_grad_targets(None, C.byref(ll), capi.ptr(out), 3, capi.ptr(out)), "cugp_loglik_grad_targets")
    assert refused(L.cugp_predict_targets(None, capi.ptr(Xt), 4, capi.ptr(out), capi.ptr(out)), "cugp_predict_targets")
    assert refused(L.cugp_get_alpha_targets(None, capi.ptr(out)), "cugp_get_alpha_targets")
    assert refused(L.cugp_cg_solve_targets(None, 5, None, 0, C.byref(ne)), "cugp_cg_solve_targets")
    # null pointers and sizes that cannot be: refused before the handle is looked at
    assert refused(L.cugp_set_targets(handle, None, 2), "cugp_set_targets")
    assert refused(L.cugp_set_targets(handle, capi.ptr(Y), 0), "cugp_set_targets")
    assert refused(L.cugp_set_targets(handle, capi.ptr(Y), -3), "cugp_set_targets")
    assert refused(L.cugp_num_targets(handle, None), "cugp_num_targets")
    assert refused(L.cugp_predict_targets(handle, None, 4, capi.ptr(out), capi.ptr(out)), "cugp_predict_targets")
    assert refused(L.cugp_predict_targets(handle, capi.ptr(Xt), 4, None, capi.ptr(out)), "cugp_predict_targets")
    assert refused(L.cugp_predict_targets(handle, capi.ptr(Xt), 0, capi.ptr(out), capi.ptr(out)), "cugp_predict_targets")
    assert refused(L.cugp_predict_targets(handle, capi.ptr(Xt), -1, capi.ptr(out), None), "cugp_predict_targets")
    assert refused(L.cugp_get_alpha_targets(handle, None), "cugp_get_alpha_targets")
    # no handle has fewer than three hyper-parameters
    for nh in (2, 0, -1):
        assert refused(L.cugp_loglik_grad_targets(handle, C.byref(ll), capi.ptr(out), nh, None), "cugp_loglik_grad_targets")
    assert (ll.value, m.value, ne.value) == (7.0, 7, 7) and not out.any()


def test_no_device_is_never_a_value():
    """Good arguments in a process without a GPU: CUGP_ERR_NODEVICE before the (dummy) handle is looked at.  Where a
    device is visible the same calls would go on to the handle, so they are only made without one."""
    L = capi.lib()
    cnt = C.c_int()
    if L.cugp_device_count(C.byref(cnt)) == capi.CUGP_OK and cnt.value > 0:
        return
    NODEV = capi.CUGP_ERR_NODEVICE
    Y, Xt, out = np.zeros((2, 10)), np.zeros((4, 3)), np.zeros(64)
    ll, ne = C.c_double(7.0), C.c_int(7)
    assert L.cugp_set_targets(DUMMY, capi.ptr(Y), 2) == NODEV
    assert L.cugp_loglik_grad_targets(DUMMY, C.byref(ll), capi.ptr(out), 3, capi.ptr(out)) == NODEV
    assert L.cugp_predict_targets(DUMMY, capi.ptr(Xt), 4, capi.ptr(out), capi.ptr(out)) == NODEV
    assert L.cugp_get_alpha_targets(DUMMY, capi.ptr(out)) == NODEV
    assert L.cugp_cg_solve_targets(DUMMY, 5, None, 0, C.byref(ne)) == NODEV
    assert (ll.value, ne.value) == (7.0, 7) and not out.any()
    with pytest.raises(capi.CugpError) as e:
        gp.Covsum(10, 3)
    assert e.value.code == NODEV
