"""The surface of cugp_append, no GPU: header, ctypes binding and built library agree on the new symbols; cugp_append_plan
(pure arithmetic) replayed; the argument refusals of cugp_append come back as CUGP_ERR_INVALID before any device call; the
Python keyword surface.
"""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import cugp_amd.gp as gp
from cugp_amd import capi
from cugp_amd.capi import ptr
from conftest import ROOT

_ip, _dp, _vpp = C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_void_p)
SYMBOLS = {
    "cugp_capacity": (r"int cugp_capacity\(const cugp_gp \*gp, int \*cap\);", [C.c_void_p, _ip]),
    "cugp_append": (r"int cugp_append\(cugp_gp \*gp, const double \*Xnew( /\*[^*]*\*/)?, const double \*ynew( /\*[^*]*\*/)?, int k\);",
                    [C.c_void_p, _dp, _dp, C.c_int]),
    "cugp_append_plan": (r"int cugp_append_plan\(int n, int k, int pass, int out\[2\]\);", [C.c_int, C.c_int, C.c_int, _ip]),
    "cugp_create_ard_padded": (r"int cugp_create_ard_padded\(int n, int d, int device, int npad_min, cugp_gp \*\*out\);",
                               [C.c_int, C.c_int, C.c_int, C.c_int, _vpp]),
}


@pytest.mark.parametrize("name", sorted(SYMBOLS))
def test_symbols_declared_bound_and_exported(name):
    """cugp_append, cugp_append_plan, cugp_capacity and cugp_create_ard_padded: in the header with the stated signature,
    bound with the same argument types, exported by the built library."""
    text = open(os.path.join(ROOT, "include", "cugp.h")).read()
    pattern, args = SYMBOLS[name]
    assert re.search(pattern, text), name
    res, bound = capi.SIGNATURES[name]
    assert res is C.c_int and bound == args
    assert hasattr(capi.lib(), name)


def test_header_says_what_is_not_built():
    text = open(os.path.join(ROOT, "include", "cugp.h")).read()
    doc = text[text.index("appending observations"):text.index("int cugp_append_plan")]
    for phrase in ("removing rows", "BCM experts", "with targets", "skips K^-1", "beyond the capacity", "CUGP_ERR_INVALID",
                   "not positive definite"):
        assert phrase in doc, phrase


def plan(n, k):
    out = (C.c_int * 2)()
    count = capi.lib().cugp_append_plan(n, k, 0, out)
    passes = []
    for p in range(count):
        assert capi.lib().cugp_append_plan(n, k, p, out) == count
        passes.append((out[0], out[1]))
    return count, passes


@pytest.mark.parametrize("k", [1, 2, 128, 129, 257])
@pytest.mark.parametrize("n", [1, 63, 127, 128, 129, 300])
def test_append_plan_replayed(n, k):
    """cugp_append_plan: no pass crosses a multiple of 128 (so each has at most 128 rows and lies in one tile row), the
    passes cover [n, n + k) exactly once, ascending; the count is the number of tile rows the new rows touch; a pass beyond
    the last is refused."""
    count, passes = plan(n, k)
    assert count == len(passes) == (n + k - 1) // 128 - n // 128 + 1
    at = n
    for a, b in passes:
        assert a == at and a < b
        assert a // 128 == (b - 1) // 128 and b - a <= 128
        at = b
    assert at == n + k
    out = (C.c_int * 2)(-7, -7)
    for p in (count, count + 3, -1):
        assert capi.lib().cugp_append_plan(n, k, p, out) == capi.CUGP_ERR_INVALID
    assert b"cugp_append_plan" in capi.lib().cugp_last_error()
    assert (out[0], out[1]) == (-7, -7)


def test_append_plan_argument_refusals():
    out = (C.c_int * 2)()
    lib = capi.lib()
    assert lib.cugp_append_plan(5, 3, 0, None) == capi.CUGP_ERR_INVALID
    for n, k in ((5, 0), (5, -2), (-1, 3), (2 ** 31 - 2, 5)):
        assert lib.cugp_append_plan(n, k, 0, out) == capi.CUGP_ERR_INVALID, (n, k)


def test_refusals_before_any_device_call():
    """NULL arguments and k <= 0 of cugp_append, NULL arguments of cugp_capacity: refused on the arguments alone (the fake
    handle is never dereferenced, no device is touched), with the call's name in cugp_last_error."""
    lib = capi.lib()
    null, fake = C.c_void_p(), C.c_void_p(1)
    X, y = np.zeros((2, 3)), np.zeros(2)
    assert lib.cugp_append(null, ptr(X), ptr(y), 2) == capi.CUGP_ERR_INVALID
    assert b"cugp_append" in lib.cugp_last_error() and b"null" in lib.cugp_last_error()
    assert lib.cugp_append(fake, None, ptr(y), 2) == capi.CUGP_ERR_INVALID
    assert lib.cugp_append(fake, ptr(X), None, 2) == capi.CUGP_ERR_INVALID
    for k in (0, -1, -128):
        assert lib.cugp_append(fake, ptr(X), ptr(y), k) == capi.CUGP_ERR_INVALID
        assert b"k must be positive" in lib.cugp_last_error()
    cap = C.c_int(-3)
    assert lib.cugp_capacity(null, C.byref(cap)) == capi.CUGP_ERR_INVALID
    assert lib.cugp_capacity(fake, None) == capi.CUGP_ERR_INVALID
    assert cap.value == -3


def test_python_surface():
    """Covsum.append(X, y), the capacity property, npad_min on every family (cugp_append needs the room)."""
    p = inspect.signature(gp.Covsum.append).parameters
    assert list(p) == ["self", "X", "y"]
    assert isinstance(gp.Covsum.capacity, property)
    p = inspect.signature(gp.Covsum.__init__).parameters
    assert p["npad_min"].default == 0 and p["ard"].default is False
    src = inspect.getsource(gp.Covsum.__init__)
    assert "cugp_create_ard_padded" in src
    assert "cugp_append" in inspect.getsource(gp.Covsum.append)


def test_python_append_shapes_without_a_device():
    """Covsum.append's shape handling, checked in front of the library call: on an object with a NULL handle every
    accepted shape reaches cugp_append (which refuses the NULL handle: CugpError, before any device call) and every other
    shape is a ValueError.  One row may come as a 1-d X with a Python or numpy scalar y, or a 0-d array."""
    g = gp.Covsum.__new__(gp.Covsum)
    g.n, g.d, g.device, g.ard, g._h, g._data_key = 5, 2, 0, False, C.c_void_p(), None
    X = np.arange(6.0).reshape(3, 2)
    y = np.arange(3.0)
    for args in ((X, y), (X[:1], y[:1]), (X[0], y[0]), (X[0], 1.5), (X[0], np.array(1.5)), ([1.0, 2.0], 3)):
        with pytest.raises(capi.CugpError, match="cugp_append: null argument"):
            g.append(*args)
    for args in ((X[0], y[:1]), (X, y[:2]), (X[:, :1], y), (X[0, :1], 1.0), (X, 1.0), (X.reshape(3, 2, 1), y)):
        with pytest.raises(ValueError):
            g.append(*args)
    assert g.n == 5 and g._data_key is None
    g._h = C.c_void_p()                                               # (nothing to destroy)
