"""The Matern interface (covariance families beside the squared exponential) without a GPU: the five new entry points
are exported and bound with their argument counts, the Python keywords exist, and every argument error comes back as
CUGP_ERR_INVALID before any device call (a null or a dummy handle is never dereferenced, an unknown kind is refused
before the device count is asked for)."""
import ctypes as C
import inspect

import numpy as np
import pytest

import cugp_amd.gp as gp
from cugp_amd import capi

NEW = [("cugp_create_kernel", 6), ("cugp_kernel_kind", 2), ("cugp_bcm_create_kernel", 7),
       ("cugp_bcm_create_split_kernel", 9), ("cugp_bcm_kernel_kind", 2)]


@pytest.mark.parametrize("name, nargs", NEW)
def test_exported_and_bound(name, nargs):
    assert name in capi.SIGNATURES
    assert len(capi.SIGNATURES[name][1]) == nargs
    fn = getattr(capi.lib(), name)
    assert fn.restype is C.c_int and len(fn.argtypes) == nargs


def test_kernel_argument_sits_in_front_of_out():
    """Today's order of arguments, `int kernel` directly in front of `out`."""
    S = capi.SIGNATURES
    for new, old in (("cugp_create_kernel", "cugp_create_padded"), ("cugp_bcm_create_kernel", "cugp_bcm_create_multi"),
                     ("cugp_bcm_create_split_kernel", "cugp_bcm_create_split_multi")):
        assert S[new][1] == S[old][1][:-1] + [C.c_int] + S[old][1][-1:], new


def test_constants():
    assert (capi.CUGP_KERNEL_SE, capi.CUGP_KERNEL_MATERN32, capi.CUGP_KERNEL_MATERN52) == (0, 1, 2)
    assert gp.KERNELS == {"se": 0, "matern32": 1, "matern52": 2}


def test_python_keywords_exist():
    import cugp_amd.bcm as bcm
    import cugp_amd.train as train
    assert inspect.signature(gp.Covsum.__init__).parameters["kernel"].default == "se"
    assert inspect.signature(gp.BCM.__init__).parameters["kernel"].default == "se"
    assert inspect.signature(gp.BCM.split).parameters["kernel"].default == "se"
    assert inspect.signature(bcm.ShardedBCM.__init__).parameters["kernel"].default == "se"
    assert isinstance(gp.Covsum.kernel, property) and isinstance(gp.BCM.kernel, property)
    assert "--kernel" in inspect.getsource(train.main)


@pytest.mark.parametrize("kernel", ["matern32", "matern52", 1, 2])
def test_ard_with_matern_raises_before_any_call(kernel):
    with pytest.raises(ValueError, match="ARD"):
        gp.Covsum(10, 3, ard=True, kernel=kernel)


@pytest.mark.parametrize("kernel", ["rbf", "matern12", -1, 3])
def test_unknown_kernel_name_raises(kernel):
    with pytest.raises(ValueError):
        gp.Covsum(10, 3, kernel=kernel)
    with pytest.raises(ValueError):
        gp.BCM([10, 10], 3, kernel=kernel)


DUMMY = C.c_void_p(0x1000)     # never dereferenced: the checks come first


@pytest.mark.parametrize("handle", [None, DUMMY], ids=["null", "dummy"])
@pytest.mark.parametrize("kind", [-1, 3])
def test_argument_errors(handle, kind):
    L = capi.lib()
    INV = capi.CUGP_ERR_INVALID
    out, k = C.c_void_p(), C.c_int(7)
    # an unknown kind: refused with good sizes, before the device count is asked for (no device here: a known kind
    # with good arguments would be CUGP_ERR_NODEVICE, never CUGP_ERR_INVALID)
    assert L.cugp_create_kernel(10, 3, 0, 0, kind, C.byref(out)) == INV
    assert b"cugp_create_kernel" in L.cugp_last_error() and not out.value
    for good in (0, 1, 2):
        assert L.cugp_create_kernel(0, 3, 0, 0, good, C.byref(out)) == INV
        assert L.cugp_create_kernel(10, 0, 0, 0, good, C.byref(out)) == INV
        assert L.cugp_create_kernel(10, 3, 0, 0, good, None) == INV
    assert L.cugp_kernel_kind(None, C.byref(k)) == INV and L.cugp_kernel_kind(handle, None) == INV
    assert L.cugp_bcm_kernel_kind(None, C.byref(k)) == INV and L.cugp_bcm_kernel_kind(handle, None) == INV
    assert k.value == 7
    dev = np.zeros(1, dtype=np.int32).ctypes.data_as(capi._ip)
    rows = np.array([10, 10], dtype=np.int32).ctypes.data_as(capi._ip)
    assert L.cugp_bcm_create_kernel(1, dev, 2, rows, 3, kind, C.byref(out)) == INV
    assert L.cugp_bcm_create_kernel(1, dev, 2, rows, 3, 1, None) == INV
    assert L.cugp_bcm_create_kernel(0, dev, 2, rows, 3, 1, C.byref(out)) == INV
    assert L.cugp_bcm_create_kernel(1, None, 2, rows, 3, 2, C.byref(out)) == INV
    assert L.cugp_bcm_create_kernel(1, dev, 2, None, 3, 2, C.byref(out)) == INV
    X, y = np.zeros((20, 3)), np.zeros(20)
    assert L.cugp_bcm_create_split_kernel(capi.ptr(X), capi.ptr(y), 20, 3, 2, 1, dev, kind, C.byref(out)) == INV
    assert L.cugp_bcm_create_split_kernel(None, capi.ptr(y), 20, 3, 2, 1, dev, 1, C.byref(out)) == INV
    assert L.cugp_bcm_create_split_kernel(capi.ptr(X), capi.ptr(y), 20, 3, 21, 1, dev, 1, C.byref(out)) == INV
    assert not out.value
