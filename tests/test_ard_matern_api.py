"""The ARD x Matern interface without a GPU: the three create calls are declared, exported and bound with `int kernel`
directly in front of `out`; an unknown kind and bad sizes come back as CUGP_ERR_INVALID before the device count is asked
for (a good call here, with no device, is CUGP_ERR_NODEVICE, never INVALID); the Python spelling kernel="matern32_ard" |
"matern52_ard" reaches Covsum, BCM, BCM.split, ShardedBCM and train.py, and the existing names and refusals stand."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import cugp_amd.gp as gp
from cugp_amd import capi
from cugp_amd.bcm import ShardedBCM

NEW = {"cugp_create_ard_kernel": "cugp_create_ard_padded", "cugp_bcm_create_ard_kernel": "cugp_bcm_create_ard",
       "cugp_bcm_create_split_ard_kernel": "cugp_bcm_create_split_ard"}
INV, NODEV = capi.CUGP_ERR_INVALID, capi.CUGP_ERR_NODEVICE


@pytest.mark.parametrize("name", NEW)
def test_declared_exported_and_bound(name):
    """In the header with `int kernel` in front of `out`, in capi.SIGNATURES as the kind-less call + that int, and in the
    library."""
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cugp.h")).read()
    m = re.search(r"\bint %s\(([^;]*)\);" % name, header)
    assert m, name
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    assert args[-2] == "int kernel" and args[-1].endswith("**out"), args
    S = capi.SIGNATURES
    assert S[name][1] == S[NEW[name]][1][:-1] + [C.c_int] + S[NEW[name]][1][-1:]
    fn = getattr(capi.lib(), name)
    assert fn.restype is C.c_int and len(fn.argtypes) == len(S[name][1])


def _calls(kind, out, n=10, d=3, rows=(10, 10), K=2):
    """The three calls with the given kind and otherwise good arguments -> [(name, return code)]."""
    L = capi.lib()
    dev = np.zeros(1, dtype=np.int32)
    r = np.array(rows, dtype=np.int32)
    X, y = np.zeros((20, 3)), np.zeros(20)
    return [("cugp_create_ard_kernel", L.cugp_create_ard_kernel(n, d, 0, 0, kind, C.byref(out))),
            ("cugp_bcm_create_ard_kernel",
             L.cugp_bcm_create_ard_kernel(1, dev.ctypes.data_as(capi._ip), len(rows), r.ctypes.data_as(capi._ip), d, kind,
                                          C.byref(out))),
            ("cugp_bcm_create_split_ard_kernel",
             L.cugp_bcm_create_split_ard_kernel(capi.ptr(X), capi.ptr(y), 20, 3, K, 1, dev.ctypes.data_as(capi._ip), kind,
                                                C.byref(out)))]


@pytest.mark.parametrize("kind", [-1, 3])
def test_unknown_kind_is_invalid_with_the_calls_name(kind):
    L = capi.lib()
    out = C.c_void_p()
    dev = np.zeros(1, dtype=np.int32).ctypes.data_as(capi._ip)
    rows = np.array([10, 10], dtype=np.int32).ctypes.data_as(capi._ip)
    X, y = np.zeros((20, 3)), np.zeros(20)
    assert L.cugp_create_ard_kernel(10, 3, 0, 0, kind, C.byref(out)) == INV
    assert b"cugp_create_ard_kernel" in L.cugp_last_error()
    assert L.cugp_bcm_create_ard_kernel(1, dev, 2, rows, 3, kind, C.byref(out)) == INV
    assert b"cugp_bcm_create_ard_kernel" in L.cugp_last_error()
    assert L.cugp_bcm_create_split_ard_kernel(capi.ptr(X), capi.ptr(y), 20, 3, 2, 1, dev, kind, C.byref(out)) == INV
    assert b"cugp_bcm_create_split_ard_kernel" in L.cugp_last_error()
    assert not out.value
    assert L.cugp_create_kernel(10, 3, 0, 0, 3, C.byref(out)) == INV            # (the isotropic call keeps refusing kind 3)


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_bad_sizes_are_invalid(kind):
    L = capi.lib()
    out = C.c_void_p()
    dev = np.zeros(1, dtype=np.int32).ctypes.data_as(capi._ip)
    rows = np.array([10, 10], dtype=np.int32).ctypes.data_as(capi._ip)
    zero = np.array([10, 0], dtype=np.int32).ctypes.data_as(capi._ip)
    X, y = np.zeros((20, 3)), np.zeros(20)
    assert L.cugp_create_ard_kernel(0, 3, 0, 0, kind, C.byref(out)) == INV
    assert L.cugp_create_ard_kernel(10, 0, 0, 0, kind, C.byref(out)) == INV
    assert L.cugp_create_ard_kernel(10, 3, 0, 0, kind, None) == INV
    assert L.cugp_bcm_create_ard_kernel(0, dev, 2, rows, 3, kind, C.byref(out)) == INV
    assert L.cugp_bcm_create_ard_kernel(1, None, 2, rows, 3, kind, C.byref(out)) == INV
    assert L.cugp_bcm_create_ard_kernel(1, dev, 0, rows, 3, kind, C.byref(out)) == INV
    assert L.cugp_bcm_create_ard_kernel(1, dev, 2, None, 3, kind, C.byref(out)) == INV
    assert L.cugp_bcm_create_ard_kernel(1, dev, 2, rows, 0, kind, C.byref(out)) == INV
    assert L.cugp_bcm_create_ard_kernel(1, dev, 2, zero, 3, kind, C.byref(out)) == INV
    assert L.cugp_bcm_create_ard_kernel(1, dev, 2, rows, 3, kind, None) == INV
    assert L.cugp_bcm_create_split_ard_kernel(None, capi.ptr(y), 20, 3, 2, 1, dev, kind, C.byref(out)) == INV
    assert L.cugp_bcm_create_split_ard_kernel(capi.ptr(X), None, 20, 3, 2, 1, dev, kind, C.byref(out)) == INV
    assert L.cugp_bcm_create_split_ard_kernel(capi.ptr(X), capi.ptr(y), 20, 3, 21, 1, dev, kind, C.byref(out)) == INV
    assert L.cugp_bcm_create_split_ard_kernel(capi.ptr(X), capi.ptr(y), 20, 0, 2, 1, dev, kind, C.byref(out)) == INV
    assert not out.value


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_good_call_without_a_device_is_nodevice(kind):
    n = C.c_int(-1)
    if capi.lib().cugp_device_count(C.byref(n)) == 0 and n.value > 0:
        pytest.skip("a GPU is visible: a good call succeeds (tests/test_gpu_ard_matern.py)")
    out = C.c_void_p()
    for name, rc in _calls(kind, out):
        assert rc == NODEV, (name, rc, capi.lib().cugp_last_error())
    assert not out.value


def test_names():
    assert gp.ARD_KERNELS == {"matern32_ard": capi.CUGP_KERNEL_MATERN32, "matern52_ard": capi.CUGP_KERNEL_MATERN52}
    assert gp.KERNELS == {"se": 0, "matern32": 1, "matern52": 2}
    assert gp.kernel_spec("matern52_ard") == (2, True) and gp.kernel_spec("MATERN32_ARD", ard=True) == (1, True)
    assert gp.kernel_spec("se", True) == (0, True) and gp.kernel_spec("matern32") == (1, False)
    assert gp.kernel_spec(2) == (2, False)


@pytest.mark.parametrize("kernel", ["matern32", "matern52", 1, 2])
def test_ard_true_with_a_matern_kernel_still_raises_and_names_the_spelling(kernel):
    X, y = np.zeros((20, 3)), np.zeros(20)
    for make in (lambda: gp.Covsum(10, 3, ard=True, kernel=kernel), lambda: gp.BCM([10, 10], 3, ard=True, kernel=kernel),
                 lambda: gp.BCM.split(X, y, 2, ard=True, kernel=kernel),
                 lambda: ShardedBCM([(X, y)], ard=True, kernel=kernel, expert_factory=lambda *a, **k: None)):
        with pytest.raises(ValueError, match="ARD") as ei:
            make()
        assert "squared-exponential only" in str(ei.value) and "_ard" in str(ei.value)


@pytest.mark.parametrize("kernel", ["se_ard", "matern12_ard", "rbf_ard", "matern52_ARD_"])
def test_unknown_ard_names_raise(kernel):
    X, y = np.zeros((20, 3)), np.zeros(20)
    with pytest.raises(ValueError):
        gp.Covsum(10, 3, kernel=kernel)
    with pytest.raises(ValueError):
        gp.BCM([10, 10], 3, kernel=kernel)
    with pytest.raises(ValueError):
        ShardedBCM([(X, y)], kernel=kernel, expert_factory=lambda *a, **k: None)


class _Recorder:
    """Stands for capi.lib(): records the create call it is asked for and fails it, so no handle is ever used."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return capi.CUGP_ERR_NODEVICE
        return call

    def cugp_last_error(self):
        return b"recorded"


@pytest.mark.parametrize("kernel, kind", [("matern32_ard", 1), ("matern52_ard", 2)])
def test_keyword_reaches_the_create_calls(monkeypatch, kernel, kind):
    """Covsum, BCM and BCM.split issue the _ard_kernel call with the kind directly in front of out."""
    rec = _Recorder()
    monkeypatch.setattr(capi, "lib", lambda: rec)
    X, y = np.zeros((20, 3)), np.zeros(20)
    with pytest.raises(capi.CugpError):
        gp.Covsum(10, 3, npad_min=256, kernel=kernel)
    assert rec.calls[-1][0] == "cugp_create_ard_kernel" and rec.calls[-1][1][:5] == (10, 3, 0, 256, kind)
    with pytest.raises(capi.CugpError):
        gp.BCM([10, 12], 3, kernel=kernel)
    assert rec.calls[-1][0] == "cugp_bcm_create_ard_kernel" and rec.calls[-1][1][4:6] == (3, kind)
    with pytest.raises(capi.CugpError):
        gp.BCM.split(X, y, 2, kernel=kernel)
    assert rec.calls[-1][0] == "cugp_bcm_create_ard_kernel" and rec.calls[-1][1][4:6] == (3, kind)
    n = len(rec.calls)
    with pytest.raises(capi.CugpError):
        gp.Covsum(10, 3, ard=True)                                   # SE-ARD keeps its own call
    assert rec.calls[n][0] == "cugp_create_ard"


class _Expert:
    def __init__(self, n, d, device, ard=False):
        self.n, self.d, self.ard = n, d, ard

    def set_data(self, X, y):
        pass

    def close(self):
        pass


@pytest.mark.parametrize("kernel, name", [("matern32_ard", "matern32"), ("matern52_ard", "matern52")])
def test_keyword_reaches_sharded_bcm(kernel, name):
    """With an injected expert_factory: ARD rows (nh = d + 2), the factory called with ard=True, .kernel the library's kind
    name beside .ard; without one the experts would be made with the same spelling."""
    X, y = np.zeros((20, 3)), np.zeros(20)
    b = ShardedBCM([(X, y), (X, y)], kernel=kernel, expert_factory=_Expert)
    assert b.ard and b.nh == 5 and b.kernel == name and b._kernel_arg == kernel
    assert all(e.ard for e in b.local.values()) and b.hp.shape == (5,)
    iso = ShardedBCM([(X, y)], kernel=name, expert_factory=_Expert)
    assert not iso.ard and iso.nh == 3 and iso._kernel_arg == name
    se = ShardedBCM([(X, y)], ard=True, expert_factory=_Expert)
    assert se.ard and se.kernel == "se" and se._kernel_arg == "se"


def test_train_accepts_the_names():
    import cugp_amd.train as train
    src = inspect.getsource(train.main)
    assert '"matern32_ard"' in src and '"matern52_ard"' in src and "bcm.ard" in src
