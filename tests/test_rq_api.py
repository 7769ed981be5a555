"""The rational quadratic interface without a GPU: the three create calls are declared, exported and bound, and the header
carries the model's formulas; NULL arguments, bad sizes and an `ard` outside {0, 1} come back as CUGP_ERR_INVALID with the
call's name before the device count is asked for (a good call here, with no device, is CUGP_ERR_NODEVICE, never INVALID);
the existing create calls keep refusing kind 3; the Python names kernel="rq" | "rq_ard" reach Covsum, BCM, BCM.split,
ShardedBCM and train.py, the number 3 and the sparse model do not."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import cugp_amd.gp as gp
from cugp_amd import capi
from cugp_amd.bcm import ShardedBCM

INV, NODEV = capi.CUGP_ERR_INVALID, capi.CUGP_ERR_NODEVICE
# new call -> the ARD call it extends by `int ard` directly in front of `out`
NEW = {"cugp_create_rq": "cugp_create_ard_padded", "cugp_bcm_create_rq": "cugp_bcm_create_ard",
       "cugp_bcm_create_split_rq": "cugp_bcm_create_split_ard"}
HEADER = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cugp.h")).read()


@pytest.mark.parametrize("name", NEW)
def test_declared_exported_and_bound(name):
    m = re.search(r"\bint %s\(([^;]*)\);" % name, HEADER)
    assert m, name
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    assert args[-2] == "int ard" and args[-1].endswith("**out"), args
    S = capi.SIGNATURES
    assert S[name][1] == S[NEW[name]][1][:-1] + [C.c_int] + S[NEW[name]][1][-1:]
    fn = getattr(capi.lib(), name)
    assert fn.restype is C.c_int and len(fn.argtypes) == len(S[name][1])


def test_header_carries_the_model():
    assert re.search(r"#define CUGP_KERNEL_RQ 3\b", HEADER) and capi.CUGP_KERNEL_RQ == 3
    text = " ".join(HEADER.split())
    for piece in ("u = s / (2 alpha)", "L = log1p(u)", "Kf = sf2 exp(-alpha L)", "H = Kf / (1 + u)",
                  "A = Kf alpha (u / (1 + u) - L)", "g_d = 1/2 sum W o A", "nh = d + 3", "nh = 4",
                  "theta = [log l, log alpha, log sigma_f, log sigma_n]", "g_0 = g_l1 + ... + g_ld"):
        assert piece in text, piece


def _ptrs():
    dev = np.zeros(1, dtype=np.int32)
    rows = np.array([10, 10], dtype=np.int32)
    zero = np.array([10, 0], dtype=np.int32)
    return dev, rows, zero, np.zeros((20, 3)), np.zeros(20)


def _refused(rc, name):
    return rc == INV and name.encode() in capi.lib().cugp_last_error()


@pytest.mark.parametrize("ard", [0, 1])
def test_null_arguments_and_bad_sizes_are_invalid_with_the_calls_name(ard):
    L = capi.lib()
    out = C.c_void_p()
    dev, rows, zero, X, y = _ptrs()
    ip = lambda a: a.ctypes.data_as(capi._ip)
    for bad in ((0, 3, 0, 0, ard, C.byref(out)), (10, 0, 0, 0, ard, C.byref(out)), (-1, 3, 0, 0, ard, C.byref(out)),
                (10, 3, 0, -1, ard, C.byref(out)), (10, 3, 0, 0, ard, None)):
        assert _refused(L.cugp_create_rq(*bad), "cugp_create_rq"), bad
    for bad in ((0, ip(dev), 2, ip(rows), 3), (1, None, 2, ip(rows), 3), (1, ip(dev), 0, ip(rows), 3),
                (1, ip(dev), 2, None, 3), (1, ip(dev), 2, ip(rows), 0), (1, ip(dev), 2, ip(zero), 3)):
        assert _refused(L.cugp_bcm_create_rq(*bad, ard, C.byref(out)), "cugp_bcm_create_rq"), bad
    assert _refused(L.cugp_bcm_create_rq(1, ip(dev), 2, ip(rows), 3, ard, None), "cugp_bcm_create_rq")
    for bad in ((None, capi.ptr(y), 20, 3, 2, 1, ip(dev)), (capi.ptr(X), None, 20, 3, 2, 1, ip(dev)),
                (capi.ptr(X), capi.ptr(y), 20, 3, 21, 1, ip(dev)), (capi.ptr(X), capi.ptr(y), 20, 0, 2, 1, ip(dev)),
                (capi.ptr(X), capi.ptr(y), 0, 3, 2, 1, ip(dev)), (capi.ptr(X), capi.ptr(y), 20, 3, 0, 1, ip(dev)),
                (capi.ptr(X), capi.ptr(y), 20, 3, 2, 0, ip(dev)), (capi.ptr(X), capi.ptr(y), 20, 3, 2, 1, None)):
        assert _refused(L.cugp_bcm_create_split_rq(*bad, ard, C.byref(out)), "cugp_bcm_create_split_rq"), bad
    assert _refused(L.cugp_bcm_create_split_rq(capi.ptr(X), capi.ptr(y), 20, 3, 2, 1, ip(dev), ard, None),
                    "cugp_bcm_create_split_rq")
    assert not out.value


@pytest.mark.parametrize("ard", [-1, 2, 3])
def test_ard_outside_0_1_is_invalid_with_the_calls_name(ard):
    L = capi.lib()
    out = C.c_void_p()
    dev, rows, _, X, y = _ptrs()
    ip = lambda a: a.ctypes.data_as(capi._ip)
    assert _refused(L.cugp_create_rq(10, 3, 0, 0, ard, C.byref(out)), "cugp_create_rq")
    assert _refused(L.cugp_bcm_create_rq(1, ip(dev), 2, ip(rows), 3, ard, C.byref(out)), "cugp_bcm_create_rq")
    assert _refused(L.cugp_bcm_create_split_rq(capi.ptr(X), capi.ptr(y), 20, 3, 2, 1, ip(dev), ard, C.byref(out)),
                    "cugp_bcm_create_split_rq")
    assert not out.value


@pytest.mark.parametrize("ard", [0, 1])
def test_good_call_without_a_device_is_nodevice(ard):
    n = C.c_int(-1)
    L = capi.lib()
    if L.cugp_device_count(C.byref(n)) == 0 and n.value > 0:
        pytest.skip("a GPU is visible: a good call succeeds (tests/test_gpu_rq.py)")
    out = C.c_void_p()
    dev, rows, _, X, y = _ptrs()
    ip = lambda a: a.ctypes.data_as(capi._ip)
    assert L.cugp_create_rq(10, 3, 0, 0, ard, C.byref(out)) == NODEV
    assert L.cugp_bcm_create_rq(1, ip(dev), 2, ip(rows), 3, ard, C.byref(out)) == NODEV
    assert L.cugp_bcm_create_split_rq(capi.ptr(X), capi.ptr(y), 20, 3, 2, 1, ip(dev), ard, C.byref(out)) == NODEV
    assert not out.value


def test_existing_create_calls_still_refuse_kind_3():
    L = capi.lib()
    out = C.c_void_p()
    dev, rows, _, X, y = _ptrs()
    ip = lambda a: a.ctypes.data_as(capi._ip)
    assert L.cugp_create_kernel(10, 3, 0, 0, 3, C.byref(out)) == INV
    assert L.cugp_create_ard_kernel(10, 3, 0, 0, 3, C.byref(out)) == INV
    assert L.cugp_bcm_create_kernel(1, ip(dev), 2, ip(rows), 3, 3, C.byref(out)) == INV
    assert L.cugp_bcm_create_ard_kernel(1, ip(dev), 2, ip(rows), 3, 3, C.byref(out)) == INV
    assert L.cugp_bcm_create_split_kernel(capi.ptr(X), capi.ptr(y), 20, 3, 2, 1, ip(dev), 3, C.byref(out)) == INV
    assert L.cugp_bcm_create_split_ard_kernel(capi.ptr(X), capi.ptr(y), 20, 3, 2, 1, ip(dev), 3, C.byref(out)) == INV
    for ard in (0, 1):
        assert L.cugp_sparse_create(20, 5, 3, 0, 3, ard, 1e-6, 0, C.byref(out)) == INV
    assert not out.value


def test_names():
    assert gp.RQ_KERNELS == {"rq": False, "rq_ard": True}
    assert gp.KERNELS == {"se": 0, "matern32": 1, "matern52": 2}                  # (the number 3 is no kernel=)
    assert gp.kernel_spec("rq") == (3, False) and gp.kernel_spec("RQ_ARD") == (3, True)
    assert gp.kernel_spec("rq_ard", ard=True) == (3, True)
    assert gp.num_hyper(3, False, 7) == 4 and gp.num_hyper(3, True, 7) == 10 and gp.num_hyper(0, True, 7) == 9
    assert gp.num_hyper(1, False, 7) == 3
    with pytest.raises(ValueError, match="rq_ard"):
        gp.kernel_spec("rq", ard=True)
    for bad in (3, "rq_iso", "rational_quadratic", "rq_ard_"):
        with pytest.raises(ValueError):
            gp.kernel_spec(bad)


@pytest.mark.parametrize("kernel", [3, "rq_iso"])
def test_the_number_3_and_a_bad_name_raise_before_any_library_call(monkeypatch, kernel):
    monkeypatch.setattr(capi, "lib", lambda: pytest.fail("a library call was made"))
    X, y = np.zeros((20, 3)), np.zeros(20)
    for make in (lambda: gp.Covsum(10, 3, kernel=kernel), lambda: gp.BCM([10, 10], 3, kernel=kernel),
                 lambda: gp.BCM.split(X, y, 2, kernel=kernel),
                 lambda: ShardedBCM([(X, y)], kernel=kernel, expert_factory=lambda *a, **k: None)):
        with pytest.raises(ValueError):
            make()


@pytest.mark.parametrize("kernel", ["rq", "rq_ard"])
def test_sparse_gp_refuses_the_family_before_any_library_call(monkeypatch, kernel):
    monkeypatch.setattr(capi, "lib", lambda: pytest.fail("a library call was made"))
    with pytest.raises(ValueError, match="rational quadratic"):
        gp.SparseGP(20, 5, 3, kernel=kernel)


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


@pytest.mark.parametrize("kernel, ard, nh", [("rq", 0, 4), ("rq_ard", 1, 6)])
def test_keyword_reaches_the_create_calls(monkeypatch, kernel, ard, nh):
    rec = _Recorder()
    monkeypatch.setattr(capi, "lib", lambda: rec)
    X, y = np.zeros((20, 3)), np.zeros(20)
    with pytest.raises(capi.CugpError):
        gp.Covsum(10, 3, npad_min=256, kernel=kernel)
    assert rec.calls[-1][0] == "cugp_create_rq" and rec.calls[-1][1][:5] == (10, 3, 0, 256, ard)
    with pytest.raises(capi.CugpError):
        gp.BCM([10, 12], 3, kernel=kernel)
    assert rec.calls[-1][0] == "cugp_bcm_create_rq" and rec.calls[-1][1][4:6] == (3, ard)
    with pytest.raises(capi.CugpError):
        gp.BCM.split(X, y, 2, kernel=kernel)
    assert rec.calls[-1][0] == "cugp_bcm_create_rq" and rec.calls[-1][1][4:6] == (3, ard)


@pytest.mark.parametrize("kernel, ard, nh", [("rq", False, 4), ("rq_ard", True, 6)])
def test_python_attributes(kernel, ard, nh):
    """nh, .ard and the nh-wide routing of a handle object, without creating a handle."""
    g = gp.Covsum.__new__(gp.Covsum)
    g.n, g.d, g.device = 10, 3, 0
    g._kind, g.ard = gp.kernel_spec(kernel)
    g.nh = gp.num_hyper(g._kind, g.ard, g.d)
    assert g.ard is ard and g.nh == nh and g._wide and g.get_param_dim() == nh
    assert gp.REPORTED_NAMES[capi.CUGP_KERNEL_RQ] == "rq"
    g._h = C.c_void_p()                       # (nothing to destroy)


class _Expert:
    def __init__(self, n, d, device, ard=False):
        self.n, self.d, self.ard = n, d, ard

    def set_data(self, X, y):
        pass

    def close(self):
        pass


def test_keyword_reaches_sharded_bcm():
    X, y = np.zeros((20, 3)), np.zeros(20)
    b = ShardedBCM([(X, y), (X, y)], kernel="rq_ard", expert_factory=_Expert)
    assert b.ard and b.nh == 6 and b.kernel == "rq" and b._kernel_arg == "rq_ard" and b._wide
    assert all(e.ard for e in b.local.values()) and b.hp.shape == (6,) and b._w == 7
    t = ShardedBCM([(X, y), (X, y)], kernel="rq", expert_factory=_Expert)
    assert not t.ard and t.nh == 4 and t.kernel == "rq" and t._kernel_arg == "rq" and t._wide
    assert t.hp.shape == (4,) and t._w == 5 and not any(e.ard for e in t.local.values())
    iso = ShardedBCM([(X, y)], kernel="matern52", expert_factory=_Expert)
    assert not iso.ard and iso.nh == 3 and not iso._wide


def test_train_accepts_the_names():
    import cugp_amd.train as train
    src = inspect.getsource(train.main)
    assert '"rq"' in src and '"rq_ard"' in src and "start_vector" in src
    assert train.start_vector([2.0, 3.0, 4.0], 3, "se") == [2.0, 3.0, 4.0]
    assert train.start_vector([2.0, 3.0, 4.0], 5, "matern52_ard") == [2.0, 2.0, 2.0, 3.0, 4.0]
    assert train.start_vector([2.0, 3.0, 4.0], 4, "rq") == [2.0, 0.0, 3.0, 4.0]
    assert train.start_vector([2.0, 3.0, 4.0], 6, "rq_ard") == [2.0, 2.0, 2.0, 0.0, 3.0, 4.0]
