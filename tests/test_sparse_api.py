"""The sparse-GP interface without a GPU: the entry points are exported and bound with the header's signatures, the header
states the model, the cap on m and what is not built, every argument error comes back as CUGP_ERR_INVALID with the call's
name before any device call (a null handle is never dereferenced, and cugp_sparse_create refuses bad arguments before it
looks for a device), good arguments without a device give CUGP_ERR_NODEVICE, never a handle, and the plumbing of SparseGP
and of train.py --inducing is in place."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cugp_amd.gp as gp
from conftest import ROOT
from cugp_amd import capi, train

_dp, _ip, _vp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_void_p
NEW = {
    "cugp_sparse_create": [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.POINTER(_vp)],
    "cugp_sparse_destroy": [_vp],
    "cugp_sparse_dims": [_vp, _ip, _ip, _ip, _ip, _ip],
    "cugp_sparse_num_hyper": [_vp, _ip],
    "cugp_sparse_set_data": [_vp, _dp, _dp],
    "cugp_sparse_set_inducing": [_vp, _dp],
    "cugp_sparse_set_loghyper": [_vp, _dp, C.c_int],
    "cugp_sparse_get_loghyper": [_vp, _dp, C.c_int],
    "cugp_sparse_bound": [_vp, _dp],
    "cugp_sparse_bound_grad": [_vp, _dp, _dp, C.c_int],
    "cugp_sparse_predict": [_vp, _dp, C.c_int, C.c_int, _dp, _dp],
    "cugp_sparse_cg_solve": [_vp, C.c_int, _dp, C.c_int, _ip],
    "cugp_sparse_plan": [C.c_int, C.c_int, C.c_int, C.c_int, _ip],
    "cugp_sparse_predict_plan": [C.c_int, C.c_int, C.c_int, _ip],
}
DECLS = {
    "cugp_sparse_create": "int n, int m, int d, int device, int kernel, int ard, double jitter, int chunk_rows, cugp_sparse **out",
    "cugp_sparse_destroy": "cugp_sparse *sp",
    "cugp_sparse_dims": "const cugp_sparse *sp, int *n, int *m, int *d, int *mpad, int *chunk_rows",
    "cugp_sparse_num_hyper": "const cugp_sparse *sp, int *nh",
    "cugp_sparse_set_data": "cugp_sparse *sp, const double *X, const double *y",
    "cugp_sparse_set_inducing": "cugp_sparse *sp, const double *Z",
    "cugp_sparse_set_loghyper": "cugp_sparse *sp, const double *hp, int nh",
    "cugp_sparse_get_loghyper": "const cugp_sparse *sp, double *hp, int nh",
    "cugp_sparse_bound": "cugp_sparse *sp, double *F",
    "cugp_sparse_bound_grad": "cugp_sparse *sp, double *F, double *g, int nh",
    "cugp_sparse_predict": "cugp_sparse *sp, const double *Xt, int nt, int with_noise, double *mean, double *var",
    "cugp_sparse_cg_solve": "cugp_sparse *sp, int budget, double *trace, int trace_cap, int *nevals",
    "cugp_sparse_plan": "int n, int m, int chunk_rows, int pass, int out[5]",
    "cugp_sparse_predict_plan": "int m, int nt, int pass, int out[2]",
}
INV = capi.CUGP_ERR_INVALID


def header():
    with open(os.path.join(ROOT, "include", "cugp.h")) as f:
        return f.read()


@pytest.mark.parametrize("name", sorted(NEW))
def test_exported_and_bound(name):
    assert name in capi.SIGNATURES
    res, args = capi.SIGNATURES[name]
    assert res is C.c_int and args == NEW[name]
    fn = getattr(capi.lib(), name)
    assert fn.restype is C.c_int and list(fn.argtypes) == NEW[name]


@pytest.mark.parametrize("name", sorted(NEW))
def test_header_declares_the_signature(name):
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, text)
    assert decl, name
    assert " ".join(decl.group(1).split()).replace(" ,", ",") == DECLS[name]


def test_header_states_the_model_the_cap_and_what_is_not_built():
    text = " ".join(re.sub(r"\n\s*\*(?!/)", " ", header()).split())      # (comment lines joined, their leading stars dropped)
    for words in ("sparse variational GP regression on M inducing inputs", "Titsias 2009",
                  "F(theta) = -N/2 log 2 pi - 1/2 log|Qff + s2 I| - 1/2 y'(Qff + s2 I)^-1 y - (N sf2 - tr Qff) / (2 s2)",
                  "Lu = chol(Kuu), A = Lu^-1 Kuf / s, B = I + A A', LB = chol(B), c = LB^-1 A y / s",
                  "var_f = sf2 - |Lu^-1 ks|^2 + |LB^-1 Lu^-1 ks|^2", "G_uf = 2 G_Phi Kuf + (beta / s2) y'",
                  "equal inputs and chunk_rows give equal bits", "m <= CUGP_SPARSE_MAX_M",
                  "every element offset of the inner factorisation's kernels fits an int",
                  "chunk_rows negative or not a multiple of 128", "NaN results with CUGP_OK",
                  "Not built: gradients with respect to Z", "one all-reduce", "FITC", "multi-target",
                  "a C++ mirror in cugp_amd/host/"):
        assert words in text, words
    assert re.search(r"#define CUGP_SPARSE_MAX_M 32768\b", header())


def refused(rc, call):
    return rc == INV and call.encode() in capi.lib().cugp_last_error()


def test_create_refusals_come_before_the_device():
    """Every bad argument of cugp_sparse_create is CUGP_ERR_INVALID whether or not a device is visible; out stays NULL."""
    L = capi.lib()
    h = _vp()
    good = dict(n=100, m=10, d=2, device=0, kernel=0, ard=0, jitter=1e-6, chunk_rows=0)
    for bad in (dict(n=0), dict(d=0), dict(m=0), dict(m=-3), dict(m=32769), dict(kernel=3), dict(kernel=-1),
                dict(chunk_rows=100), dict(chunk_rows=-128), dict(chunk_rows=129), dict(jitter=0.0), dict(jitter=-1e-6),
                dict(jitter=float("nan")), dict(jitter=float("inf"))):
        a = dict(good, **bad)
        rc = L.cugp_sparse_create(a["n"], a["m"], a["d"], a["device"], a["kernel"], a["ard"], a["jitter"], a["chunk_rows"],
                                  C.byref(h))
        assert refused(rc, "cugp_sparse_create"), bad
        assert not h.value
    assert refused(L.cugp_sparse_create(100, 10, 2, 0, 0, 0, 1e-6, 0, None), "cugp_sparse_create")


def test_null_handles_and_plan_arguments():
    L = capi.lib()
    out = np.zeros(8)
    F, ne, iv = C.c_double(7.0), C.c_int(7), (C.c_int * 5)(*([7] * 5))
    assert refused(L.cugp_sparse_dims(None, None, None, None, None, None), "cugp_sparse_dims")
    assert refused(L.cugp_sparse_num_hyper(None, C.byref(ne)), "cugp_sparse_num_hyper")
    assert refused(L.cugp_sparse_set_data(None, capi.ptr(out), capi.ptr(out)), "cugp_sparse_set_data")
    assert refused(L.cugp_sparse_set_inducing(None, capi.ptr(out)), "cugp_sparse_set_inducing")
    assert refused(L.cugp_sparse_set_loghyper(None, capi.ptr(out), 3), "cugp_sparse_set_loghyper")
    assert refused(L.cugp_sparse_get_loghyper(None, capi.ptr(out), 3), "cugp_sparse_get_loghyper")
    assert refused(L.cugp_sparse_bound(None, C.byref(F)), "cugp_sparse_bound")
    assert refused(L.cugp_sparse_bound_grad(None, C.byref(F), capi.ptr(out), 3), "cugp_sparse_bound_grad")
    assert refused(L.cugp_sparse_predict(None, capi.ptr(out), 1, 1, capi.ptr(out), capi.ptr(out)), "cugp_sparse_predict")
    assert refused(L.cugp_sparse_cg_solve(None, 5, None, 0, C.byref(ne)), "cugp_sparse_cg_solve")
    assert L.cugp_sparse_destroy(None) == capi.CUGP_OK
    for n, m, chunk, p in ((0, 10, 0, 0), (100, 0, 0, 0), (100, 32769, 0, 0), (100, 10, 100, 0), (100, 10, -128, 0),
                           (100, 10, 0, -1), (100, 10, 0, 1), (300, 10, 128, 3)):
        assert refused(L.cugp_sparse_plan(n, m, chunk, p, iv), "cugp_sparse_plan"), (n, m, chunk, p)
    assert refused(L.cugp_sparse_plan(100, 10, 0, 0, None), "cugp_sparse_plan")
    assert (F.value, ne.value) == (7.0, 7) and not out.any() and list(iv) == [7] * 5
    assert L.cugp_sparse_plan(300, 10, 128, 2, iv) == 3 and list(iv) == [256, 44, 128, 1, 128]


def test_predict_plan_refusals():
    """cugp_sparse_plan's conventions: CUGP_ERR_INVALID with the call's name, out untouched, no device looked for."""
    L = capi.lib()
    iv = (C.c_int * 2)(7, 7)
    for m, nt, p in ((0, 10, 0), (-1, 10, 0), (32769, 10, 0), (16, 0, 0), (16, -5, 0), (16, 10, -1), (16, 10, 1),
                     (16, 349440, 1), (16, 349441, 2), (32768, 5000, 4)):
        assert refused(L.cugp_sparse_predict_plan(m, nt, p, iv), "cugp_sparse_predict_plan"), (m, nt, p)
    assert refused(L.cugp_sparse_predict_plan(16, 10, 0, None), "cugp_sparse_predict_plan")
    assert list(iv) == [7, 7]
    assert L.cugp_sparse_predict_plan(16, 349441, 1, iv) == 2 and list(iv) == [349440, 1]
    assert L.cugp_sparse_predict_plan(32768, 2 ** 31 - 1, 0, iv) == -(-(2 ** 31 - 1) // 1280) and list(iv) == [0, 1280]


@pytest.mark.parametrize("m, nt", [(16, 20), (16, 349569), (2048, 1000000), (32768, 5000)])
def test_predict_plan_covers_every_test_row_once(m, nt):
    """Every test row lies in exactly one pass, the passes ascend, no pass but the last is ragged, and a pass is the rule's:
    whole 128-row tiles whose three [rows][mpad] matrices of doubles stay within 1 GiB, at most 2^20 rows."""
    passes = gp.sparse_predict_plan(m, nt)
    mpad = -(-m // 128) * 128
    full = max(128, min((1 << 30) // (3 * mpad * 8) // 128 * 128, 1 << 20))
    assert len(passes) == -(-nt // full)
    nxt = 0
    for i, (r0, cnt) in enumerate(passes):
        assert r0 == nxt and cnt > 0
        assert cnt == full if i < len(passes) - 1 else cnt <= full
        assert r0 % 128 == 0 and 3 * (-(-cnt // 128) * 128) * mpad * 8 <= 1 << 30
        nxt = r0 + cnt
    assert nxt == nt
    first = {(16, 20): (1, 20), (16, 349569): (2, 349440), (2048, 1000000): (46, 21760), (32768, 5000): (4, 1280)}[m, nt]
    assert (len(passes), passes[0][1]) == first


def test_no_device_is_never_a_handle():
    L = capi.lib()
    cnt = C.c_int()
    if L.cugp_device_count(C.byref(cnt)) == capi.CUGP_OK and cnt.value > 0:
        return
    h = _vp()
    assert L.cugp_sparse_create(100, 10, 2, 0, 0, 0, 1e-6, 0, C.byref(h)) == capi.CUGP_ERR_NODEVICE
    assert not h.value
    with pytest.raises(capi.CugpError):
        gp.SparseGP(100, 10, 2)


class _Lib:
    """Records the calls in place of the library (no device): what SparseGP hands over."""

    def __init__(self):
        self.calls = []

    def cugp_sparse_create(self, n, m, d, device, kind, ard, jitter, chunk, out):
        self.calls.append(("create", n, m, d, device, kind, ard, jitter, chunk))
        out._obj.value = 0x10
        return 0

    def cugp_sparse_destroy(self, h):
        self.calls.append(("destroy",))
        return 0

    def cugp_sparse_set_data(self, h, X, y):
        self.calls.append(("set_data", X[0], y[0]))
        return 0

    def cugp_sparse_set_inducing(self, h, Z):
        self.calls.append(("set_inducing", Z[0]))
        return 0

    def cugp_sparse_set_loghyper(self, h, hp, nh):
        self.calls.append(("set_loghyper", [hp[i] for i in range(nh)]))
        return 0

    def cugp_sparse_get_loghyper(self, h, hp, nh):
        for i in range(nh):
            hp[i] = 0.5 + i
        return 0

    def cugp_sparse_bound(self, h, F):
        F._obj.value = -3.5
        return 0

    def cugp_sparse_bound_grad(self, h, F, g, nh):
        self.calls.append(("bound_grad", nh))
        F._obj.value = -3.5
        for i in range(nh):
            g[i] = 1.0 + i
        return 0

    def cugp_sparse_predict(self, h, Xt, nt, with_noise, m, v):
        self.calls.append(("predict", nt, with_noise))
        m[0], v[0] = 1.0, 2.0
        return 0

    def cugp_sparse_cg_solve(self, h, budget, tr, cap, ne):
        self.calls.append(("cg_solve", budget, cap))
        ne._obj.value = 5
        for k in range(2 * (self.nh + 1)):
            tr[k] = float(k)
        return 0

    def cugp_sparse_plan(self, n, m, chunk, p, out):
        out[0], out[1], out[2], out[3], out[4] = p * 128, 128, 128, 1, 128
        return 2

    def cugp_sparse_predict_plan(self, m, nt, p, out):
        self.calls.append(("predict_plan", m, nt, p))
        out[0], out[1] = p * 256, min(256, nt - p * 256)
        return -(-nt // 256)


@pytest.mark.parametrize("kernel, ard, nh, kind", [("se", False, 3, 0), ("se", True, 6, 0), ("matern52_ard", False, 6, 2),
                                                   ("matern32", False, 3, 1)])
def test_sparsegp_plumbing(monkeypatch, kernel, ard, nh, kind):
    fake = _Lib()
    fake.nh = nh
    monkeypatch.setattr(capi, "lib", lambda: fake)
    X, y = np.arange(40.0).reshape(10, 4), np.arange(10.0)
    s = gp.SparseGP.from_subset(X, y, 3, seed=1, kernel=kernel, ard=ard, jitter=1e-5, chunk_rows=256)
    assert (s.n, s.m, s.d, s.nh) == (10, 3, 4, nh)
    assert fake.calls[0] == ("create", 10, 3, 4, 0, kind, 1 if nh == 6 else 0, 1e-5, 256)
    assert fake.calls[1] == ("set_data", 0.0, 0.0) and fake.calls[2][0] == "set_inducing"
    rows = np.sort(np.random.default_rng(1).choice(10, 3, replace=False))
    assert fake.calls[2][1] == X[rows[0], 0]
    s.set_loghyperparam(np.arange(nh) * 0.5)
    assert fake.calls[-1] == ("set_loghyper", list(np.arange(nh) * 0.5))
    with pytest.raises(ValueError):
        s.set_loghyperparam(np.zeros(nh + 1))
    with pytest.raises(ValueError):
        s.set_inducing(np.zeros((4, 4)))
    assert list(s.get_loghyperparam()) == [0.5 + i for i in range(nh)]
    assert s.bound() == -3.5
    F, g = s.bound_grad()
    assert F == -3.5 and g.shape == (nh,) and g[-1] == nh
    m, v = s.predict(np.zeros((7, 4)), with_noise=False)
    assert m.shape == v.shape == (7,) and (m[0], v[0]) == (1.0, 2.0) and fake.calls[-1] == ("predict", 7, 0)
    assert s.cg_solve(budget=7).shape == (2, nh + 1) and fake.calls[-1] == ("cg_solve", 7, 36)
    assert s.plan() == [(0, 128, 128, 1, 128), (128, 128, 128, 1, 128)]
    assert s.predict_plan(600) == [(0, 256), (256, 256), (512, 88)] and fake.calls[-1] == ("predict_plan", 3, 600, 2)
    s.close()
    assert fake.calls[-1] == ("destroy",)


BASE = ["--numchunks", "1", "--rows", "100", "--inputs", "x", "--labels", "y"]


def test_train_inducing(monkeypatch, capsys):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    parse = lambda argv: train.main(argv, parse_only=True)     # noqa: E731
    assert parse(BASE).inducing == 0                            # the default stays: the exact model
    a = parse(BASE + ["--inducing", "32", "--kernel", "matern52_ard"])
    assert (a.inducing, a.kernel, a.objective) == (32, "matern52_ard", "ll")
    for bad in (BASE + ["--inducing", "101"], BASE + ["--inducing", "-1"], BASE + ["--inducing", "8", "--objective", "loo"],
                ["--numchunks", "4"] + BASE[2:] + ["--inducing", "8"]):
        with pytest.raises(SystemExit):
            parse(bad)
    assert "the sparse model is built for a single model over all rows" in capsys.readouterr().err
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        parse(BASE + ["--inducing", "8"])
