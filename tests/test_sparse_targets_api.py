"""The interface of multi-target regression over one set of inducing points without a GPU: the seven entry points are exported
and bound with the header's signatures, the header states the model, the conventions and the refusals, a null handle or
argument is refused as CUGP_ERR_INVALID with the call's name before any device call and nothing is written, without a device
no handle exists to call them on (CUGP_ERR_NODEVICE from cugp_sparse_create), and the plumbing of SparseGP is in place: the
shapes, and the target-major hand-over of a [n, p] array."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cugp_amd.gp as gp
from conftest import ROOT
from cugp_amd import capi

_dp, _ip, _vp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_void_p
NEW = {
    "cugp_sparse_set_targets": [_vp, _dp, C.c_int],
    "cugp_sparse_num_targets": [_vp, _ip],
    "cugp_sparse_bound_targets": [_vp, _dp, _dp],
    "cugp_sparse_bound_grad_targets": [_vp, _dp, _dp, C.c_int, _dp],
    "cugp_sparse_bound_grad_z_targets": [_vp, _dp, _dp, C.c_int, _dp, _dp],
    "cugp_sparse_predict_targets": [_vp, _dp, C.c_int, C.c_int, _dp, _dp],
    "cugp_sparse_cg_solve_targets": [_vp, C.c_int, C.c_int, _dp, C.c_int, _ip],
}
DECLS = {
    "cugp_sparse_set_targets": "cugp_sparse *sp, const double *Y, int p",
    "cugp_sparse_num_targets": "const cugp_sparse *sp, int *p",
    "cugp_sparse_bound_targets": "cugp_sparse *sp, double *F, double *F_each",
    "cugp_sparse_bound_grad_targets": "cugp_sparse *sp, double *F, double *g, int nh, double *F_each",
    "cugp_sparse_bound_grad_z_targets": "cugp_sparse *sp, double *F, double *g, int nh, double *gZ, double *F_each",
    "cugp_sparse_predict_targets": "cugp_sparse *sp, const double *Xt, int nt, int with_noise, double *mean, double *var",
    "cugp_sparse_cg_solve_targets": "cugp_sparse *sp, int budget, int inducing, double *trace, int trace_cap, int *nevals",
}
INV = capi.CUGP_ERR_INVALID


def header():
    with open(os.path.join(ROOT, "include", "cugp.h")) as f:
        return f.read()


@pytest.mark.parametrize("name", sorted(NEW))
def test_exported_and_bound(name):
    assert name in capi.SIGNATURES
    res, args = capi.SIGNATURES[name]
    assert res is C.c_int and args == NEW[name] and len(args) == len(DECLS[name].split(","))
    fn = getattr(capi.lib(), name)
    assert fn.restype is C.c_int and list(fn.argtypes) == NEW[name]


@pytest.mark.parametrize("name", sorted(NEW))
def test_header_declares_the_signature(name):
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, text)
    assert decl, name
    assert " ".join(decl.group(1).split()).replace(" ,", ",") == DECLS[name]


def test_header_states_the_model_the_conventions_and_the_refusals():
    text = " ".join(re.sub(r"\n\s*\*(?!/)", " ", header()).split())
    for words in ("multi-target regression over one set of inducing points", "F = sum_t F_t",
                  "F_t = ((((-N/2 log 2 pi - sum log LB_ii) - N/2 log s2) - y_t'y_t / (2 s2)) + c'_t'c'_t / (2 s2^2)) - (N sf2 - tr P) / (2 s2)",
                  "summed in target order", "H = p (I - B^-1) - sum_t gamma'_t gamma'_t' / s2^2", "H2 = H - p P / s2",
                  "G_c' = W_c R' + sum_t y_t,c (beta'_t / s2^2)'", "the rank-one part becomes rank p",
                  "g_f = -(2 (S_uf,nl + S_uu,nl / 2) - p N sf2 / s2)",
                  "g_n = -(((p sum_i (1 - [B^-1]_ii) - p N) + (((sum_t y_t'y_t - sum_t c'_t'c'_t / s2) + p (N sf2 - tr P)) / s2)) "
                  "- sum_t gamma'_t'gamma'_t / s2^2)",
                  "mean_t = Vt c'_t / s2", "the variance does not depend on y", "runs ONCE for all targets",
                  "Y [p][n] target-major", "cugp_sparse_set_data is still required", "its y is unrelated to the targets",
                  "Targets persist until replaced", "a second call may change p", "p has no cap other than memory",
                  "0 before cugp_sparse_set_targets", "F_each (may be NULL)", "mean [p][nt] target-major and var [nt] (may be NULL)",
                  "var has the bits of cugp_sparse_predict", "it reads nothing of y",
                  "cugp_sparse_cg_solve (inducing == 0) or cugp_sparse_cg_solve_z (inducing != 0)",
                  "The single-target calls are untouched, in bits and in launches",
                  "it makes the single-target results stale and the reverse",
                  "cugp_sparse_set_loghyper, _set_inducing, _set_data and _set_targets make the targets' results stale",
                  "a NULL handle, Y or F", "p < 1", "cugp_sparse_set_targets before cugp_sparse_set_data",
                  "any targets call before cugp_sparse_set_targets or cugp_sparse_set_inducing", "an nh that is not the handle's",
                  "a NULL Xt, mean, g or gZ where one is required", "NaN results with CUGP_OK",
                  "per-target hyper-parameters", "leave-one-out over targets"):
        assert words in text, words
    # the sparse model's "Not built" list no longer names what this adds
    not_built = re.search(r"Not built: gradients with respect to Z of the predictions.*?cugp_amd/host/\.", text).group(0)
    assert "multi-target" not in not_built and "FITC" in not_built


def refused(rc, call):
    return rc == INV and call.encode() in capi.lib().cugp_last_error()


def test_null_arguments_are_refused_before_the_device():
    L = capi.lib()
    out, F, ne, p = np.zeros(8), C.c_double(7.0), C.c_int(7), C.c_int(7)
    P = capi.ptr
    assert refused(L.cugp_sparse_set_targets(None, P(out), 2), "cugp_sparse_set_targets")
    assert refused(L.cugp_sparse_set_targets(None, None, 2), "cugp_sparse_set_targets")
    assert refused(L.cugp_sparse_set_targets(None, P(out), 0), "cugp_sparse_set_targets")
    assert refused(L.cugp_sparse_num_targets(None, C.byref(p)), "cugp_sparse_num_targets")
    assert refused(L.cugp_sparse_bound_targets(None, C.byref(F), P(out)), "cugp_sparse_bound_targets")
    assert refused(L.cugp_sparse_bound_grad_targets(None, C.byref(F), P(out), 3, P(out)), "cugp_sparse_bound_grad_targets")
    assert refused(L.cugp_sparse_bound_grad_z_targets(None, C.byref(F), P(out), 3, P(out), P(out)),
                   "cugp_sparse_bound_grad_z_targets")
    assert refused(L.cugp_sparse_predict_targets(None, P(out), 1, 1, P(out), P(out)), "cugp_sparse_predict_targets")
    assert refused(L.cugp_sparse_cg_solve_targets(None, 5, 0, None, 0, C.byref(ne)), "cugp_sparse_cg_solve_targets")
    assert refused(L.cugp_sparse_cg_solve_targets(None, 5, 1, P(out), 1, C.byref(ne)), "cugp_sparse_cg_solve_targets")
    assert (F.value, ne.value, p.value) == (7.0, 7, 7) and not out.any()


def test_no_device_is_never_a_handle_to_call_them_on():
    L = capi.lib()
    cnt = C.c_int()
    if L.cugp_device_count(C.byref(cnt)) == capi.CUGP_OK and cnt.value > 0:
        return
    h = _vp()
    assert L.cugp_sparse_create(100, 10, 2, 0, 0, 0, 1e-6, 0, C.byref(h)) == capi.CUGP_ERR_NODEVICE and not h.value


class _Lib:
    """Records the calls in place of the library (no device): what SparseGP hands over."""
    N, M, D, P = 10, 3, 4, 5

    def __init__(self, nh):
        self.calls, self.nh, self.Y = [], nh, None

    def cugp_sparse_create(self, n, m, d, device, kind, ard, jitter, chunk, out):
        out._obj.value = 0x10
        return 0

    def cugp_sparse_destroy(self, h):
        return 0

    def cugp_sparse_set_targets(self, h, Y, p):
        self.calls.append(("set_targets", p))
        self.Y = np.array([Y[i] for i in range(p * self.N)]).reshape(p, self.N)
        return 0

    def cugp_sparse_num_targets(self, h, p):
        p._obj.value = self.P
        return 0

    def _row(self, F, g, nh, each):
        F._obj.value = -2.5
        if g is not None:
            for i in range(nh):
                g[i] = 1.0 + i
        for t in range(self.P):
            each[t] = 100.0 + t

    def cugp_sparse_bound_targets(self, h, F, each):
        self.calls.append(("bound_targets",))
        self._row(F, None, 0, each)
        return 0

    def cugp_sparse_bound_grad_targets(self, h, F, g, nh, each):
        self.calls.append(("bound_grad_targets", nh))
        self._row(F, g, nh, each)
        return 0

    def cugp_sparse_bound_grad_z_targets(self, h, F, g, nh, gZ, each):
        self.calls.append(("bound_grad_z_targets", nh))
        self._row(F, g, nh, each)
        for i in range(self.M * self.D):
            gZ[i] = 10.0 + i
        return 0

    def cugp_sparse_predict_targets(self, h, Xt, nt, with_noise, mean, var):
        self.calls.append(("predict_targets", nt, with_noise))
        for i in range(self.P * nt):
            mean[i] = float(i)
        for i in range(nt):
            var[i] = 0.5 + i
        return 0

    def cugp_sparse_cg_solve_targets(self, h, budget, inducing, tr, cap, ne):
        self.calls.append(("cg_solve_targets", budget, inducing, cap))
        ne._obj.value = 5
        for k in range(2 * (self.nh + 1)):
            tr[k] = float(k)
        return 0


@pytest.mark.parametrize("ard, nh", [(False, 3), (True, 6)])
def test_sparsegp_plumbing(monkeypatch, ard, nh):
    fake = _Lib(nh)
    monkeypatch.setattr(capi, "lib", lambda: fake)
    s = gp.SparseGP(_Lib.N, _Lib.M, _Lib.D, ard=ard)
    Y = np.arange(_Lib.N * _Lib.P, dtype=np.float64).reshape(_Lib.N, _Lib.P)          # [n, p]: one column per target
    s.set_targets(Y)
    assert fake.calls[-1] == ("set_targets", _Lib.P) and np.array_equal(fake.Y, Y.T)    # handed over target-major
    s.set_targets(np.asfortranarray(Y))
    assert np.array_equal(fake.Y, Y.T)
    for bad in (np.zeros(_Lib.N), np.zeros((_Lib.N + 1, 2)), np.zeros((_Lib.N, 0)), np.zeros((2, _Lib.N))):
        with pytest.raises(ValueError):
            s.set_targets(bad)
    assert s.num_targets == _Lib.P
    F, each = s.bound_targets()
    assert F == -2.5 and each.shape == (_Lib.P,) and each[-1] == 104.0 and fake.calls[-1] == ("bound_targets",)
    F, g, each = s.bound_grad_targets()
    assert F == -2.5 and g.shape == (nh,) and g[-1] == nh and each.shape == (_Lib.P,) and fake.calls[-1] == ("bound_grad_targets", nh)
    F, g, gZ, each = s.bound_grad_z_targets()
    assert g.shape == (nh,) and gZ.shape == (_Lib.M, _Lib.D) and gZ[2, 3] == 21.0 and each[0] == 100.0
    assert fake.calls[-1] == ("bound_grad_z_targets", nh)
    m, v = s.predict_targets(np.zeros((7, _Lib.D)))
    assert m.shape == (_Lib.P, 7) and v.shape == (7,) and m[1, 0] == 7.0 and fake.calls[-1] == ("predict_targets", 7, 1)
    s.predict_targets(np.zeros((2, _Lib.D)), with_noise=False)
    assert fake.calls[-1] == ("predict_targets", 2, 0)
    assert s.cg_solve_targets(budget=7).shape == (2, nh + 1) and fake.calls[-1] == ("cg_solve_targets", 7, 0, 36)
    assert s.cg_solve_targets(budget=7, inducing=True).shape == (2, nh + 1) and fake.calls[-1] == ("cg_solve_targets", 7, 1, 36)
    s.close()


def test_the_build_knows_every_header_the_sources_include():
    """An edit of a header that build.HEADERS does not list would leave a stale library in place (the build id is a hash
    over the listed files): every local header a source or a listed header includes is listed."""
    from cugp_amd import build
    listed = set(build.HEADERS)
    assert "sparse_targets_device.h" in listed
    for f in build.SOURCES + build.HEADERS:
        with open(os.path.join(build.CSRC, f)) as fh:
            for inc in re.findall(r'^#include "([^"/]+)"', fh.read(), flags=re.M):
                assert inc in listed, (f, inc)


def test_the_build_lists_every_source_file():
    """A file of csrc/ that build.SOURCES + build.HEADERS leaves out is not compiled or not hashed: an edit of it would
    leave a stale library in place."""
    from cugp_amd import build
    listed = set(build.SOURCES + build.HEADERS)
    assert len(listed) == len(build.SOURCES + build.HEADERS)
    on_disk = {f for f in os.listdir(build.CSRC) if f.endswith((".cpp", ".hip", ".h"))}
    assert on_disk == listed, (sorted(on_disk - listed), sorted(listed - on_disk))
