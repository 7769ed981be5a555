"""The inducing-input gradient's interface without a GPU: the three entry points are exported and bound with the header's
signatures, the header states the formula and what is still not built, a null handle is refused as CUGP_ERR_INVALID with the
call's name before any device call and nothing is written, without a device no handle exists to call them on
(CUGP_ERR_NODEVICE from cugp_sparse_create), and the plumbing of SparseGP and of train.py --learn-inducing is in place."""
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
    "cugp_sparse_bound_grad_z": [_vp, _dp, _dp, C.c_int, _dp],
    "cugp_sparse_get_inducing": [_vp, _dp],
    "cugp_sparse_cg_solve_z": [_vp, C.c_int, _dp, C.c_int, _ip],
}
DECLS = {
    "cugp_sparse_bound_grad_z": "cugp_sparse *sp, double *F, double *g, int nh, double *gZ",
    "cugp_sparse_get_inducing": "const cugp_sparse *sp, double *Z",
    "cugp_sparse_cg_solve_z": "cugp_sparse *sp, int budget, double *trace, int trace_cap, int *nevals",
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


def test_header_states_the_formula_and_what_is_not_built():
    text = " ".join(re.sub(r"\n\s*\*(?!/)", " ", header()).split())
    for words in ("dk(z_j, x) / dz_jc = -H(z_j, x) (z_jc - x_c) s_c",
                  "dF/dz_jc = -s_c sum_i G_uf[j,i] H(z_j,x_i) (z_jc - x_ic) - s_c sum_b (2 G_uu)[j,b] H(z_j,z_b) (z_jc - z_bc)",
                  "Matern 3/2: 3 sf2 e^-a", "Matern 5/2: (5/3) sf2 (1 + a) e^-a", "s_c = 1 / l^2 (ARD: w_c^2)",
                  "weight 1 here, not the 1/2 of the trace", "the jitter have no derivative", "no N M^2 product is added",
                  "*F and g carry ITS bits", "in cugp_sparse_set_inducing's layout", "[theta, vec Z]",
                  "CUGP_ERR_NOMEM when the partial blocks of the Z pass cannot be allocated: the handle stays as it was",
                  "Not built: gradients with respect to Z of the predictions", "FITC", "multi-target"):
        assert words in text, words
    assert "given by the caller and fixed" not in text


def refused(rc, call):
    return rc == INV and call.encode() in capi.lib().cugp_last_error()


def test_null_arguments_are_refused_before_the_device():
    L = capi.lib()
    out, F, ne = np.zeros(8), C.c_double(7.0), C.c_int(7)
    assert refused(L.cugp_sparse_bound_grad_z(None, C.byref(F), capi.ptr(out), 3, capi.ptr(out)), "cugp_sparse_bound_grad_z")
    assert refused(L.cugp_sparse_get_inducing(None, capi.ptr(out)), "cugp_sparse_get_inducing")
    assert refused(L.cugp_sparse_cg_solve_z(None, 5, None, 0, C.byref(ne)), "cugp_sparse_cg_solve_z")
    assert refused(L.cugp_sparse_cg_solve_z(None, 0, capi.ptr(out), 1, C.byref(ne)), "cugp_sparse_cg_solve_z")
    assert (F.value, ne.value) == (7.0, 7) and not out.any()


def test_no_device_is_never_a_handle_to_call_them_on():
    L = capi.lib()
    cnt = C.c_int()
    if L.cugp_device_count(C.byref(cnt)) == capi.CUGP_OK and cnt.value > 0:
        return
    h = _vp()
    assert L.cugp_sparse_create(100, 10, 2, 0, 0, 0, 1e-6, 0, C.byref(h)) == capi.CUGP_ERR_NODEVICE and not h.value


class _Lib:
    """Records the calls in place of the library (no device): what SparseGP hands over."""

    def __init__(self, nh):
        self.calls, self.nh = [], nh

    def cugp_sparse_create(self, n, m, d, device, kind, ard, jitter, chunk, out):
        out._obj.value = 0x10
        return 0

    def cugp_sparse_destroy(self, h):
        return 0

    def cugp_sparse_bound_grad_z(self, h, F, g, nh, gZ):
        self.calls.append(("bound_grad_z", nh))
        F._obj.value = -2.5
        for i in range(nh):
            g[i] = 1.0 + i
        for i in range(3 * 4):
            gZ[i] = 10.0 + i
        return 0

    def cugp_sparse_get_inducing(self, h, Z):
        self.calls.append(("get_inducing",))
        for i in range(3 * 4):
            Z[i] = 0.5 * i
        return 0

    def _solve(self, which, budget, tr, cap, ne):
        self.calls.append((which, budget, cap))
        ne._obj.value = 5
        for k in range(2 * (self.nh + 1)):
            tr[k] = float(k)
        return 0

    def cugp_sparse_cg_solve(self, h, budget, tr, cap, ne):
        return self._solve("cg_solve", budget, tr, cap, ne)

    def cugp_sparse_cg_solve_z(self, h, budget, tr, cap, ne):
        return self._solve("cg_solve_z", budget, tr, cap, ne)


@pytest.mark.parametrize("ard, nh", [(False, 3), (True, 6)])
def test_sparsegp_plumbing(monkeypatch, ard, nh):
    fake = _Lib(nh)
    monkeypatch.setattr(capi, "lib", lambda: fake)
    s = gp.SparseGP(10, 3, 4, ard=ard)
    F, g, gZ = s.bound_grad_z()
    assert F == -2.5 and g.shape == (nh,) and g[-1] == nh and fake.calls[-1] == ("bound_grad_z", nh)
    assert gZ.shape == (3, 4) and gZ[0, 0] == 10.0 and gZ[2, 3] == 21.0          # [m][d], set_inducing's layout
    Z = s.get_inducing()
    assert Z.shape == (3, 4) and Z[1, 0] == 2.0 and fake.calls[-1] == ("get_inducing",)
    assert s.cg_solve(budget=7).shape == (2, nh + 1) and fake.calls[-1] == ("cg_solve", 7, 36)      # the default: today's path
    assert s.cg_solve(budget=7, inducing=False).shape == (2, nh + 1) and fake.calls[-1] == ("cg_solve", 7, 36)
    assert s.cg_solve(budget=7, inducing=True).shape == (2, nh + 1) and fake.calls[-1] == ("cg_solve_z", 7, 36)
    s.close()


BASE = ["--numchunks", "1", "--rows", "100", "--inputs", "x", "--labels", "y"]


def test_train_learn_inducing(monkeypatch, capsys):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    parse = lambda argv: train.main(argv, parse_only=True)     # noqa: E731
    assert parse(BASE).learn_inducing is False
    assert parse(BASE + ["--inducing", "32"]).learn_inducing is False            # the default stays: Z fixed
    a = parse(BASE + ["--inducing", "32", "--learn-inducing", "--kernel", "matern52_ard"])
    assert (a.inducing, a.learn_inducing, a.kernel) == (32, True, "matern52_ard")
    with pytest.raises(SystemExit):
        parse(BASE + ["--learn-inducing"])
    assert "--learn-inducing needs --inducing M" in capsys.readouterr().err


def test_train_hands_the_flag_to_cg_solve(monkeypatch):
    import inspect
    src = inspect.getsource(train.train_sparse)
    assert "cg_solve(args.budget, inducing=args.learn_inducing)" in src
