"""The leave-one-out interface without a GPU: the three entry points are exported and bound with the header's signatures, the
header says what is and is not built, every argument error comes back as CUGP_ERR_INVALID with the call's name before any
device call (a null or a dummy handle is never dereferenced), good arguments without a device give CUGP_ERR_NODEVICE, never
a value, and the keyword plumbing of Covsum and of train.py --objective is in place."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cugp_amd.gp as gp
from conftest import ROOT
from cugp_amd import capi, train

_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
NEW = {"cugp_loo": [C.c_void_p, _dp, _dp, C.c_int],
       "cugp_loo_predict": [C.c_void_p, _dp, _dp, _dp],
       "cugp_cg_solve_loo": [C.c_void_p, C.c_int, _dp, C.c_int, _ip]}
DECLS = {"cugp_loo": "cugp_gp *gp, double *lpl, double *g, int nh",
         "cugp_loo_predict": "cugp_gp *gp, double *mean, double *var, double *logp",
         "cugp_cg_solve_loo": "cugp_gp *gp, int budget, double *trace, int trace_cap, int *nevals"}
INV = capi.CUGP_ERR_INVALID
DUMMY = C.c_void_p(0x1000)     # never dereferenced: the checks come first


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


def test_header_says_what_is_and_is_not_built():
    text = " ".join(re.sub(r"\n\s*\*(?!/)", " ", header()).split())      # (comment lines joined, their leading stars dropped)
    for words in ("leave-one-out cross-validation", "mu_i = y_i - alpha_i / kappa_i", "noise included",
                  "allocates no N^2 scratch", "CUGP_ERR_NOMEM", "nh must equal cugp_num_hyper",
                  "Not built: LOO over the m targets of cugp_set_targets", "a batched or sharded LOO for a product of experts",
                  "a C++ Covsum method in cugp_amd/host/", "14 = k_loo_product"):
        assert words in text, words


def refused(rc, call):
    return rc == INV and call.encode() in capi.lib().cugp_last_error()


@pytest.mark.parametrize("handle", [None, DUMMY], ids=["null", "dummy"])
def test_argument_errors(handle):
    L = capi.lib()
    out = np.zeros(64)
    lpl, ne = C.c_double(7.0), C.c_int(7)
    # a null handle, whatever else is given
    assert refused(L.cugp_loo(None, C.byref(lpl), capi.ptr(out), 3), "cugp_loo")
    assert refused(L.cugp_loo_predict(None, capi.ptr(out), capi.ptr(out), capi.ptr(out)), "cugp_loo_predict")
    assert refused(L.cugp_cg_solve_loo(None, 5, None, 0, C.byref(ne)), "cugp_cg_solve_loo")
    # null results, an nh no handle has, a budget that is none: refused before the handle is looked at
    assert refused(L.cugp_loo(handle, None, capi.ptr(out), 3), "cugp_loo")
    for nh in (2, 0, -1):
        assert refused(L.cugp_loo(handle, C.byref(lpl), capi.ptr(out), nh), "cugp_loo")
        assert refused(L.cugp_loo(handle, C.byref(lpl), None, nh), "cugp_loo")
    assert refused(L.cugp_loo_predict(handle, None, capi.ptr(out), None), "cugp_loo_predict")
    assert refused(L.cugp_loo_predict(handle, capi.ptr(out), None, None), "cugp_loo_predict")
    for budget in (0, -3):
        assert refused(L.cugp_cg_solve_loo(handle, budget, None, 0, C.byref(ne)), "cugp_cg_solve_loo")
    assert (lpl.value, ne.value) == (7.0, 7) and not out.any()


def test_no_device_is_never_a_value():
    """Good arguments in a process without a GPU: CUGP_ERR_NODEVICE before the (dummy) handle is looked at.  Where a
    device is visible the same calls would go on to the handle, so they are only made without one."""
    L = capi.lib()
    cnt = C.c_int()
    if L.cugp_device_count(C.byref(cnt)) == capi.CUGP_OK and cnt.value > 0:
        return
    NODEV = capi.CUGP_ERR_NODEVICE
    out = np.zeros(64)
    lpl, ne = C.c_double(7.0), C.c_int(7)
    assert L.cugp_loo(DUMMY, C.byref(lpl), capi.ptr(out), 3) == NODEV
    assert L.cugp_loo(DUMMY, C.byref(lpl), None, 3) == NODEV
    assert L.cugp_loo_predict(DUMMY, capi.ptr(out), capi.ptr(out), None) == NODEV
    assert L.cugp_cg_solve_loo(DUMMY, 5, None, 0, C.byref(ne)) == NODEV
    assert (lpl.value, ne.value) == (7.0, 7) and not out.any()


class _Lib:
    """Records the three calls in place of the library (no device): what Covsum hands over."""

    def __init__(self):
        self.calls = []

    def cugp_loo(self, h, lpl, g, nh):
        self.calls.append(("cugp_loo", g is not None, nh))
        lpl._obj.value = -3.5
        if g is not None:
            for i in range(nh):
                g[i] = 1.0 + i
        return 0

    def cugp_loo_predict(self, h, m, v, lp):
        self.calls.append(("cugp_loo_predict", lp is not None))
        m[0], v[0], lp[0] = 1.0, 2.0, 3.0
        return 0

    def cugp_cg_solve_loo(self, h, budget, tr, cap, ne):
        self.calls.append(("cugp_cg_solve_loo", budget, cap))
        ne._obj.value = 5                                    # five evaluations, two iterates; the rest stays NaN
        for k in range(2 * (self.nh + 1)):
            tr[k] = float(k)
        return 0


@pytest.mark.parametrize("nh, d, ard", [(3, 4, False), (6, 4, True)])
def test_covsum_plumbing(monkeypatch, nh, d, ard):
    fake = _Lib()
    fake.nh = nh
    monkeypatch.setattr(capi, "lib", lambda: fake)
    g = gp.Covsum.__new__(gp.Covsum)
    g.n, g.d, g.nh, g.ard, g._h = 5, d, nh, ard, C.c_void_p()
    lpl, gr = g.loo()
    assert lpl == -3.5 and gr.shape == (nh,) and gr[-1] == nh
    assert g.loo(want_grad=False) == (-3.5, None)
    m, v, lp = g.loo_predict()
    assert m.shape == v.shape == lp.shape == (5,) and (m[0], v[0], lp[0]) == (1.0, 2.0, 3.0)
    tr = g.cg_solve_loo(budget=7)
    assert tr.shape == (2, nh + 1)
    assert g.cg_solve_loo().shape == (2, nh + 1)
    assert fake.calls == [("cugp_loo", True, nh), ("cugp_loo", False, nh), ("cugp_loo_predict", True),
                          ("cugp_cg_solve_loo", 7, 36), ("cugp_cg_solve_loo", 100, 408)]
    g._h = None                                             # (nothing to destroy)


BASE = ["--numchunks", "1", "--rows", "10", "--inputs", "x", "--labels", "y"]


def parse(argv):
    return train.main(argv, parse_only=True)


def test_train_objective(monkeypatch, capsys):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    assert parse(BASE).objective == "ll"                       # the default stays
    assert parse(BASE + ["--objective", "ll"]).objective == "ll"
    a = parse(BASE + ["--objective", "loo", "--kernel", "matern52_ard"])
    assert (a.objective, a.kernel, a.budget) == ("loo", "matern52_ard", 100)
    for bad in (BASE + ["--objective", "cv"], ["--numchunks", "4"] + BASE[2:] + ["--objective", "loo"]):
        with pytest.raises(SystemExit):
            parse(bad)
    assert "leave-one-out is built for a single expert" in capsys.readouterr().err
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        parse(BASE + ["--objective", "loo"])
    assert parse(["--numchunks", "4"] + BASE[2:]).objective == "ll"     # (several experts: as before)


def test_iterate_record_is_the_same_loop():
    """cugp_cg_solve_loo's loop (minimize.cpp: cugp_cg_minimize_n_iterates, internal) against cugp_cg_minimize_n on a host
    objective with a narrow curved valley: the same end point and evaluation count to the bit, and its record is the
    start and a subsequence of the evaluations along which the objective never rises, ending at the end point."""
    L = capi.lib()
    fn = L.cugp_cg_minimize_n_iterates
    fn.restype = C.c_int
    fn.argtypes = [capi.OBJECTIVE_N, C.c_void_p, _dp, C.c_int, C.c_int, _dp, C.c_int, _ip, _ip]

    @capi.OBJECTIVE_N
    def rosen(_ctx, th, nh, f, g):
        x = [th[i] for i in range(nh)]
        f[0] = sum(100.0 * (x[i + 1] - x[i] ** 2) ** 2 + (1 - x[i]) ** 2 for i in range(nh - 1))
        for i in range(nh):
            g[i] = 0.0
        for i in range(nh - 1):
            g[i] += -400.0 * x[i] * (x[i + 1] - x[i] ** 2) - 2 * (1 - x[i])
            g[i + 1] += 200.0 * (x[i + 1] - x[i] ** 2)
    nh, budget = 4, 40
    start = np.array([-1.2, 1.0, -0.5, 0.8])
    a, b = start.copy(), start.copy()
    full, rows = np.full((200, nh + 1), np.nan), np.full((200, nh + 1), np.nan)
    na, nb, nr = C.c_int(), C.c_int(), C.c_int()
    assert L.cugp_cg_minimize_n(rosen, None, capi.ptr(a), nh, budget, capi.ptr(full), 200, C.byref(na)) == 0
    assert fn(rosen, None, capi.ptr(b), nh, budget, capi.ptr(rows), 200, C.byref(nb), C.byref(nr)) == 0
    assert na.value == nb.value and np.array_equal(a.view(np.uint64), b.view(np.uint64))
    k = nr.value
    assert 2 <= k <= na.value and np.all(np.isnan(rows[k:]))
    it, ev = rows[:k], full[: na.value]
    assert np.array_equal(it[0], ev[0]) and np.array_equal(it[-1, :-1], b)
    assert np.any(ev[1:, -1] > ev[:-1, -1])                  # (the evaluations do rise: probes that were rejected)
    assert np.all(it[1:, -1] < it[:-1, -1])
    pos = 0
    for r in it:                                             # a subsequence of the evaluations, in order
        while not np.array_equal(ev[pos].view(np.uint64), r.view(np.uint64)):
            pos += 1
            assert pos < len(ev)
