"""The surface of the batched and sharded input gradients of a product of experts, no GPU: header, ctypes binding and built
library agree on the three new symbols; the header documents the rows layout and the refusals; every refusal that all
ranks detect from the shared arguments comes back as CUGP_ERR_INVALID, with the call's name in cugp_last_error, before any
collective or device call -- so on a machine without a GPU."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import cugp_amd.gp as gp
from cugp_amd import capi
from cugp_amd.bcm import ShardedBCM
from cugp_amd.capi import ptr
from conftest import ROOT

HEADER = open(os.path.join(ROOT, "include", "cugp.h")).read()


@pytest.mark.parametrize("name,nargs", [("cugp_bcm_predict_grad", 9), ("cugp_bcm_predict_grad_form", 2),
                                        ("cugp_bcm_predict_grad_allgather", 15)])
def test_symbols_declared_bound_and_exported(name, nargs):
    m = re.search(r"\bint %s\s*\(([^;]*)\)\s*;" % name, HEADER)
    assert m, name
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert len([a for a in args.split(",") if a.strip()]) == nargs
    assert name in capi.SIGNATURES
    assert len(capi.SIGNATURES[name][1]) == nargs
    assert hasattr(capi.lib(), name)


def test_header_signature_of_the_form_across_ranks():
    m = re.search(r"\bint cugp_bcm_predict_grad_allgather\s*\(([^;]*)\)\s*;", HEADER)
    args = " ".join(re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split()).replace(" ,", ",")
    assert args == ("cugp_bcm *b, cugp_comm *c, int per, int nexperts, const double *Xt, int nt, int d, int mode, "
                    "int with_noise, double sf2, double sn2, double *mean, double *var, double *dmean, double *dvar")
    assert re.search(r"\bint cugp_bcm_predict_grad_form\s*\(\s*const cugp_bcm \*b,\s*int \*form\s*\)", HEADER)
    sig = capi.SIGNATURES["cugp_bcm_predict_grad_allgather"][1]
    assert sig[:2] == [C.c_void_p, C.c_void_p] and sig[9:11] == [C.c_double, C.c_double]
    assert [sig[i] for i in (2, 3, 5, 6, 7, 8)] == [C.c_int] * 6


def test_header_documents_rows_and_refusals():
    text = " ".join(re.sub(r"^ \*", "", HEADER, flags=re.M).split())     # (the comment blocks' leading " *" removed)
    for phrase in ("[m nt | v nt | dmean nt*d | dvar nt*d]", "(2 + 2 d) nt doubles",
                   "{status, local expert count, [per] slots of (2 + 2 d) nt doubles",
                   "[mean nt | var nt | dmean nt*d | dvar nt*d | world x {status, count}]",
                   "NULL c or Xt; nt, d, per or nexperts <= 0; per * world < nexperts; an unknown mode; dmean and dvar both "
                   "NULL; d different from a non-NULL b's",
                   "0 no call yet, 1 expert by expert, 2 every device set as a group",
                   "all four outputs NaN", "A world of one without an id uses no RCCL"):
        assert phrase in text, phrase
    # the two "Not built" lines no longer list what this adds
    assert "a batched launch for the experts of a BCM. */" not in HEADER
    assert "Not built: the form across ranks" not in HEADER


def test_python_surface():
    p = inspect.signature(gp.Comm.predict_grad_allgather).parameters
    assert list(p)[1:] == ["bcm", "per", "nexperts", "Xt", "d", "combine", "with_noise", "sf2", "sn2", "want_var_grad"]
    assert p["combine"].default is None and p["with_noise"].default is True and p["want_var_grad"].default is True
    p = inspect.signature(ShardedBCM.predict_grad).parameters
    assert list(p)[1:] == ["Xt", "combine", "with_noise"]
    assert p["combine"].default is None and p["with_noise"].default is True
    assert isinstance(gp.BCM.predict_grad_form, property)


def test_form_query_on_null():
    lib = capi.lib()
    f = C.c_int(7)
    assert lib.cugp_bcm_predict_grad_form(None, C.byref(f)) == capi.CUGP_ERR_INVALID
    assert b"cugp_bcm_predict_grad_form" in lib.cugp_last_error()
    assert f.value == 7


@pytest.fixture(scope="module")
def comm():
    """A world of one without an id: no RCCL, and creating it touches no device."""
    c = gp.Comm(None, 0, 1, 0)
    yield c
    c.close()


def test_refusals_before_any_collective_or_device_call(comm):
    """Every refusal of the shared arguments that can be provoked without a cugp_bcm.  The one left out -- d different from
    a non-NULL b's -- needs a BCM handle, and cugp_bcm_create_* creates the experts' handles on their device, so it cannot
    be made on a machine without a GPU: tests/test_gpu_bcm_predict_grad_batched.py::test_status_protocol_then_recovery
    holds that refusal (outputs untouched, the call's name in cugp_last_error)."""
    lib = capi.lib()
    nt, d = 3, 2
    Xt = np.zeros((nt, d))
    m, v, dm, dv = np.empty(nt), np.empty(nt), np.empty((nt, d)), np.empty((nt, d))

    def call(c=comm._h, per=1, nexperts=1, xt=ptr(Xt), nt=nt, d=d, mode=0, dm_=ptr(dm), dv_=ptr(dv), b=None):
        lib.cugp_bcm_predict_grad_form(None, None)        # (leaves another call's name in cugp_last_error)
        rc = lib.cugp_bcm_predict_grad_allgather(b, c, per, nexperts, xt, nt, d, mode, 1, 1.0, 0.1, ptr(m), ptr(v), dm_, dv_)
        return rc, lib.cugp_last_error()
    cases = [dict(c=None), dict(xt=None), dict(nt=0), dict(nt=-2), dict(d=0), dict(d=-1), dict(per=0), dict(per=-1),
             dict(nexperts=0), dict(nexperts=-3), dict(per=1, nexperts=2), dict(per=2, nexperts=3), dict(mode=-2),
             dict(mode=4), dict(mode=99), dict(dm_=None, dv_=None)]
    for kw in cases:
        m[:], dm[:] = 5.0, 5.0
        rc, err = call(**kw)
        assert rc == capi.CUGP_ERR_INVALID, kw
        assert b"cugp_bcm_predict_grad_allgather" in err, (kw, err)
        assert np.all(m == 5.0) and np.all(dm == 5.0)     # a refusal touches no output


def test_unknown_combine_raises_before_any_library_call():
    c = gp.Comm.__new__(gp.Comm)                          # no handle at all: the name is checked first
    c._h = None
    with pytest.raises(ValueError):
        c.predict_grad_allgather(None, 1, 1, np.zeros((1, 2)), 2, combine="robust")
    with pytest.raises(ValueError):
        c.predict_grad_allgather(None, 1, 1, np.zeros((1, 2)), 2, combine="poe")     # no BCM and no sf2 / sn2
