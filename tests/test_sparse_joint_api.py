"""The interface of the sparse model's joint covariance, draws and input gradients without a GPU: the four entry points are
exported and bound with the header's signatures, the header states the model, the conventions and the refusals, a null
handle or argument is refused as CUGP_ERR_INVALID with the call's name before any device call and nothing is written, and
the plumbing of SparseGP is in place: shapes, flags, the default jitter rule and the normals handed over."""
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
    "cugp_sparse_predict_cov_plan": [C.c_int, C.c_int, _ip],
    "cugp_sparse_predict_cov": [_vp, _dp, C.c_int, C.c_int, _dp, _dp],
    "cugp_sparse_predict_sample": [_vp, _dp, C.c_int, C.c_int, C.c_double, C.c_int, _dp, _dp],
    "cugp_sparse_predict_grad": [_vp, _dp, C.c_int, C.c_int, _dp, _dp, _dp, _dp],
}
DECLS = {
    "cugp_sparse_predict_cov_plan": "int m, int nt, int out[4]",
    "cugp_sparse_predict_cov": "cugp_sparse *sp, const double *Xt, int nt, int with_noise, double *mean, double *cov",
    "cugp_sparse_predict_sample": "cugp_sparse *sp, const double *Xt, int nt, int with_noise, double jitter, int nsamples, "
                                  "const double *normals, double *samples",
    "cugp_sparse_predict_grad": "cugp_sparse *sp, const double *Xt, int nt, int with_noise, double *mean, double *var, "
                                "double *dmean, double *dvar",
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
    for words in ("joint predictive covariance, posterior draws and input gradients of the sparse model",
                  "cov = k(Xt,Xt) - Wt Wt^T + Vt Vt^T (+ s2 I with noise)", "the lower triangle mirrored: exactly symmetric",
                  "not bit for bit (the summation orders differ)", "nothing of it is added to cov",
                  "samples[s nt + t] = mean[t] + sum_{k <= t} C[t][k] normals[s nt + k]", "C = chol(cov + jitter I)",
                  "the normals are the caller's", "that is not positive definite gives NaN with CUGP_OK",
                  "dk(x*, z_j) / dx*_c = -G_j (x*_c - z_jc) s_c", "exactly as stated above cugp_predict_grad",
                  "a = beta' / s2", "U = (Wt - Vt LB^-1) Lu^-1", "var_f = sf2 - ks_t^T U_t",
                  "dmean / dx*_c = -s_c sum_j a_j G_j (x*_c - z_jc)", "dvar / dx*_c = +2 s_c sum_j U_tj G_j (x*_c - z_jc)",
                  "The noisy and the latent variance have the same gradient", "pure arithmetic, no device",
                  "at the process's current tuning", "nt > CUGP_SPARSE_MAX_M", "Wt and Vt must be whole",
                  "Both refuse exactly where the plan does", "a NULL dvar skips U and its two triangular products",
                  "cugp_sparse_predict's bits for the same with_noise", "any nt", "evaluate first when it is stale",
                  "a targets evaluation in between", "a jitter that is negative or not finite", "nsamples <= 0",
                  "dmean and dvar both NULL"):
        assert words in text, words
    # the two "Not built" lists: what this adds is no longer missing, what it leaves out is named
    not_built = re.search(r"Not built: gradients with respect to Z of the predictions.*?cugp_amd/host/\.", text).group(0)
    assert "gradients of the joint covariance or of draws" in not_built and "FITC" in not_built
    tg = re.search(r"Not built for the targets:.*?already\)\.", text).group(0)
    assert "input gradients and draws per target" in tg and "the joint covariance reads no y" in tg


def refused(rc, call):
    return rc == INV and call.encode() in capi.lib().cugp_last_error()


def test_null_arguments_are_refused_before_the_device():
    L, P = capi.lib(), capi.ptr
    out = np.zeros(16)
    assert refused(L.cugp_sparse_predict_cov(None, P(out), 2, 1, P(out), P(out)), "cugp_sparse_predict_cov")
    assert refused(L.cugp_sparse_predict_sample(None, P(out), 2, 1, 0.0, 2, P(out), P(out)), "cugp_sparse_predict_sample")
    assert refused(L.cugp_sparse_predict_grad(None, P(out), 2, 1, P(out), P(out), P(out), P(out)), "cugp_sparse_predict_grad")
    assert refused(L.cugp_sparse_predict_cov_plan(10, 10, None), "cugp_sparse_predict_cov_plan")
    assert not out.any()
    plan = (C.c_int * 4)()
    assert L.cugp_sparse_predict_cov_plan(65, 129, plan) == capi.CUGP_OK and plan[0] == 256 and plan[1] in (64, 128)
    assert gp.sparse_predict_cov_plan(65, 129) == tuple(plan)
    with pytest.raises(Exception):
        gp.sparse_predict_cov_plan(65, 32769)


class _Lib:
    """Records the calls in place of the library (no device): what SparseGP hands over."""
    N, M, D = 10, 3, 4

    def __init__(self):
        self.calls, self.normals, self.hp = [], None, np.array([0.3, 0.5, -1.0])

    def cugp_sparse_create(self, n, m, d, device, kind, ard, jitter, chunk, out):
        out._obj.value = 0x10
        return 0

    def cugp_sparse_destroy(self, h):
        return 0

    def cugp_sparse_get_loghyper(self, h, hp, nh):
        for i in range(nh):
            hp[i] = self.hp[i]
        return 0

    def cugp_sparse_predict_cov(self, h, Xt, nt, with_noise, mean, cov):
        self.calls.append(("cov", nt, with_noise))
        for i in range(nt):
            mean[i] = float(i)
        for i in range(nt * nt):
            cov[i] = 100.0 + i
        return 0

    def cugp_sparse_predict_sample(self, h, Xt, nt, with_noise, jitter, ns, normals, samples):
        self.calls.append(("sample", nt, with_noise, jitter, ns))
        self.normals = np.array([normals[i] for i in range(ns * nt)]).reshape(ns, nt)
        for i in range(ns * nt):
            samples[i] = float(i)
        return 0

    def cugp_sparse_predict_grad(self, h, Xt, nt, with_noise, mean, var, dmean, dvar):
        self.calls.append(("grad", nt, with_noise, dvar is not None))
        for i in range(nt):
            mean[i], var[i] = float(i), 0.5 + i
        for i in range(nt * self.D):
            dmean[i] = 10.0 + i
            if dvar is not None:
                dvar[i] = 20.0 + i
        return 0

    def cugp_sparse_predict_cov_plan(self, m, nt, out):
        self.calls.append(("plan", m, nt))
        out[0], out[1], out[2], out[3] = 256, 64, 2, 256
        return 0


def test_sparsegp_plumbing(monkeypatch):
    fake = _Lib()
    monkeypatch.setattr(capi, "lib", lambda: fake)
    s = gp.SparseGP(_Lib.N, _Lib.M, _Lib.D)
    Xt = np.zeros((5, _Lib.D))
    m, cov = s.predict_joint(Xt)
    assert m.shape == (5,) and cov.shape == (5, 5) and cov[1, 0] == 105.0 and fake.calls[-1] == ("cov", 5, 1)
    s.predict_joint(Xt, with_noise=False)
    assert fake.calls[-1] == ("cov", 5, 0)
    m, v, dm, dv = s.predict_grad(Xt)
    assert m.shape == v.shape == (5,) and dm.shape == dv.shape == (5, _Lib.D) and dm[1, 0] == 14.0 and dv[0, 1] == 21.0
    assert fake.calls[-1] == ("grad", 5, 1, True)
    m, v, dm, dv = s.predict_grad(Xt, with_noise=False, want_var_grad=False)
    assert dv is None and dm.shape == (5, _Lib.D) and fake.calls[-1] == ("grad", 5, 0, False)
    # draws: latent by default with jitter 1e-8 sf2; with noise 0; a given jitter as given; the normals as given or from rng
    z = np.arange(15, dtype=np.float64).reshape(3, 5)
    out = s.sample_posterior(Xt, 3, normals=z)
    assert out.shape == (3, 5) and out[1, 0] == 5.0 and np.array_equal(fake.normals, z)
    assert fake.calls[-1] == ("sample", 5, 0, 1e-8 * float(np.exp(2.0 * 0.5)), 3)
    s.sample_posterior(Xt, 3, with_noise=True, normals=z)
    assert fake.calls[-1] == ("sample", 5, 1, 0.0, 3)
    s.sample_posterior(Xt, 2, jitter=0.25, rng=7)
    assert fake.calls[-1] == ("sample", 5, 0, 0.25, 2)
    assert np.array_equal(fake.normals, np.random.default_rng(7).standard_normal((2, 5)))
    s.sample_posterior(Xt, 2, jitter=0.25, rng=np.random.default_rng(9))
    assert np.array_equal(fake.normals, np.random.default_rng(9).standard_normal((2, 5)))
    assert s.predict_cov_plan(129) == (256, 64, 2, 256) and fake.calls[-1] == ("plan", _Lib.M, 129)
    s.close()


def test_the_build_knows_the_new_header():
    from cugp_amd import build
    assert "sparse_predict_device.h" in build.HEADERS
    with open(os.path.join(build.CSRC, "kernels.hip")) as f:
        assert '#include "sparse_predict_device.h"' in f.read()
