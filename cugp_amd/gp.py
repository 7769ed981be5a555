"""Python mirror of the reference's host interface over the C-ABI.

`Covsum` keeps the method names and argument meaning of the reference class
(cpp_serial_gp/covkernel.h:20-37); `BCM` those of distributed_gp/BCM.h:15-26.  Every method is a
thin call into libcugp.so -- no arithmetic happens in Python.
"""
import ctypes as C
import math

import numpy as np

from . import capi
from .capi import check, f64, ptr


KERNELS = {"se": capi.CUGP_KERNEL_SE, "matern32": capi.CUGP_KERNEL_MATERN32, "matern52": capi.CUGP_KERNEL_MATERN52}
KERNEL_NAMES = {v: k for k, v in KERNELS.items()}
# one length scale per input dimension with a Matern kind (GPML covMaternard): the name sets ard=True by itself
ARD_KERNELS = {"matern32_ard": capi.CUGP_KERNEL_MATERN32, "matern52_ard": capi.CUGP_KERNEL_MATERN52}
# rational quadratic (GPML covRQiso / covRQard; cugp_create_rq): the name -> one length scale per dimension?  Both forms
# carry the shape parameter alpha in front of sigma_f, sigma_n and use the nh-wide (_ard) calls; the number 3 is not a kernel=
RQ_KERNELS = {"rq": False, "rq_ard": True}
REPORTED_NAMES = dict(KERNEL_NAMES)
REPORTED_NAMES[capi.CUGP_KERNEL_RQ] = "rq"


def num_hyper(kind, ard, d):
    """entries of the log-hyper-parameter vector: length scales (1, ARD d), the family's shape parameters (RQ: alpha),
    sigma_f, sigma_n"""
    return (int(d) if ard else 1) + (1 if kind == capi.CUGP_KERNEL_RQ else 0) + 2


def is_wide(kind, ard):
    """the handle takes the nh-wide (_ard) calls: ARD, or rational quadratic in either form"""
    return bool(ard) or kind == capi.CUGP_KERNEL_RQ


COMBINE = {"poe": capi.CUGP_COMBINE_POE, "gpoe": capi.CUGP_COMBINE_GPOE, "bcm": capi.CUGP_COMBINE_BCM,
           "rbcm": capi.CUGP_COMBINE_RBCM}


def combine_mode(combine):
    """"poe" | "gpoe" | "bcm" | "rbcm" -> the C ABI's CUGP_COMBINE_* number; anything else raises ValueError (before any
    library call)."""
    if not isinstance(combine, str) or combine.lower() not in COMBINE:
        raise ValueError("combine must be None or one of %s, not %r" % (sorted(COMBINE), combine))
    return COMBINE[combine.lower()]


def prior_scalars(hp):
    """(sf2, sn2) = (exp(2 theta_f), exp(2 theta_n)) from a log-hyper vector, by the C library's exp -- the bits the
    library's own kernels are given (numpy's exp may round differently)."""
    return math.exp(float(hp[-2]) * 2), math.exp(float(hp[-1]) * 2)


def kernel_kind(kernel):
    """"se" | "matern32" | "matern52" (or the C ABI's CUGP_KERNEL_* number) -> the number."""
    if isinstance(kernel, str):
        if kernel.lower() not in KERNELS:
            raise ValueError("kernel must be one of %s, not %r" % (sorted(KERNELS), kernel))
        return KERNELS[kernel.lower()]
    if int(kernel) not in KERNEL_NAMES:
        raise ValueError("unknown kernel kind %r" % (kernel,))
    return int(kernel)


def kernel_spec(kernel, ard=False):
    """(kind, ard) of a kernel= / ard= pair: the isotropic names with ard as given (ard=True is squared-exponential
    only), or one of ARD_KERNELS' names, which are ARD whatever `ard` says."""
    if isinstance(kernel, str) and kernel.lower() in ARD_KERNELS:
        return ARD_KERNELS[kernel.lower()], True
    if isinstance(kernel, str) and kernel.lower() in RQ_KERNELS:
        if ard and not RQ_KERNELS[kernel.lower()]:
            raise ValueError('ard=True is squared-exponential only; the ARD rational quadratic kernel is kernel="rq_ard"')
        return capi.CUGP_KERNEL_RQ, RQ_KERNELS[kernel.lower()]
    if isinstance(kernel, str) and kernel.lower().endswith("_ard"):
        raise ValueError("kernel must be one of %s, not %r"
                         % (sorted(KERNELS) + sorted(ARD_KERNELS) + sorted(RQ_KERNELS), kernel))
    kind = kernel_kind(kernel)
    if ard and kind != capi.CUGP_KERNEL_SE:
        raise ValueError('ard=True is squared-exponential only; the ARD Matern kernels are kernel="%s_ard"'
                         % KERNEL_NAMES[kind])
    return kind, bool(ard)


class Covsum:
    """One GP expert on one GPU.  Covsum(n, d) as covkernel.cpp:14-37; X, y are given per call as in
    the reference and uploaded whenever their CONTENTS differ from what the GPU holds (the reference
    recomputes K from the arguments on every call; comparing n*d doubles is nothing beside an O(n^3)
    evaluation, and an in-place edit of y or a recycled array address can not go unnoticed).
    ard=True: one length scale per input dimension (cugp_create_ard; GPML covSEard's order): the hyper-parameter
    vector is [log l_1 .. log l_d, log sigma_f, log sigma_n], gradients and cg_solve traces have d + 2 (+ 1) entries.
    kernel="se" | "matern32" | "matern52": the covariance family (cugp_create_kernel; GPML covMaterniso with d = 3, 5),
    same three hyper-parameters; fixed for the life of the handle.  ard=True is squared-exponential only;
    kernel="matern32_ard" | "matern52_ard" (GPML covMaternard; cugp_create_ard_kernel) is ARD with a Matern kind: .ard
    is True, nh = d + 2, and .kernel reports "matern32" / "matern52".
    kernel="rq" | "rq_ard" (rational quadratic, GPML covRQiso / covRQard; cugp_create_rq): the hyper-parameter vector is
    [log l, log alpha, log sigma_f, log sigma_n] (nh = 4, .ard False) or [log l_1 .. log l_d, log alpha, log sigma_f,
    log sigma_n] (nh = d + 3, .ard True); .kernel reports "rq".  Everything an ARD handle does works on both.
    npad_min: rows the handle has room for (capacity); append(X, y) adds observations up to it."""

    def __init__(self, n, d, device=0, npad_min=0, ard=False, kernel="se"):
        self.n, self.d, self.device = int(n), int(d), int(device)
        self._kind, self.ard = kernel_spec(kernel, ard)
        self.nh = num_hyper(self._kind, self.ard, self.d)
        self._h = C.c_void_p()
        if self._kind == capi.CUGP_KERNEL_RQ:
            check(capi.lib().cugp_create_rq(self.n, self.d, self.device, int(npad_min), 1 if self.ard else 0,
                                            C.byref(self._h)))
        elif self.ard and self._kind != capi.CUGP_KERNEL_SE:
            check(capi.lib().cugp_create_ard_kernel(self.n, self.d, self.device, int(npad_min), self._kind,
                                                    C.byref(self._h)))
        elif self._kind != capi.CUGP_KERNEL_SE:
            check(capi.lib().cugp_create_kernel(self.n, self.d, self.device, int(npad_min), self._kind,
                                                C.byref(self._h)))
        elif self.ard:
            if npad_min:
                check(capi.lib().cugp_create_ard_padded(self.n, self.d, self.device, int(npad_min), C.byref(self._h)))
            else:
                check(capi.lib().cugp_create_ard(self.n, self.d, self.device, C.byref(self._h)))
        else:
            check(capi.lib().cugp_create_padded(self.n, self.d, self.device, int(npad_min), C.byref(self._h)))
        self._data_key = None

    # -- lifetime --
    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            capi.lib().cugp_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def _wide(self):
        """takes the nh-wide (_ard) calls: ARD, or rational quadratic in either form"""
        return is_wide(self._kind, self.ard)

    @property
    def handle(self):
        return self._h

    @property
    def kernel(self):
        """The handle's covariance family as the library reports it: "se", "matern32" or "matern52"."""
        k = C.c_int()
        check(capi.lib().cugp_kernel_kind(self._h, C.byref(k)))
        return REPORTED_NAMES[k.value]

    # -- data --
    def set_data(self, X, y):
        X, y = f64(X), f64(y)
        if X.shape != (self.n, self.d) or y.shape != (self.n,):
            raise ValueError("expected X %s and y %s" % ((self.n, self.d), (self.n,)))
        check(capi.lib().cugp_set_data(self._h, ptr(X), ptr(y)))
        self._data_key = (X.copy(), y.copy())

    @property
    def capacity(self):
        """The rows the handle can hold (cugp_capacity): its padded size, fixed by n and npad_min when it was created."""
        c = C.c_int()
        check(capi.lib().cugp_capacity(self._h, C.byref(c)))
        return c.value

    def append(self, X, y):
        """Append observations (cugp_append): X [k, d] with y [k], or one row as a 1-d X with a scalar y.  A handle that
        holds its inverse quantities is extended in place at O(k n^2); any other handle only takes the data and the next
        evaluation factors all rows.  self.n grows by k; set_data keeps taking the current n rows."""
        X, y = np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64)
        if X.ndim == 1 and y.ndim == 0:
            X, y = X.reshape(1, -1), y.reshape(1)
        X, y = f64(X), f64(y)                                        # (contiguous; ascontiguousarray alone turns a scalar into 1-d)
        if X.ndim != 2 or X.shape[1] != self.d or y.shape != (X.shape[0],):
            raise ValueError("expected X (k, %d) with y (k,), or one row (%d,) with a scalar y" % (self.d, self.d))
        try:
            check(capi.lib().cugp_append(self._h, ptr(X), ptr(y), int(X.shape[0])))
        except capi.CugpError:
            # a refusal leaves n alone; a device error after the rows were taken leaves a stale handle of n + k rows
            # whose new rows may not have arrived: follow the library's n and forget the data key, so that the next
            # bound data is set afresh
            n, d, npad = C.c_int(), C.c_int(), C.c_int()
            if capi.lib().cugp_dims(self._h, C.byref(n), C.byref(d), C.byref(npad)) == capi.CUGP_OK and n.value != self.n:
                self.n, self._data_key = n.value, None
            raise
        self.n += int(X.shape[0])
        k = self._data_key
        self._data_key = None if k is None else (np.concatenate([k[0], X]), np.concatenate([k[1], y]))

    def set_data_device(self, dX_ptr, dy_ptr):
        check(capi.lib().cugp_set_data_device(self._h, C.c_void_p(dX_ptr), C.c_void_p(dy_ptr)))
        self._data_key = None

    def _bind(self, X, y):
        if X is None:
            return
        X = f64(X)
        y = f64(y) if y is not None else (self._data_key[1] if self._data_key is not None else np.zeros(self.n))
        k = self._data_key
        if k is None or k[0].shape != X.shape or not np.array_equal(k[0], X) or not np.array_equal(k[1], y):
            self.set_data(X, y)

    # -- hyper-parameters --
    def set_loghyperparam(self, hp):
        hp = f64(hp)
        if self._wide:
            if hp.shape != (self.nh,):
                raise ValueError("expected %d log-hyper-parameters" % self.nh)
            check(capi.lib().cugp_set_loghyper_ard(self._h, ptr(hp), self.nh))
        else:
            check(capi.lib().cugp_set_loghyper(self._h, ptr(hp)))

    set_loghyper_eigen = set_loghyperparam

    def get_loghyperparam(self):
        out = np.empty(self.nh)
        if self._wide:
            check(capi.lib().cugp_get_loghyper_ard(self._h, ptr(out), self.nh))
        else:
            check(capi.lib().cugp_get_loghyper(self._h, ptr(out)))
        return out

    def get_param_dim(self):
        return self.nh if self._wide else self.d   # covkernel.cpp:661-663 returns numdim; ARD: the number of hyper-parameters

    # -- objective --
    def compute_loglikelihood(self, X=None, y=None):
        self._bind(X, y)
        ll = C.c_double()
        check(capi.lib().cugp_loglik(self._h, C.byref(ll)))
        return ll.value

    def compute_gradient_loghyperparam(self, X=None, y=None):
        self._bind(X, y)
        if self._wide:
            return self.loglik_grad()[1]
        g = np.empty(3)
        check(capi.lib().cugp_grad(self._h, ptr(g)))
        return g

    def loglik_grad(self, X=None, y=None):
        self._bind(X, y)
        ll = C.c_double()
        g = np.empty(self.nh)
        if self._wide:
            check(capi.lib().cugp_loglik_grad_ard(self._h, C.byref(ll), ptr(g), self.nh))
        else:
            check(capi.lib().cugp_loglik_grad(self._h, C.byref(ll), ptr(g)))
        return ll.value, g

    def enqueue(self, want_grad=True):
        check(capi.lib().cugp_loglik_grad_enqueue(self._h, 1 if want_grad else 0))

    def fetch(self):
        ll = C.c_double()
        g = np.empty(self.nh)
        if self._wide:
            check(capi.lib().cugp_loglik_grad_fetch_ard(self._h, C.byref(ll), ptr(g), self.nh))
        else:
            check(capi.lib().cugp_loglik_grad_fetch(self._h, C.byref(ll), ptr(g)))
        return ll.value, g

    def last_quad_logdet(self):
        q, d = C.c_double(), C.c_double()
        check(capi.lib().cugp_last_quad_logdet(self._h, C.byref(q), C.byref(d)))
        return q.value, d.value

    # -- intermediates --
    def compute_K_train(self, X=None):
        """Covsum::compute_K_train(X, out): the full symmetric n x n covariance (labels are not used)."""
        self._bind(X, None)
        K = np.empty((self.n, self.n))
        check(capi.lib().cugp_compute_K_train(self._h, ptr(K)))
        return K

    def compute_squared_dist(self, c):
        S = np.empty((self.n, self.n))
        check(capi.lib().cugp_compute_squared_dist(self._h, float(c), ptr(S)))
        return S

    def compute_k_test(self, Xt):
        Xt = f64(Xt).reshape(-1, self.d)
        Ks = np.empty((Xt.shape[0], self.n))
        check(capi.lib().cugp_compute_k_test(self._h, ptr(Xt), Xt.shape[0], ptr(Ks)))
        return Ks

    def get_cholesky(self):
        L = np.empty((self.n, self.n))
        check(capi.lib().cugp_get_cholesky(self._h, ptr(L)))
        return L

    def get_K_inverse(self):
        Ki = np.empty((self.n, self.n))
        check(capi.lib().cugp_get_K_inverse(self._h, ptr(Ki)))
        return Ki

    def get_alpha(self):
        a = np.empty(self.n)
        check(capi.lib().cugp_get_alpha(self._h, ptr(a)))
        return a

    # -- multi-target regression: m target vectors over the same X and hyper-parameters, one factorisation --
    def set_targets(self, Y):
        """Y [n, m], one column per target (cugp_set_targets; handed over target-major).  set_data is still required:
        it supplies X, and its y is unrelated to the targets."""
        Y = f64(Y)
        if Y.ndim != 2 or Y.shape[0] != self.n or Y.shape[1] < 1:
            raise ValueError("expected Y of shape (%d, m), m >= 1" % self.n)
        Yt = f64(Y.T)
        check(capi.lib().cugp_set_targets(self._h, ptr(Yt), Yt.shape[0]))

    @property
    def num_targets(self):
        m = C.c_int()
        check(capi.lib().cugp_num_targets(self._h, C.byref(m)))
        return m.value

    def loglik_grad_targets(self):
        """(LL = sum_t LL_t, gradient of -LL [nh], LL_t [m]) from one factorisation (cugp_loglik_grad_targets)."""
        ll = C.c_double()
        g, each = np.empty(self.nh), np.empty(self.num_targets)
        check(capi.lib().cugp_loglik_grad_targets(self._h, C.byref(ll), ptr(g), self.nh, ptr(each)))
        return ll.value, g, each

    def predict_targets(self, Xtest):
        """(mean [nt, m], var [nt]) at the test points; the variance is compute_test_means_and_variances' own."""
        Xt = f64(Xtest).reshape(-1, self.d)
        nt = Xt.shape[0]
        mean, var = np.empty((self.num_targets, nt)), np.empty(nt)
        check(capi.lib().cugp_predict_targets(self._h, ptr(Xt), nt, ptr(mean), ptr(var)))
        return f64(mean.T), var

    def get_alpha_targets(self):
        """K^-1 Y, [n, m]."""
        a = np.empty((self.num_targets, self.n))
        check(capi.lib().cugp_get_alpha_targets(self._h, ptr(a)))
        return f64(a.T)

    def cg_solve_targets(self, budget=100):
        """Conjugate gradients on -sum_t LL_t (cugp_cg_solve_targets); the trace [n_evals, nh + 1] = (theta, -LL)."""
        tr = np.zeros((4 * budget + 8, self.nh + 1))
        ne = C.c_int()
        check(capi.lib().cugp_cg_solve_targets(self._h, budget, ptr(tr), tr.shape[0], C.byref(ne)))
        return tr[: ne.value]

    # -- leave-one-out cross-validation from the factored model (GPML 5.10-5.13), on the data the handle holds --
    def loo(self, want_grad=True):
        """(L_LOO, g): the sum of the leave-one-out log predictive densities and the gradient of -L_LOO [nh] in
        loglik_grad's convention and order (cugp_loo); want_grad=False: (L_LOO, None), no N^2 scratch."""
        lpl = C.c_double()
        g = np.empty(self.nh) if want_grad else None
        check(capi.lib().cugp_loo(self._h, C.byref(lpl), ptr(g) if want_grad else None, self.nh))
        return lpl.value, g

    def loo_predict(self):
        """(mean, var, logp), n each: every training row predicted from the other n - 1 (cugp_loo_predict); var is the
        variance of y_i, noise included; logp sums to loo()'s L_LOO."""
        m, v, lp = np.empty(self.n), np.empty(self.n), np.empty(self.n)
        check(capi.lib().cugp_loo_predict(self._h, ptr(m), ptr(v), ptr(lp)))
        return m, v, lp

    def cg_solve_loo(self, budget=100):
        """Conjugate gradients on -L_LOO from the current hyper-parameters (cugp_cg_solve_loo), every family; the trace
        [n_iterates, nh + 1] = (theta, -L_LOO) of the start and of the point every line search ended at: the objective
        never rises along it, and the last row is the end point (rejected probes are not recorded)."""
        budget = int(budget)
        tr = np.full((4 * max(budget, 0) + 8, self.nh + 1), np.nan)
        ne = C.c_int()
        check(capi.lib().cugp_cg_solve_loo(self._h, budget, ptr(tr), tr.shape[0], C.byref(ne)))
        rows = 1
        while rows < min(ne.value, tr.shape[0]) and not np.isnan(tr[rows, 0]):
            rows += 1
        return tr[:rows]

    # -- prediction --
    def compute_test_means_and_variances(self, X, y, Xtest):
        self._bind(X, y)
        Xt = f64(Xtest).reshape(-1, self.d)
        m, v = np.empty(Xt.shape[0]), np.empty(Xt.shape[0])
        check(capi.lib().cugp_predict(self._h, ptr(Xt), Xt.shape[0], ptr(m), ptr(v)))
        return m, v

    def predict_latent(self, Xtest):
        """The latent function at the test points (cugp_predict_latent), on the data the handle holds: (mean, var_f) --
        cugp_predict's mean bit for bit, var_f = sf2 - |W_t|^2 without the noise term."""
        Xt = f64(Xtest).reshape(-1, self.d)
        m, v = np.empty(Xt.shape[0]), np.empty(Xt.shape[0])
        check(capi.lib().cugp_predict_latent(self._h, ptr(Xt), Xt.shape[0], ptr(m), ptr(v)))
        return m, v

    def predict_grad(self, Xtest, with_noise=True, want_var_grad=True):
        """Mean, variance and their gradients with respect to the test inputs (cugp_predict_grad), on the data the handle
        holds: (mean [nt], var [nt], dmean [nt, d], dvar [nt, d] or None).  mean / var carry the bits of
        compute_test_means_and_variances (with_noise) or predict_latent; want_var_grad=False skips the second triangular
        product and returns None for dvar."""
        Xt = f64(Xtest).reshape(-1, self.d)
        nt = Xt.shape[0]
        m, v, dm = np.empty(nt), np.empty(nt), np.empty((nt, self.d))
        dv = np.empty((nt, self.d)) if want_var_grad else None
        check(capi.lib().cugp_predict_grad(self._h, ptr(Xt), nt, 1 if with_noise else 0, ptr(m), ptr(v), ptr(dm),
                                           ptr(dv) if want_var_grad else None))
        return m, v, dm, dv

    def compute_test_joint(self, X, y, Xtest, with_noise=True):
        """Joint predictive distribution at the test points (cugp_predict_cov): (mean [nt], cov [nt, nt]), cov =
        k(Xt,Xt) - Ks K^-1 Ks^T (+ sigma_n^2 I with noise), exactly symmetric; mean has cugp_predict's bits."""
        self._bind(X, y)
        Xt = f64(Xtest).reshape(-1, self.d)
        nt = Xt.shape[0]
        m, cov = np.empty(nt), np.empty((nt, nt))
        check(capi.lib().cugp_predict_cov(self._h, ptr(Xt), nt, 1 if with_noise else 0, ptr(m), ptr(cov)))
        return m, cov

    def sample_posterior(self, X, y, Xtest, nsamples, with_noise=False, jitter=None, rng=None, normals=None):
        """Posterior draws at the test points (cugp_predict_sample): [nsamples, nt] = mean + normals C^T, C the lower
        Cholesky factor of cov + jitter I (cov as compute_test_joint).  normals [nsamples, nt] default to
        rng.standard_normal (rng: a numpy Generator or a seed); jitter None: 1e-8 sf2 for latent draws, 0 with noise."""
        self._bind(X, y)
        Xt = f64(Xtest).reshape(-1, self.d)
        nt, ns = Xt.shape[0], int(nsamples)
        if normals is None:
            gen = rng if isinstance(rng, np.random.Generator) else np.random.default_rng(rng)
            normals = gen.standard_normal((ns, nt))
        Z = f64(normals).reshape(ns, nt)
        if jitter is None:
            jitter = 0.0 if with_noise else 1e-8 * float(np.exp(2.0 * self.get_loghyperparam()[-2]))
        out = np.empty((ns, nt))
        check(capi.lib().cugp_predict_sample(self._h, ptr(Xt), nt, 1 if with_noise else 0, float(jitter), ns, ptr(Z),
                                             ptr(out)))
        return out

    @staticmethod
    def get_negative_log_predprob(actual, predmean, predvar):
        a, m, v = f64(actual), f64(predmean), f64(predvar)
        out = C.c_double()
        check(capi.lib().cugp_nlpp(ptr(a), ptr(m), ptr(v), a.shape[0], C.byref(out)))
        return out.value

    # -- optimisers --
    def cg_solve(self, X=None, y=None, budget=100):
        """Covsum::cg_solve; returns the evaluation trace [n_evals, 4] = (hp0, hp1, hp2, -LL); ARD: [n_evals, d + 3]."""
        self._bind(X, y)
        tr = np.zeros((4 * budget + 8, self.nh + 1))
        ne = C.c_int()
        solve = capi.lib().cugp_cg_solve_ard if self._wide else capi.lib().cugp_cg_solve
        check(solve(self._h, budget, ptr(tr), tr.shape[0], C.byref(ne)))
        return tr[: ne.value]

    def cg_solve_sparing(self, X=None, y=None, budget=100):
        """Opt-in: the same line search, but the gradient (two thirds of an evaluation) only where the search reads
        it.  -> (trace, gradient evaluations made)."""
        self._bind(X, y)
        tr = np.zeros((4 * budget + 8, 4))
        ne, ng = C.c_int(), C.c_int()
        check(capi.lib().cugp_cg_solve_sparing(self._h, budget, ptr(tr), tr.shape[0], C.byref(ne), C.byref(ng)))
        return tr[: ne.value], ng.value

    def rprop_solve(self, X=None, y=None, iters=100):
        self._bind(X, y)
        tr = np.zeros((2 * iters + 8, 4))
        ne = C.c_int()
        check(capi.lib().cugp_rprop_solve(self._h, iters, ptr(tr), tr.shape[0], C.byref(ne)))
        return tr[: ne.value]

    # -- timing --
    def set_profiling(self, level):
        check(capi.lib().cugp_set_profiling(self._h, int(level)))

    def set_overlap(self, enable):
        """Inverse blocks on further streams while the factorisation runs (default on; cugp_set_overlap)."""
        check(capi.lib().cugp_set_overlap(self._h, 1 if enable else 0))

    def set_tuning(self, key, value, own=True):
        """One launch-shape key (kernels.h TUNE_*) for THIS handle alone (cugp_set_handle_tuning); own=False hands the
        key back to the process default (cugp_set_tuning)."""
        check(capi.lib().cugp_set_handle_tuning(self._h, int(key), int(value), 1 if own else 0))

    def get_tuning(self, key):
        v = C.c_int()
        check(capi.lib().cugp_get_handle_tuning(self._h, int(key), C.byref(v)))
        return v.value

    def chain_first(self):
        """True where the handle's factorisation stream runs at the device's highest priority (cugp_chain_first)."""
        v = C.c_int()
        check(capi.lib().cugp_chain_first(self._h, C.byref(v)))
        return bool(v.value)

    def phase_ms(self):
        """Main-stream phases of the last evaluation.  With the overlap on, "potrf" includes the inverse blocks
        running beside it and "trtri" is what was left of them when the factorisation ended ("lauum" ~ 0)."""
        ms = np.empty(6)
        check(capi.lib().cugp_get_phase_ms(self._h, ptr(ms)))
        return dict(zip(("kbuild", "potrf", "trtri", "lauum", "tail", "total"), ms.tolist()))

    def kernel_stats(self, reset=False, kind=0):
        """Per-launch timings of one kernel kind (include/cugp.h: cugp_get_kernel_stats_kind); "disp_ms" (profiling
        level 5): the same launches from the end of the launch in front of each on its stream."""
        s, n, f, dms = C.c_double(), C.c_longlong(), C.c_double(), C.c_double()
        check(capi.lib().cugp_get_kernel_stats_dispatch_ms(self._h, int(kind), C.byref(dms)))
        check(capi.lib().cugp_get_kernel_stats_kind(self._h, int(kind), C.byref(s), C.byref(n), C.byref(f),
                                                    1 if reset else 0))
        return {"sum_ms": s.value, "launches": n.value, "flop": f.value, "disp_ms": dms.value}


class SparseGP:
    """Sparse variational GP regression on m inducing inputs (cugp_sparse_*; Titsias 2009): n data rows streamed in
    chunks of chunk_rows (0: the library's choice) against Z [m, d], given by the caller and fixed.  kernel / ard as
    Covsum's; the hyper-parameter vector is Covsum's ([log l, log sf, log sn], ARD [log l_1 .. log l_d, log sf, log sn]);
    jitter is the absolute eps of Kuu = k(Z, Z) + eps I.  bound() is a lower bound on the exact log marginal likelihood
    of all n rows; gradients are those of -bound, in loglik_grad's convention and order."""

    def __init__(self, n, m, d, device=0, kernel="se", ard=False, jitter=1e-6, chunk_rows=0):
        self.n, self.m, self.d, self.device = int(n), int(m), int(d), int(device)
        self._kind, self.ard = kernel_spec(kernel, ard)
        if self._kind == capi.CUGP_KERNEL_RQ:
            raise ValueError("SparseGP: the rational quadratic kernel is not built for the sparse model")
        self.nh = self.d + 2 if self.ard else 3
        self.jitter, self.chunk_rows = float(jitter), int(chunk_rows)
        self._h = C.c_void_p()
        check(capi.lib().cugp_sparse_create(self.n, self.m, self.d, self.device, self._kind, 1 if self.ard else 0,
                                            self.jitter, self.chunk_rows, C.byref(self._h)))

    @classmethod
    def from_subset(cls, X, y, m, seed=0, **kw):
        """A model over (X, y) whose inducing inputs are m rows of X drawn without replacement (numpy default_rng(seed)),
        in ascending row order; data and Z are set."""
        X, y = f64(X), f64(y)
        rows = np.sort(np.random.default_rng(seed).choice(X.shape[0], int(m), replace=False))
        s = cls(X.shape[0], int(m), X.shape[1], **kw)
        s.set_data(X, y)
        s.set_inducing(X[rows])
        return s

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            capi.lib().cugp_sparse_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def set_data(self, X, y):
        X, y = f64(X), f64(y)
        if X.shape != (self.n, self.d) or y.shape != (self.n,):
            raise ValueError("expected X %s and y %s" % ((self.n, self.d), (self.n,)))
        check(capi.lib().cugp_sparse_set_data(self._h, ptr(X), ptr(y)))

    def set_inducing(self, Z):
        Z = f64(Z)
        if Z.shape != (self.m, self.d):
            raise ValueError("expected Z %s" % ((self.m, self.d),))
        check(capi.lib().cugp_sparse_set_inducing(self._h, ptr(Z)))

    def set_loghyperparam(self, hp):
        hp = f64(hp)
        if hp.shape != (self.nh,):
            raise ValueError("expected %d log-hyper-parameters" % self.nh)
        check(capi.lib().cugp_sparse_set_loghyper(self._h, ptr(hp), self.nh))

    def get_loghyperparam(self):
        out = np.empty(self.nh)
        check(capi.lib().cugp_sparse_get_loghyper(self._h, ptr(out), self.nh))
        return out

    def bound(self):
        """F, the variational lower bound on the log marginal likelihood (cugp_sparse_bound)."""
        F = C.c_double()
        check(capi.lib().cugp_sparse_bound(self._h, C.byref(F)))
        return F.value

    def bound_grad(self):
        """(F, g): the bound and the gradient of -F [nh] (cugp_sparse_bound_grad)."""
        F, g = C.c_double(), np.empty(self.nh)
        check(capi.lib().cugp_sparse_bound_grad(self._h, C.byref(F), ptr(g), self.nh))
        return F.value, g

    def predict(self, Xtest, with_noise=True):
        """(mean, var) at the test points (cugp_sparse_predict); with_noise adds exp(2 theta_n) to the variance."""
        Xt = f64(Xtest).reshape(-1, self.d)
        m, v = np.empty(Xt.shape[0]), np.empty(Xt.shape[0])
        check(capi.lib().cugp_sparse_predict(self._h, ptr(Xt), Xt.shape[0], 1 if with_noise else 0, ptr(m), ptr(v)))
        return m, v

    def get_inducing(self):
        """Z [m, d] as the handle holds it (cugp_sparse_get_inducing): what was set, or where cg_solve(inducing=True) ended."""
        Z = np.empty((self.m, self.d))
        check(capi.lib().cugp_sparse_get_inducing(self._h, ptr(Z)))
        return Z

    def bound_grad_z(self):
        """(F, g, gZ): the bound, the gradient of -F [nh] with bound_grad's bits, and the gradient of -F with respect to
        the inducing inputs [m, d] in set_inducing's layout (cugp_sparse_bound_grad_z)."""
        F, g, gZ = C.c_double(), np.empty(self.nh), np.empty((self.m, self.d))
        check(capi.lib().cugp_sparse_bound_grad_z(self._h, C.byref(F), ptr(g), self.nh, ptr(gZ)))
        return F.value, g, gZ

    def cg_solve(self, budget=100, inducing=False):
        """Conjugate gradients on -F from the current hyper-parameters (cugp_sparse_cg_solve); the trace [n_iterates,
        nh + 1] = (theta, -F) of the start and of the point every line search ended at, as Covsum.cg_solve_loo's.
        inducing: the inducing inputs are variables too (cugp_sparse_cg_solve_z over [theta, vec Z]; the trace keeps
        (theta, -F), get_inducing() reads Z back)."""
        budget = int(budget)
        tr = np.full((4 * max(budget, 0) + 8, self.nh + 1), np.nan)
        ne = C.c_int()
        solve = capi.lib().cugp_sparse_cg_solve_z if inducing else capi.lib().cugp_sparse_cg_solve
        check(solve(self._h, budget, ptr(tr), tr.shape[0], C.byref(ne)))
        rows = 1
        while rows < min(ne.value, tr.shape[0]) and not np.isnan(tr[rows, 0]):
            rows += 1
        return tr[:rows]

    # -- multi-target regression: p target vectors over the same X, hyper-parameters and inducing inputs --
    def set_targets(self, Y):
        """Y [n, p], one column per target (cugp_sparse_set_targets; handed over target-major).  set_data is still
        required: it supplies X, and its y is unrelated to the targets."""
        Y = f64(Y)
        if Y.ndim != 2 or Y.shape[0] != self.n or Y.shape[1] < 1:
            raise ValueError("expected Y of shape (%d, p), p >= 1" % self.n)
        Yt = f64(Y.T)
        check(capi.lib().cugp_sparse_set_targets(self._h, ptr(Yt), Yt.shape[0]))

    @property
    def num_targets(self):
        p = C.c_int()
        check(capi.lib().cugp_sparse_num_targets(self._h, C.byref(p)))
        return p.value

    def bound_targets(self):
        """(F = sum_t F_t, F_t [p]) from one pass over the data (cugp_sparse_bound_targets)."""
        F, each = C.c_double(), np.empty(self.num_targets)
        check(capi.lib().cugp_sparse_bound_targets(self._h, C.byref(F), ptr(each)))
        return F.value, each

    def bound_grad_targets(self):
        """(F = sum_t F_t, gradient of -F [nh], F_t [p]) (cugp_sparse_bound_grad_targets)."""
        F, g, each = C.c_double(), np.empty(self.nh), np.empty(self.num_targets)
        check(capi.lib().cugp_sparse_bound_grad_targets(self._h, C.byref(F), ptr(g), self.nh, ptr(each)))
        return F.value, g, each

    def bound_grad_z_targets(self):
        """(F, g [nh], gZ [m, d], F_t [p]): bound_grad_targets and the gradient of -F with respect to the inducing inputs
        in set_inducing's layout (cugp_sparse_bound_grad_z_targets)."""
        F, g, gZ, each = C.c_double(), np.empty(self.nh), np.empty((self.m, self.d)), np.empty(self.num_targets)
        check(capi.lib().cugp_sparse_bound_grad_z_targets(self._h, C.byref(F), ptr(g), self.nh, ptr(gZ), ptr(each)))
        return F.value, g, gZ, each

    def predict_targets(self, Xtest, with_noise=True):
        """(mean [p, nt], var [nt]) at the test points (cugp_sparse_predict_targets); the variance is predict's own."""
        Xt = f64(Xtest).reshape(-1, self.d)
        nt = Xt.shape[0]
        mean, var = np.empty((self.num_targets, nt)), np.empty(nt)
        check(capi.lib().cugp_sparse_predict_targets(self._h, ptr(Xt), nt, 1 if with_noise else 0, ptr(mean), ptr(var)))
        return mean, var

    def cg_solve_targets(self, budget=100, inducing=False):
        """Conjugate gradients on -sum_t F_t (cugp_sparse_cg_solve_targets); the trace [n_iterates, nh + 1] = (theta, -F)
        as cg_solve's.  inducing: the inducing inputs are variables too (get_inducing() reads Z back)."""
        budget = int(budget)
        tr = np.full((4 * max(budget, 0) + 8, self.nh + 1), np.nan)
        ne = C.c_int()
        check(capi.lib().cugp_sparse_cg_solve_targets(self._h, budget, 1 if inducing else 0, ptr(tr), tr.shape[0], C.byref(ne)))
        rows = 1
        while rows < min(ne.value, tr.shape[0]) and not np.isnan(tr[rows, 0]):
            rows += 1
        return tr[:rows]

    # -- the joint distribution at test points, draws from it and gradients with respect to the test inputs --
    def predict_joint(self, Xtest, with_noise=True):
        """Joint predictive distribution at the test points (cugp_sparse_predict_cov): (mean [nt], cov [nt, nt]), cov =
        k(Xt,Xt) - Wt Wt^T + Vt Vt^T (+ exp(2 theta_n) I with noise), exactly symmetric; mean has predict's bits."""
        Xt = f64(Xtest).reshape(-1, self.d)
        nt = Xt.shape[0]
        m, cov = np.empty(nt), np.empty((nt, nt))
        check(capi.lib().cugp_sparse_predict_cov(self._h, ptr(Xt), nt, 1 if with_noise else 0, ptr(m), ptr(cov)))
        return m, cov

    def sample_posterior(self, Xtest, nsamples, with_noise=False, jitter=None, rng=None, normals=None):
        """Posterior draws at the test points (cugp_sparse_predict_sample): [nsamples, nt] = mean + normals C^T, C the
        lower Cholesky factor of cov + jitter I (cov as predict_joint).  normals [nsamples, nt] default to
        rng.standard_normal (rng: a numpy Generator or a seed); jitter None: 1e-8 sf2 for latent draws, 0 with noise."""
        Xt = f64(Xtest).reshape(-1, self.d)
        nt, ns = Xt.shape[0], int(nsamples)
        if normals is None:
            gen = rng if isinstance(rng, np.random.Generator) else np.random.default_rng(rng)
            normals = gen.standard_normal((ns, nt))
        Z = f64(normals).reshape(ns, nt)
        if jitter is None:
            jitter = 0.0 if with_noise else 1e-8 * float(np.exp(2.0 * self.get_loghyperparam()[-2]))
        out = np.empty((ns, nt))
        check(capi.lib().cugp_sparse_predict_sample(self._h, ptr(Xt), nt, 1 if with_noise else 0, float(jitter), ns,
                                                    ptr(Z), ptr(out)))
        return out

    def predict_grad(self, Xtest, with_noise=True, want_var_grad=True):
        """Mean, variance and their gradients with respect to the test inputs (cugp_sparse_predict_grad): (mean [nt],
        var [nt], dmean [nt, d], dvar [nt, d] or None).  mean / var carry predict's bits for the same with_noise;
        want_var_grad=False skips U and its two triangular products and returns None for dvar."""
        Xt = f64(Xtest).reshape(-1, self.d)
        nt = Xt.shape[0]
        m, v, dm = np.empty(nt), np.empty(nt), np.empty((nt, self.d))
        dv = np.empty((nt, self.d)) if want_var_grad else None
        check(capi.lib().cugp_sparse_predict_grad(self._h, ptr(Xt), nt, 1 if with_noise else 0, ptr(m), ptr(v), ptr(dm),
                                                  ptr(dv) if want_var_grad else None))
        return m, v, dm, dv

    def predict_cov_plan(self, nt):
        """The product launch of predict_joint at nt test points (cugp_sparse_predict_cov_plan), at the process's current
        tuning: (nt padded to 128, tile edge 64 or 128, k ranges per tile, their length)."""
        return sparse_predict_cov_plan(self.m, nt)

    def plan(self):
        """The schedule (cugp_sparse_plan): one (row0, rows, rows_padded, split, kstep) per pass over the data."""
        return sparse_plan(self.n, self.m, self.chunk_rows)

    def predict_plan(self, nt):
        """The passes predict() takes nt test points in (cugp_sparse_predict_plan): one (row0, rows) per pass."""
        return sparse_predict_plan(self.m, nt)


def sparse_plan(n, m, chunk_rows=0):
    """cugp_sparse_plan's passes for n rows against m inducing inputs: [(row0, rows, rows_padded, split, kstep)]."""
    out = (C.c_int * 5)()
    passes, i = [], 0
    while True:
        count = capi.lib().cugp_sparse_plan(int(n), int(m), int(chunk_rows), i, out)
        if count < 0:
            check(count)
        passes.append(tuple(out))
        i += 1
        if i >= count:
            return passes


def sparse_predict_plan(m, nt):
    """cugp_sparse_predict_plan's passes for nt test points against m inducing inputs: [(row0, rows)]."""
    out = (C.c_int * 2)()
    passes, i = [], 0
    while True:
        count = capi.lib().cugp_sparse_predict_plan(int(m), int(nt), i, out)
        if count < 0:
            check(count)
        passes.append(tuple(out))
        i += 1
        if i >= count:
            return passes


def sparse_predict_cov_plan(m, nt):
    """cugp_sparse_predict_cov_plan for nt test points against m inducing inputs: (ntpad, tile edge, split, kstep)."""
    out = (C.c_int * 4)()
    check(capi.lib().cugp_sparse_predict_cov_plan(int(m), int(nt), out))
    return tuple(out)


class Comm:
    """The library's own RCCL communicator (cugp_comm_*, csrc/comm.cpp): one process per GPU, expert k on rank k mod W.
    `unique_id`: the 128 bytes rank 0 got from Comm.unique_id(), handed to every rank by the caller (ShardedBCM
    broadcasts them through torch.distributed); None with world == 1: no communicator, nothing to exchange."""

    ID_BYTES = 128

    @staticmethod
    def unique_id():
        buf = (C.c_ubyte * Comm.ID_BYTES)()
        check(capi.lib().cugp_comm_unique_id(buf, Comm.ID_BYTES))
        return bytes(buf)

    def __init__(self, unique_id, rank, world, device):
        self.rank, self.world, self.device = int(rank), int(world), int(device)
        self._h = C.c_void_p()
        idbuf = (C.c_ubyte * Comm.ID_BYTES).from_buffer_copy(unique_id) if unique_id is not None else None
        check(capi.lib().cugp_comm_create(idbuf, Comm.ID_BYTES if unique_id is not None else 0, self.rank, self.world,
                                          self.device, C.byref(self._h)))

    def loglik_grad_allgather(self, bcm, per, nh=3):
        """One sharded objective evaluation: this rank's experts (`bcm`: a BCM, or None on a rank that owns none)
        evaluated, everybody's rows gathered -> [world * per, 1 + nh] (rank r's i-th expert in row r * per + i).
        nh: 3, or an ARD BCM's d + 2 -- explicit, since a rank without experts has no BCM to ask; the _ard call is
        taken for an ARD BCM and, without a BCM, for nh != 3."""
        nh = int(nh)
        out = np.empty((self.world * int(per), 1 + nh))
        h = bcm._h if bcm is not None else None
        if bcm._wide if bcm is not None else nh != 3:
            check(capi.lib().cugp_bcm_loglik_grad_allgather_ard(h, self._h, int(per), nh, ptr(out)))
        else:
            if nh != 3:
                raise ValueError("an isotropic BCM has 3 hyper-parameters, not nh = %d" % nh)
            check(capi.lib().cugp_bcm_loglik_grad_allgather(h, self._h, int(per), ptr(out)))
        return out

    def predict_allgather(self, bcm, per, nexperts, Xt, combine=None, with_noise=True, sf2=None, sn2=None):
        """Product-of-experts prediction across the ranks (cugp_bcm_predict_allgather): this rank's experts (`bcm`, or
        None on a rank that owns none) predict Xt, one all-gather moves every rank's rows, the product of experts over
        all `nexperts` experts in expert order -> (mean, var).  Every rank passes the same per, nexperts and Xt.
        combine: None, or "poe" | "gpoe" | "bcm" | "rbcm" -- the rule on the experts' latent distributions
        (cugp_bcm_predict_allgather_mode); then sf2 = exp(2 theta_f) and sn2 = exp(2 theta_n) are needed on every rank
        (a rank without experts has no BCM to read them from; with a BCM they default to its hyper-parameters')."""
        mode = None if combine is None else combine_mode(combine)
        Xt = f64(Xt)
        nt = Xt.shape[0]
        m, v = np.empty(nt), np.empty(nt)
        if mode is not None:
            if sf2 is None or sn2 is None:
                if bcm is None:
                    raise ValueError("a rank without experts must pass sf2 and sn2")
                sf2, sn2 = bcm.prior_scalars()
            check(capi.lib().cugp_bcm_predict_allgather_mode(bcm._h if bcm is not None else None, self._h, int(per),
                                                             int(nexperts), ptr(Xt), nt, mode, 1 if with_noise else 0,
                                                             float(sf2), float(sn2), ptr(m), ptr(v)))
            return m, v
        check(capi.lib().cugp_bcm_predict_allgather(bcm._h if bcm is not None else None, self._h, int(per),
                                                    int(nexperts), ptr(Xt), nt, ptr(m), ptr(v)))
        return m, v

    def predict_grad_allgather(self, bcm, per, nexperts, Xt, d, combine=None, with_noise=True, sf2=None, sn2=None,
                               want_var_grad=True):
        """The combined prediction and its gradients with respect to the test inputs across the ranks
        (cugp_bcm_predict_grad_allgather): this rank's experts (`bcm`, or None on a rank that owns none) fill their
        gradient rows, one all-gather moves every rank's, the chain rule of the rule on the device -> (mean [nt],
        var [nt], dmean [nt, d], dvar [nt, d] or None).  Every rank passes the same per, nexperts, Xt, d, combine and
        want_var_grad.  combine: None -- the reference's product of the noisy predictions -- or "poe" | "gpoe" | "bcm" |
        "rbcm"; sf2, sn2 as predict_allgather's (not read for combine=None)."""
        mode = capi.CUGP_COMBINE_REFERENCE if combine is None else combine_mode(combine)
        d = int(d)
        Xt = f64(Xt).reshape(-1, d)
        nt = Xt.shape[0]
        if sf2 is None or sn2 is None:
            if bcm is not None:
                sf2, sn2 = bcm.prior_scalars()
            elif combine is None:
                sf2, sn2 = 0.0, 0.0
            else:
                raise ValueError("a rank without experts must pass sf2 and sn2")
        m, v, dm = np.empty(nt), np.empty(nt), np.empty((nt, d))
        dv = np.empty((nt, d)) if want_var_grad else None
        check(capi.lib().cugp_bcm_predict_grad_allgather(bcm._h if bcm is not None else None, self._h, int(per),
                                                         int(nexperts), ptr(Xt), nt, d, mode, 1 if with_noise else 0,
                                                         float(sf2), float(sn2), ptr(m), ptr(v), ptr(dm),
                                                         ptr(dv) if want_var_grad else None))
        return m, v, dm, dv

    @staticmethod
    def _shard_list(shards):
        return (C.c_void_p * len(shards))(*[getattr(s, "value", s) for s in shards])

    def sparse_sharded_bound_grad(self, shards, per, nshards, what, nh, m, d):
        """One evaluation of a sparse model whose rows are sharded over the ranks (cugp_sparse_sharded_bound_grad).
        shards: this rank's shard handles (cugp_sparse_create_shard's) in slot order; what: 0 -> F, 1 -> (F, g [nh]),
        2 -> (F, g, gZ [m, d]).  Every rank passes the same per, nshards and what."""
        what = int(what)
        F, g, gZ = C.c_double(), np.empty(int(nh)), np.empty((int(m), int(d)))
        check(capi.lib().cugp_sparse_sharded_bound_grad(self._shard_list(shards), len(shards), self._h, int(per), int(nshards),
                                                        what, C.byref(F), ptr(g) if what >= 1 else None, int(nh),
                                                        ptr(gZ) if what == 2 else None))
        return (F.value,) + ((g,) if what >= 1 else ()) + ((gZ,) if what == 2 else ())

    def sparse_sharded_cg_solve(self, shards, per, nshards, budget, nh, inducing=False):
        """Conjugate gradients on -F of the sharded sparse model (cugp_sparse_sharded_cg_solve), run by every rank alike;
        the trace [n_iterates, nh + 1] = (theta, -F) as SparseGP.cg_solve's."""
        budget = int(budget)
        tr = np.full((4 * max(budget, 0) + 8, int(nh) + 1), np.nan)
        ne = C.c_int()
        check(capi.lib().cugp_sparse_sharded_cg_solve(self._shard_list(shards), len(shards), self._h, int(per), int(nshards),
                                                      budget, 1 if inducing else 0, ptr(tr), tr.shape[0], C.byref(ne)))
        rows = 1
        while rows < min(ne.value, tr.shape[0]) and not np.isnan(tr[rows, 0]):
            rows += 1
        return tr[:rows]

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            capi.lib().cugp_comm_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BCM:
    """Experts resident on the GPU(s) of this process (class BCM, distributed_gp/BCM.h).  `devices` lists the
    GPUs (expert k on devices[k mod len], cg_solver.cpp:93; default: the one `device`).  `BCM.split` reproduces
    the reference constructor's row partition (BCM.cpp:85-110).
    ard=True: every expert an ARD handle (cugp_bcm_create_ard): the shared hyper-parameter vector is [log l_1 .. log l_d,
    log sigma_f, log sigma_n] (nh = d + 2), gradients have nh entries, rows and cg_solve traces 1 + nh columns.
    ard=True is squared-exponential only; kernel="matern32_ard" | "matern52_ard" makes every expert an ARD Matern handle
    (cugp_bcm_create_ard_kernel), as Covsum."""

    def __init__(self, rows, d, device=0, devices=None, kernel="se", ard=False):
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        devs = np.ascontiguousarray([device] if devices is None else list(devices), dtype=np.int32)
        self.rows, self.d, self.device, self.devices = rows.tolist(), int(d), int(devs[0]), devs.tolist()
        self._kind, self.ard = kernel_spec(kernel, ard)
        self.nh = num_hyper(self._kind, self.ard, self.d)
        self._h = C.c_void_p()
        if self._kind == capi.CUGP_KERNEL_RQ:
            check(capi.lib().cugp_bcm_create_rq(len(self.devices), devs.ctypes.data_as(capi._ip), len(self.rows),
                                                rows.ctypes.data_as(capi._ip), self.d, 1 if self.ard else 0,
                                                C.byref(self._h)))
        elif self.ard and self._kind != capi.CUGP_KERNEL_SE:
            check(capi.lib().cugp_bcm_create_ard_kernel(len(self.devices), devs.ctypes.data_as(capi._ip),
                                                        len(self.rows), rows.ctypes.data_as(capi._ip), self.d,
                                                        self._kind, C.byref(self._h)))
        elif self.ard:
            check(capi.lib().cugp_bcm_create_ard(len(self.devices), devs.ctypes.data_as(capi._ip), len(self.rows),
                                                 rows.ctypes.data_as(capi._ip), self.d, C.byref(self._h)))
        elif self._kind != capi.CUGP_KERNEL_SE:
            check(capi.lib().cugp_bcm_create_kernel(len(self.devices), devs.ctypes.data_as(capi._ip), len(self.rows),
                                                    rows.ctypes.data_as(capi._ip), self.d, self._kind,
                                                    C.byref(self._h)))
        else:
            check(capi.lib().cugp_bcm_create_multi(len(self.devices), devs.ctypes.data_as(capi._ip), len(self.rows),
                                                   rows.ctypes.data_as(capi._ip), self.d, C.byref(self._h)))

    @property
    def _wide(self):
        """takes the nh-wide (_ard) calls: ARD, or rational quadratic in either form"""
        return is_wide(self._kind, self.ard)

    @property
    def kernel(self):
        """The covariance family of every expert: "se", "matern32" or "matern52"."""
        k = C.c_int()
        check(capi.lib().cugp_bcm_kernel_kind(self._h, C.byref(k)))
        return REPORTED_NAMES[k.value]

    @classmethod
    def split(cls, X, y, K, device=0, devices=None, kernel="se", ard=False):
        X, y = f64(X), f64(y)
        N, D = X.shape
        part = N // K
        rows = [part] * (K - 1) + [N - part * (K - 1)]
        b = cls(rows, D, device, devices, kernel=kernel, ard=ard)
        off = 0
        for k in range(K):
            b.set_expert_data(k, X[off: off + rows[k]], y[off: off + rows[k]])
            off += part
        return b

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            capi.lib().cugp_bcm_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_expert_data(self, k, X, y):
        X, y = f64(X), f64(y)
        check(capi.lib().cugp_bcm_set_expert_data(self._h, k, ptr(X), ptr(y)))

    def set_BCM_log_hyperparam(self, hp):
        hp = f64(hp)
        if self._wide:
            if hp.shape != (self.nh,):
                raise ValueError("expected %d log-hyper-parameters" % self.nh)
            check(capi.lib().cugp_bcm_set_loghyper_ard(self._h, ptr(hp), self.nh))
        else:
            check(capi.lib().cugp_bcm_set_loghyper(self._h, ptr(hp)))

    set_BCM_loghyper_eigen = set_BCM_log_hyperparam

    def get_loghyperparam(self):
        out = np.empty(self.nh)
        if self._wide:
            check(capi.lib().cugp_bcm_get_loghyper_ard(self._h, ptr(out), self.nh))
        else:
            check(capi.lib().cugp_bcm_get_loghyper(self._h, ptr(out)))
        return out

    def loglik_grad(self):
        """-> (sum LL, sum grad[nh], per-expert LL) over the experts of this GPU."""
        ll = C.c_double()
        g = np.empty(self.nh)
        per = np.empty(len(self.rows))
        if self._wide:
            check(capi.lib().cugp_bcm_loglik_grad_ard(self._h, C.byref(ll), ptr(g), self.nh, ptr(per)))
        else:
            check(capi.lib().cugp_bcm_loglik_grad(self._h, C.byref(ll), ptr(g), ptr(per)))
        return ll.value, g, per

    def loglik_grad_rows(self):
        """-> [K, 1 + nh] rows (LL_k, gradient of -LL_k): what a multi-GPU BCM all-reduces."""
        rows = np.empty((len(self.rows), 1 + self.nh))
        if self._wide:
            check(capi.lib().cugp_bcm_loglik_grad_rows_ard(self._h, ptr(rows), self.nh))
        else:
            check(capi.lib().cugp_bcm_loglik_grad_rows(self._h, ptr(rows)))
        return rows

    def loglik_grad_rows_device(self, dev_rows_ptr, slots):
        """Leave every local expert's (LL_k, gradient) row in DEVICE memory: row slots[k] of the [., 1 + nh] buffer at
        dev_rows_ptr (same GPU) -- the payload of an all-reduce that never touches the host."""
        slots = np.ascontiguousarray(slots, dtype=np.int32)
        if self._wide:
            check(capi.lib().cugp_bcm_loglik_grad_rows_device_ard(self._h, C.c_void_p(dev_rows_ptr),
                                                                  slots.ctypes.data_as(capi._ip), self.nh))
        else:
            check(capi.lib().cugp_bcm_loglik_grad_rows_device(self._h, C.c_void_p(dev_rows_ptr),
                                                              slots.ctypes.data_as(capi._ip)))

    def expert(self, k):
        """Borrowed view of expert k as a Covsum-like object (prediction, intermediates); owned by the BCM."""
        h = C.c_void_p()
        check(capi.lib().cugp_bcm_expert(self._h, int(k), C.byref(h)))
        e = Covsum.__new__(Covsum)
        e.n, e.d, e.device, e._h, e._data_key = self.rows[k], self.d, self.devices[k % len(self.devices)], h, None
        e.ard, e.nh, e._kind = self.ard, self.nh, self._kind
        e.close = lambda: None                    # not ours to destroy
        return e

    def get_BCM_loglikelihood(self):
        return self.loglik_grad()[0]

    def get_BCM_gradient_hyper(self):
        return self.loglik_grad()[1]

    def predict_partial(self, Xt):
        Xt = f64(Xt).reshape(-1, self.d)
        sp, spm = np.empty(Xt.shape[0]), np.empty(Xt.shape[0])
        check(capi.lib().cugp_bcm_predict_partial(self._h, ptr(Xt), Xt.shape[0], ptr(sp), ptr(spm)))
        return sp, spm

    def compute_BCM_test_means_and_var(self, Xt):
        Xt = f64(Xt).reshape(-1, self.d)
        m, v = np.empty(Xt.shape[0]), np.empty(Xt.shape[0])
        check(capi.lib().cugp_bcm_predict(self._h, ptr(Xt), Xt.shape[0], ptr(m), ptr(v)))
        return m, v

    def prior_scalars(self):
        """(sf2, sn2) = (exp(2 theta_f), exp(2 theta_n)) of the shared hyper-parameters, as the library forms them."""
        hp = self.get_loghyperparam()
        return prior_scalars(hp)

    def predict(self, Xt, combine=None, with_noise=True):
        """(mean, var) at Xt.  combine=None: the reference's product of the experts' noisy predictions
        (compute_BCM_test_means_and_var, its bits; with_noise is not read).  "poe" | "gpoe" | "bcm" | "rbcm": the rule on
        the experts' latent distributions (cugp_bcm_predict_mode; include/cugp.h: CUGP_COMBINE_*), var with sn2 added
        when with_noise."""
        if combine is None:
            return self.compute_BCM_test_means_and_var(Xt)
        mode = combine_mode(combine)
        Xt = f64(Xt).reshape(-1, self.d)
        m, v = np.empty(Xt.shape[0]), np.empty(Xt.shape[0])
        check(capi.lib().cugp_bcm_predict_mode(self._h, ptr(Xt), Xt.shape[0], mode, 1 if with_noise else 0, ptr(m),
                                               ptr(v)))
        return m, v

    @property
    def predict_grad_form(self):
        """How the last predict_grad ran (cugp_bcm_predict_grad_form): 0 no call yet, 1 expert by expert, 2 every
        device set as one group of batched launches."""
        f = C.c_int()
        check(capi.lib().cugp_bcm_predict_grad_form(self._h, C.byref(f)))
        return f.value

    def predict_grad(self, Xt, combine=None, with_noise=True):
        """(mean, var, dmean [nt, d], dvar [nt, d]) of the combined prediction at Xt (cugp_bcm_predict_grad: the experts'
        gradients by one group of batched launches per device set, the chain rule of the rule on the host).  combine=None: the reference's product of the noisy
        predictions (predict(Xt)'s bits; with_noise is not read); else the rule on the latent distributions, as predict."""
        mode = capi.CUGP_COMBINE_REFERENCE if combine is None else combine_mode(combine)
        Xt = f64(Xt).reshape(-1, self.d)
        nt = Xt.shape[0]
        m, v, dm, dv = np.empty(nt), np.empty(nt), np.empty((nt, self.d)), np.empty((nt, self.d))
        check(capi.lib().cugp_bcm_predict_grad(self._h, ptr(Xt), nt, mode, 1 if with_noise else 0, ptr(m), ptr(v),
                                               ptr(dm), ptr(dv)))
        return m, v, dm, dv

    get_BCM_negative_log_predprob = staticmethod(Covsum.get_negative_log_predprob)

    def cg_solve(self, budget=100):
        """-> the evaluation trace [n_evals, 1 + nh] = (theta, -LL)."""
        tr = np.zeros((4 * budget + 8, 1 + self.nh))
        ne = C.c_int()
        solve = capi.lib().cugp_bcm_cg_solve_ard if self._wide else capi.lib().cugp_bcm_cg_solve
        check(solve(self._h, budget, ptr(tr), tr.shape[0], C.byref(ne)))
        return tr[: ne.value]


def poe_finish(sum_prec, sum_prec_mean):
    sp, spm = f64(sum_prec), f64(sum_prec_mean)
    m, v = np.empty_like(sp), np.empty_like(sp)
    check(capi.lib().cugp_poe_finish(ptr(sp), ptr(spm), sp.shape[0], ptr(m), ptr(v)))
    return m, v


def poe_combine(rows, mode, sf2, sn2, with_noise=True):
    """cugp_poe_combine: the combination rule `mode` ("poe" | "gpoe" | "bcm" | "rbcm", or the CUGP_COMBINE_* number) on
    latent rows [K, 2, nt] (1/var_f, m/var_f per expert) -> (mean, var); pure host code, needs no GPU."""
    rows = f64(rows)
    if rows.ndim != 3 or rows.shape[1] != 2:
        raise ValueError("rows must be [K, 2, nt]")
    K, _, nt = rows.shape
    m, v = np.empty(nt), np.empty(nt)
    check(capi.lib().cugp_poe_combine(ptr(rows), K, nt, combine_mode(mode) if isinstance(mode, str) else int(mode),
                                      float(sf2), float(sn2), 1 if with_noise else 0, ptr(m), ptr(v)))
    return m, v


def poe_combine_grad(mean, var, dmean, dvar, mode, sf2):
    """cugp_poe_combine_grad: the chain rule of the combination rule `mode` ("poe" | "gpoe" | "bcm" | "rbcm", None or
    "reference" for the product of noisy predictions, or the CUGP_COMBINE_* number) on the experts' means and variances
    [K, nt] and their gradients [K, nt, d] -> (dmean [nt, d], dvar [nt, d]); pure host code, needs no GPU."""
    mean, var, dmean, dvar = f64(mean), f64(var), f64(dmean), f64(dvar)
    if mean.ndim != 2 or var.shape != mean.shape or dmean.ndim != 3 or dmean.shape[:2] != mean.shape or dvar.shape != dmean.shape:
        raise ValueError("mean, var must be [K, nt] and dmean, dvar [K, nt, d]")
    K, nt, d = dmean.shape
    if mode is None or mode == "reference":
        mode = capi.CUGP_COMBINE_REFERENCE
    elif isinstance(mode, str):
        mode = combine_mode(mode)
    om, ov = np.empty((nt, d)), np.empty((nt, d))
    check(capi.lib().cugp_poe_combine_grad(ptr(mean), ptr(var), ptr(dmean), ptr(dvar), K, nt, d, int(mode), float(sf2),
                                           ptr(om), ptr(ov)))
    return om, ov


def cg_minimize(fn, theta, budget=100):
    """Host CG loop of the library on a Python objective fn(theta)->(f, g)."""
    def cb(_ctx, th, f, g):
        fv, gv = fn(np.array([th[0], th[1], th[2]]))
        f[0] = fv
        for i in range(3):
            g[i] = gv[i]
    th = f64(theta).copy()
    tr = np.zeros((4 * budget + 8, 4))
    ne = C.c_int()
    check(capi.lib().cugp_cg_minimize(capi.OBJECTIVE(cb), None, ptr(th), budget, ptr(tr), tr.shape[0],
                                      C.byref(ne)))
    return th, tr[: ne.value]


def cg_minimize_n(fn, theta, budget=100):
    """The same loop over len(theta) entries (cugp_cg_minimize_n) on a Python objective fn(theta)->(f, g);
    -> (theta, trace [n_evals, nh + 1])."""
    th = f64(theta).copy()
    nh = th.shape[0]

    def cb(_ctx, t, n, f, g):
        fv, gv = fn(np.array([t[i] for i in range(n)]))
        f[0] = fv
        for i in range(n):
            g[i] = gv[i]
    tr = np.zeros((4 * budget + 8, nh + 1))
    ne = C.c_int()
    check(capi.lib().cugp_cg_minimize_n(capi.OBJECTIVE_N(cb), None, ptr(th), nh, budget, ptr(tr), tr.shape[0],
                                        C.byref(ne)))
    return th, tr[: ne.value]


def cg_minimize_sparing(value_fn, gradient_fn, theta, budget=100):
    """Evaluation-sparing CG on Python callbacks value_fn(theta)->f, gradient_fn(theta)->g.
    -> (theta, trace, gradient evaluations made)."""
    def vf(_ctx, th, f):
        f[0] = value_fn(np.array([th[0], th[1], th[2]]))

    def gf(_ctx, th, g):
        gv = gradient_fn(np.array([th[0], th[1], th[2]]))
        for i in range(3):
            g[i] = gv[i]
    th = f64(theta).copy()
    tr = np.zeros((4 * budget + 8, 4))
    ne, ng = C.c_int(), C.c_int()
    check(capi.lib().cugp_cg_minimize_sparing(capi.VALUE_FN(vf), capi.GRADIENT_FN(gf), None, ptr(th), budget,
                                              ptr(tr), tr.shape[0], C.byref(ne), C.byref(ng)))
    return th, tr[: ne.value], ng.value


def rprop_minimize(fn, theta, iters=100):
    def cb(_ctx, th, f, g):
        fv, gv = fn(np.array([th[0], th[1], th[2]]))
        f[0] = fv
        for i in range(3):
            g[i] = gv[i]
    th = f64(theta).copy()
    tr = np.zeros((2 * iters + 8, 4))
    ne = C.c_int()
    check(capi.lib().cugp_rprop_minimize(capi.OBJECTIVE(cb), None, ptr(th), iters, ptr(tr), tr.shape[0],
                                         C.byref(ne)))
    return th, tr[: ne.value]


def test_gemm_nt(A, B, device=0):
    A, B = f64(A), f64(B)
    m, k = A.shape
    n = B.shape[0]
    Cm = np.empty((m, n))
    check(capi.lib().cugp_test_gemm_nt(m, n, k, ptr(A), ptr(B), ptr(Cm), device))
    return Cm


def mfma_peak_tflops(device=0):
    out = C.c_double()
    check(capi.lib().cugp_mfma_peak_tflops(device, C.byref(out)))
    return out.value


def potrf(K, device=0):
    K = f64(K)
    L = np.empty_like(K)
    check(capi.lib().cugp_potrf(K.shape[0], ptr(K), ptr(L), device))
    return L


def potri(K, device=0):
    K = f64(K)
    Ki = np.empty_like(K)
    check(capi.lib().cugp_potri(K.shape[0], ptr(K), ptr(Ki), device))
    return Ki


def chol_and_det(K, y, device=0):
    K, y = f64(K), f64(y)
    q, d = C.c_double(), C.c_double()
    check(capi.lib().cugp_chol_and_det(K.shape[0], ptr(K), ptr(y), C.byref(q), C.byref(d), device))
    return q.value, d.value


def potrs_vec(K, y, device=0):
    K, y = f64(K), f64(y)
    x = np.empty(K.shape[0])
    check(capi.lib().cugp_potrs_vec(K.shape[0], ptr(K), ptr(y), ptr(x), device))
    return x
