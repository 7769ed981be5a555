"""fp64 numpy stand-ins for gp.Covsum, gp.SparseGP and gp.BCM with the library's method names, for the call-sequence
harness (tests/handle_sequences.py) to run on without a GPU (tests/test_handle_sequences_cpu.py).

What is modelled is the HOST STATE of a handle, not its kernels: each class keeps its factor, inverse quantities, target
results, LOO results and prediction scratch behind explicit validity flags and shared buffers, as the library does (A
holds K, then L; one scratch for all predictions; the two sides of a sparse model share their work area; ...).  The
numbers come from the existing stand-ins' formulas (truth.standin, truth_append.standin_append, truth_loo.standin,
truth_targets.standin_from, truth_sparse_targets.standin, truth_sparse_joint.standin, truth_predict_grad, truth_poe_modes):
no new numerics.  The gradient continued from a valid factor takes alpha = K^-1 y (truth.standin's order), the combined
evaluation alpha = T' (T y) (truth_predict_grad.standin's): two routes that agree to rounding only, as in the library.

A covariance that cannot be factored (the poison steps of the harness) gives NaN results, never an exception: the
factorisations fall back on numerical_failure.nan_flow_cholesky, and finite input takes the route it always took.

MUTATIONS: names that, when in the module's set ACTIVE, switch one invalidation off.  Every handle created while a name is
active carries it -- the twin too: a mutation shows only through what the long-lived handle has lived through.
"""
import functools

import numpy as np

import numerical_failure as nf
import truth
import truth_append
import truth_ard_matern as tam
import truth_loo
import truth_poe_modes as tpm
import truth_predict_grad as tpg
import truth_sparse_joint as tsj
import truth_sparse_targets as tst

TILE = 128
MUTATIONS = (
    "hp_keeps_targets",          # set_loghyperparam leaves the target results valid
    "append_keeps_loo_n",        # append leaves the old n in the LOO pass
    "smaller_prediction_reads_scratch",   # a prediction at fewer points than the previous one returns the previous rows
    "hp_tolerance",              # an unchanged-hp set is detected with a tolerance of 1e-9
    "k_train_keeps_factor",      # compute_K_train leaves factor_valid set
    "targets_keep_columns",      # set_targets with an unchanged padded width does not clear the old columns
    "sparse_sides_independent",  # evaluating one side does not mark the other stale
    "set_inducing_keeps_row_z",  # set_inducing keeps row_z
    "expert_data_keeps_sum",     # BCM: set_expert_data on one expert keeps the cached sum
    "view_taken_for_group",      # BCM: an expert view's own evaluation at the BCM's hp is taken for the group's
    "failed_eval_keeps_gradient",    # an evaluation whose LL is not finite leaves the previous evaluation's gradient in place
    "sparse_kuu_failure_keeps_row",  # a side keeps its previous result row when Kuu cannot be factored
)
ACTIVE = set()


class Refused(RuntimeError):
    code = -1                                                        # CUGP_ERR_INVALID


def _spec(kernel, ard):
    """(kind, ard) as gp.kernel_spec: kind 0 SE, 1 Matern 3/2, 2 Matern 5/2."""
    k = kernel.lower()
    if k.endswith("_ard"):
        k, ard = k[:-4], True
    return {"se": 0, "matern32": truth.MATERN32, "matern52": truth.MATERN52}[k], bool(ard)


def descriptor(kind, ard, hp):
    hp = [float(h) for h in hp]
    if ard:
        return tam.ARDMatern(hp, kind, np.float64) if kind else truth.ARD(hp, np.float64)
    return truth.Matern(hp, kind, np.float64) if kind else truth.SE(hp, np.float64)


def _same_hp(a, b):
    if "hp_tolerance" in ACTIVE:
        return bool(np.all(np.abs(a - b) <= 1e-9))
    return bool(np.all(a == b))


def _pad(n):
    return (n + TILE - 1) // TILE * TILE


def _cg(fn, theta, budget):
    """The library's own conjugate-gradient loop (host code, no device) on a Python objective."""
    from cugp_amd import gp
    return gp.cg_minimize_n(fn, theta, budget)


# -- a covariance that cannot be factored is no error (include/cugp.h): NaN results, never an exception.  Every helper
# takes the route it always took on finite input, so the healthy sequences keep their bits.
def _quiet(fn):
    """NaN and inf are results here, not warnings."""
    @functools.wraps(fn)
    def wrapped(*a, **kw):
        with np.errstate(all="ignore"):
            return fn(*a, **kw)
    return wrapped


def _chol(K):
    """The lower factor; of a matrix that has none, nf.nan_flow_cholesky's: healthy columns, then NaN."""
    try:
        return np.linalg.cholesky(K)
    except np.linalg.LinAlgError:
        return nf.nan_flow_cholesky(K)


def _trisolve(L, B):
    """L^-1 B; NaN throughout once L holds a NaN (every result the handles report from it sums over a NaN row)."""
    import scipy.linalg as sl
    if not np.all(np.isfinite(L)):
        return np.full(np.shape(B), np.nan)
    return sl.solve_triangular(L, B, lower=True)


# ================================================================================================ Covsum
class Covsum:
    def __init__(self, n, d, device=0, npad_min=0, ard=False, kernel="se"):
        self.n, self.d = int(n), int(d)
        self._kind, self.ard = _spec(kernel, ard)
        self.nh = self.d + 2 if self.ard else 3
        self.capacity = _pad(max(self.n, int(npad_min)))
        self.mut = frozenset(ACTIVE)
        self.X, self.y = np.zeros((self.capacity, self.d)), np.zeros(self.capacity)
        self.theta = np.zeros(self.nh)
        self.have_data = self.factor_valid = self.inverse_valid = False
        self.A = None                                                # K, then L: one buffer, as the library's
        self.T = self.Ki = self.alpha = self.z = None
        self.logdet = self.last_ll = np.nan
        self.last_g = np.full(self.nh, np.nan)
        self.pred = np.zeros((0, 2))                                 # the scratch of predict / predict_latent / predict_grad
        self.pred_nt = 0
        self.loo_n, self.loo_valid, self.loo_row, self.loo_pt = self.n, False, None, None
        self.tg_m = self.tg_mpad = 0
        self.tg_y, self.tg_valid, self.tg_out = None, False, None

    def close(self):
        pass

    @property
    def cov(self):
        return descriptor(self._kind, self.ard, self.theta)

    def _stale(self, loo=True):
        """The factor and the inverse are gone; loo: so are the LOO results (they depend on data and hp alone, so a call
        that only rebuilds the factor leaves them)."""
        self.factor_valid = self.inverse_valid = False
        if loo:
            self.loo_valid = False

    # -- data and hyper-parameters
    def set_data(self, X, y):
        self.X[:self.n], self.y[:self.n] = X, y
        self.have_data = True
        self.tg_valid = False
        self._stale()

    def set_loghyperparam(self, hp):
        hp = np.asarray(hp, dtype=np.float64)
        if _same_hp(hp, self.theta):
            return
        self.theta = hp.copy()
        self._stale()
        if "hp_keeps_targets" not in self.mut:
            self.tg_valid = False

    def get_loghyperparam(self):
        return self.theta.copy()

    def append(self, X, y):
        X, y = np.atleast_2d(X), np.atleast_1d(y)
        k = len(y)
        if self.tg_m > 0:
            raise Refused("append: the handle has targets set")
        if self.n + k > self.capacity:
            raise Refused("append: %d + %d rows exceed the capacity of %d" % (self.n, k, self.capacity))
        n0, update = self.n, self.inverse_valid
        self.X[n0:n0 + k], self.y[n0:n0 + k] = X, y
        self.n = n0 + k
        if "append_keeps_loo_n" not in self.mut:
            self.loo_n = self.n
        self.tg_valid = False
        self._stale()
        if update:                                                   # the bordering of truth_append, from the factors held
            self._border(n0, k)
            if not np.isfinite(self.last_ll):                        # a Schur complement that cannot be factored: nothing of the
                self.factor_valid = self.inverse_valid = False       # evaluation is kept (cugp_append's discard_eval)
                self.last_ll, self.last_g = np.nan, np.full(self.nh, np.nan)

    # -- the evaluations
    @_quiet
    def _finish(self, alpha):
        """ll and the gradient from T, K^-1, log|K| and alpha (truth.standin's formulas)."""
        n, c = self.n, self.cov
        self.alpha = alpha
        self.z = self.T @ self.y[:n]
        self.last_ll = -0.5 * (self.z @ self.z + self.logdet + n * truth.LL_CONST)
        _, terms = c.train(self.X[:n])
        W = self.Ki - np.outer(alpha, alpha)
        if not ("failed_eval_keeps_gradient" in self.mut and not np.isfinite(self.last_ll)):
            self.last_g = np.array(terms(W) + (c.sn2 * np.trace(W),))
        self.factor_valid = self.inverse_valid = True

    def _build_factor(self):
        n, c = self.n, self.cov
        self.A = _chol(c.train(self.X[:n])[0] + c.sn2 * np.eye(n))

    @_quiet
    def _eval(self, grad):
        """An evaluation from the covariance build on (enqueue_eval)."""
        import scipy.linalg as sl
        n = self.n
        self._stale(loo=False)
        self._build_factor()
        L = self.A
        self.logdet = 2 * np.log(np.diag(L)).sum()
        if not grad:
            self.z = _trisolve(L, self.y[:n])
            self.last_ll = -0.5 * (self.z @ self.z + self.logdet + n * truth.LL_CONST)
            self.factor_valid = True
            return
        self.T = _trisolve(L, np.eye(n))
        self.Ki = self.T.T @ self.T
        self._finish(self.T.T @ (self.T @ self.y[:n]))

    @_quiet
    def _continue(self):
        """The inverse quantities from the factor A holds (enqueue_continue): whatever A holds."""
        import scipy.linalg as sl
        n = self.n
        L = np.tril(self.A)
        self.T = _trisolve(L, np.eye(n))
        self.Ki = self.T.T @ self.T
        self.logdet = 2 * np.log(np.abs(np.diag(L))).sum()
        self._finish(self.Ki @ self.y[:n])

    @_quiet
    def _border(self, n0, k):
        """truth_append.standin_append's pass over the new rows, on the T, K^-1, z, alpha the handle holds."""
        import scipy.linalg as sl
        c, X, y = self.cov, self.X, self.y
        T, Ki, z, a, logdet = self.T, self.Ki, self.z, self.alpha, self.logdet
        for r0, r1 in truth_append.plan(n0, k):
            kk = r1 - r0
            B = c.k(X[r0:r1], X[:r0])
            P = B @ T.T
            V = P @ T
            S = c.k(X[r0:r1], X[r0:r1]) + c.sn2 * np.eye(kk) - P @ P.T
            Cf = _chol(S)
            Ci = _trisolve(Cf, np.eye(kk))
            Q = -(Ci @ V)
            zb = Ci @ (y[r0:r1] - P @ z)
            T = np.block([[T, np.zeros((r0, kk))], [Q, Ci]])
            Ki = np.block([[Ki + Q.T @ Q, Q.T @ Ci], [Ci.T @ Q, Ci.T @ Ci]])
            a = np.concatenate([a + Q.T @ zb, Ci.T @ zb])
            z = np.concatenate([z, zb])
            logdet = logdet + 2 * np.log(np.diag(Cf)).sum()
        self.T, self.Ki, self.logdet = T, Ki, logdet
        grown = np.zeros((self.n, self.n))                           # (A keeps the old factor in its corner, as the library's)
        grown[:n0, :n0] = self.A
        self.A = grown
        self._finish(a)

    def _need_factor(self):
        if not self.have_data:
            raise Refused("no training data set")
        if not self.factor_valid:
            self._eval(False)

    def _need_inverse(self):
        if not self.have_data:
            raise Refused("no training data set")
        if not self.inverse_valid:
            if self.factor_valid:
                self._continue()
            else:
                self._eval(True)

    def compute_loglikelihood(self, X=None, y=None):
        self._need_factor()
        return self.last_ll

    def loglik_grad(self, X=None, y=None):
        self._need_inverse()
        return self.last_ll, self.last_g.copy()

    def compute_gradient_loghyperparam(self, X=None, y=None):
        return self.loglik_grad()[1]

    def enqueue(self, want_grad=True):
        self._eval(bool(want_grad))

    def fetch(self):
        return self.last_ll, self.last_g.copy()

    def last_quad_logdet(self):
        if not self.factor_valid:
            raise Refused("no evaluation available")
        return self.z @ self.z, self.logdet

    # -- intermediates
    @_quiet
    def compute_K_train(self, X=None):
        n, c = self.n, self.cov
        K = c.train(self.X[:n])[0] + c.sn2 * np.eye(n)
        self.A = K.copy()                                            # A is overwritten: the factor is gone
        self.inverse_valid = False
        if "k_train_keeps_factor" not in self.mut:
            self.factor_valid = False
        return K

    def compute_squared_dist(self, c):
        if self.ard:
            raise Refused("compute_squared_dist: an ARD handle has no single length scale")
        S = truth.sqdist(self.X[:self.n], self.X[:self.n], np.float64) / c
        self.A = S.copy()
        self._stale(loo=False)
        return S

    @_quiet
    def compute_k_test(self, Xt):
        return self.cov.k(np.asarray(Xt, dtype=np.float64).reshape(-1, self.d), self.X[:self.n])

    def get_cholesky(self):
        if not self.factor_valid:
            raise Refused("get_cholesky: evaluate the likelihood first")
        return np.tril(self.A)

    def get_K_inverse(self):
        if not self.inverse_valid:
            raise Refused("get_K_inverse: evaluate the gradient first")
        return self.Ki.copy()

    def get_alpha(self):
        if not self.inverse_valid:
            raise Refused("get_alpha: evaluate the gradient first")
        return self.alpha.copy()

    # -- prediction: one scratch, grown on demand, for the three calls
    def _through_scratch(self, cols):
        """Write the columns of a prediction into the scratch and read nt rows back, as the library's copies do."""
        nt = len(cols[0])
        if self.pred.shape[0] < _pad(nt) or self.pred.shape[1] < len(cols):
            self.pred = np.zeros((_pad(nt), max(len(cols), self.pred.shape[1])))
            self.pred_nt = 0
        if not ("smaller_prediction_reads_scratch" in self.mut and nt < self.pred_nt):
            for j, col in enumerate(cols):
                self.pred[:nt, j] = col
        self.pred_nt = nt
        return [self.pred[:nt, j].copy() for j in range(len(cols))]

    @_quiet
    def _predict(self, Xtest, latent):
        self._need_inverse()
        c = self.cov
        Xt = np.asarray(Xtest, dtype=np.float64).reshape(-1, self.d)
        Ks = c.k(Xt, self.X[:self.n])
        Wt = Ks @ self.T.T
        return Xt, Ks, Wt, Ks @ self.alpha, c.sf2 + (0.0 if latent else c.sn2) - (Wt * Wt).sum(1)

    def compute_test_means_and_variances(self, X, y, Xtest):
        _, _, _, m, v = self._predict(Xtest, False)
        return tuple(self._through_scratch([m, v]))

    def predict_latent(self, Xtest):
        _, _, _, m, v = self._predict(Xtest, True)
        return tuple(self._through_scratch([m, v]))

    @_quiet
    def predict_grad(self, Xtest, with_noise=True, want_var_grad=True):
        Xt, Ks, Wt, m, v = self._predict(Xtest, not with_noise)
        c = self.cov
        grads = tam.gradients if isinstance(c, tam.ARDMatern) else tpg.gradients
        dm, dv = grads(c, Xt, self.X[:self.n], self.alpha, Wt @ self.T)
        cols = self._through_scratch([m, v] + list(dm.T) + list(dv.T))
        d = self.d
        return cols[0], cols[1], np.array(cols[2:2 + d]).T.copy(), np.array(cols[2 + d:]).T.copy()

    @_quiet
    def compute_test_joint(self, X, y, Xtest, with_noise=True):
        Xt, _, Wt, m, _ = self._predict(Xtest, True)
        c = self.cov
        cov = c.k(Xt, Xt) - Wt @ Wt.T
        return m, cov + c.sn2 * np.eye(len(Xt)) if with_noise else cov

    @_quiet
    def sample_posterior(self, X, y, Xtest, nsamples, with_noise=False, jitter=None, rng=None, normals=None):
        m, cov = self.compute_test_joint(None, None, Xtest, with_noise)
        try:
            Cf = np.linalg.cholesky(cov + float(jitter or 0.0) * np.eye(len(m)))
        except np.linalg.LinAlgError:
            return np.full((int(nsamples), len(m)), np.nan)
        return m[None, :] + np.asarray(normals, dtype=np.float64).reshape(int(nsamples), len(m)) @ Cf.T

    # -- leave-one-out (truth_loo.standin's formulas on the K^-1 and alpha held); the results are kept until the handle is stale
    @_quiet
    def _loo(self, want_grad):
        self._need_inverse()
        if self.loo_valid and (self.loo_row[1] is not None or not want_grad):
            return
        n, c = self.loo_n, self.cov                                  # (the rows of the LOO pass)
        Ki, a, y = self.Ki[:n, :n], self.alpha[:n], self.y[:n]
        self.loo_pt = truth_loo.point_quantities(np.diag(Ki).copy(), a, y, truth.LL_CONST)
        ll = 0.0
        for v in self.loo_pt[2]:
            ll = ll + v
        g = None
        if want_grad:
            W = truth_loo.fused(Ki, a)
            g = np.array(c.train(self.X[:n])[1](W) + (c.sn2 * np.trace(W),))
        self.loo_row, self.loo_valid = (ll, g), True

    def loo(self, want_grad=True):
        self._loo(want_grad)
        return self.loo_row[0], (self.loo_row[1].copy() if want_grad else None)

    def loo_predict(self):
        self._loo(False)
        return tuple(np.array(v, dtype=np.float64) for v in self.loo_pt)

    # -- targets: Y lives zero padded to whole 128-column tiles; the sums run over the padded width
    def set_targets(self, Y):
        Y = np.asarray(Y, dtype=np.float64)
        if not self.have_data:
            raise Refused("set_targets: no training data set")
        m, mpad = Y.shape[1], _pad(Y.shape[1])
        self.tg_valid = False
        if mpad != self.tg_mpad:
            self.tg_y, self.tg_mpad = np.zeros((mpad, self.capacity)), mpad
        elif "targets_keep_columns" not in self.mut:
            self.tg_y[:] = 0.0
        self.tg_y[:m, :self.n] = Y.T
        self.tg_m = m

    @property
    def num_targets(self):
        return self.tg_m

    @_quiet
    def _targets(self):
        if self.tg_m <= 0:
            raise Refused("no targets set")
        self._need_inverse()
        if self.tg_valid:
            return
        n, m, c = self.n, self.tg_m, self.cov                        # truth_targets.standin_from, A over the padded width
        Z = self.tg_y[:, :n] @ self.T.T
        A = Z @ self.T
        each = -0.5 * ((Z[:m] * Z[:m]).sum(1) + self.logdet + n * truth.LL_CONST)
        ll = 0.0
        for v in each:
            ll = ll + v
        W = m * self.Ki - A.T @ A
        g = np.array(c.train(self.X[:n])[1](W) + (c.sn2 * np.trace(W),))
        self.tg_out, self.tg_valid = (ll, g, each, A[:m].copy()), True

    def loglik_grad_targets(self):
        self._targets()
        return self.tg_out[0], self.tg_out[1].copy(), self.tg_out[2].copy()

    def get_alpha_targets(self):
        self._targets()
        return self.tg_out[3].T.copy()

    @_quiet
    def predict_targets(self, Xtest):
        self._targets()
        Xt, Ks, Wt, _, v = self._predict(Xtest, False)
        return Ks @ self.tg_out[3].T, v

    # -- optimisers: the library's loop over this handle's objective; the end point stays set
    def _solve(self, objective, budget):
        def fn(th):
            self.set_loghyperparam(th)
            return objective()
        end, trace = _cg(fn, self.theta.copy(), budget)
        self.set_loghyperparam(end)
        return trace

    def cg_solve(self, X=None, y=None, budget=100):
        def objective():
            ll, g = self.loglik_grad()
            return -ll, g
        return self._solve(objective, budget)

    def cg_solve_loo(self, budget=100):
        def objective():
            ll, g = self.loo(True)
            return -ll, g
        return self._solve(objective, budget)


# ================================================================================================ SparseGP
class _Side:
    def __init__(self):
        self.Y = None                    # [p][n]
        self.valid = self.row_grad = self.row_z = False
        self.row = self.gz = None


class SparseGP:
    """The two sides share one work area (the library's P, the factor handle b and the chunk scratch): the side evaluated
    last owns it, and a prediction reads the solves of its side out of it."""

    def __init__(self, n, m, d, device=0, kernel="se", ard=False, jitter=1e-6, chunk_rows=0):
        self.n, self.m, self.d = int(n), int(m), int(d)
        self._kind, self.ard = _spec(kernel, ard)
        self.nh = self.d + 2 if self.ard else 3
        self.jitter, self.chunk_rows = float(jitter), int(chunk_rows)
        self.mut = frozenset(ACTIVE)
        self.X = self.Z = None
        self.theta = np.zeros(self.nh)
        self.own, self.tg = _Side(), _Side()
        self.work = None                 # (Y of the side that wrote it)

    def close(self):
        pass

    @property
    def cov(self):
        return descriptor(self._kind, self.ard, self.theta)

    def _all_stale(self, keep_row_z=False):
        self.own.valid = self.tg.valid = False
        if not keep_row_z:
            self.own.row_z = self.tg.row_z = False

    def set_data(self, X, y):
        self.X = np.array(X, dtype=np.float64)
        self.own.Y = np.array(y, dtype=np.float64)[None, :]
        self._all_stale()

    def set_inducing(self, Z):
        self.Z = np.array(Z, dtype=np.float64)
        self._all_stale(keep_row_z="set_inducing_keeps_row_z" in self.mut)

    def get_inducing(self):
        if self.Z is None:
            raise Refused("no inducing inputs set")
        return self.Z.copy()

    def set_loghyperparam(self, hp):
        hp = np.asarray(hp, dtype=np.float64)
        if _same_hp(hp, self.theta):
            return
        self.theta = hp.copy()
        self._all_stale()

    def get_loghyperparam(self):
        return self.theta.copy()

    def set_targets(self, Y):
        self.tg.Y = np.array(Y, dtype=np.float64).T.copy()
        self.tg.valid = self.tg.row_z = False

    @property
    def num_targets(self):
        return 0 if self.tg.Y is None else len(self.tg.Y)

    def _eval(self, side, want_grad=False, want_z=False):
        if self.X is None:
            raise Refused("no data set")
        if side.Y is None:
            raise Refused("no targets set")
        if self.Z is None:
            raise Refused("no inducing inputs set")
        other = self.tg if side is self.own else self.own
        if side.valid and (side.row_grad or not want_grad):
            if want_z and not side.row_z:                            # the Z gradient alone, on the row that is held
                side.gz, side.row_z = self._standin(side.Y)[5], True
            return
        if "sparse_sides_independent" not in self.mut:
            other.valid = False
        F, g, each, _, _, gz = self._standin(side.Y)
        self.work = side.Y                                           # the work area now holds this side's solves
        if ("sparse_kuu_failure_keeps_row" in self.mut and side.row is not None and len(side.row[2]) == len(each)
                and not np.isfinite(F) and not self._kuu_finite()):
            side.row_grad, side.valid = want_grad, True              # (the row of the evaluation before stays)
            if want_z:
                side.gz, side.row_z = gz if side.gz is None else side.gz, True
            return
        side.row, side.row_grad, side.valid = (F, g, each), want_grad, True
        if want_z:
            side.gz, side.row_z = gz, True

    @_quiet
    def _kuu_finite(self):
        return bool(np.all(np.isfinite(self.cov.k(self.Z, self.Z))))

    @_quiet
    def _standin(self, Y, Xt=None):
        """tst.standin; NaN throughout where Kuu or B cannot be factored (scipy refuses a matrix that is not finite, LAPACK
        one that is not positive definite), or where the bound comes out not finite: the library's `pd`."""
        Xt = self.X[:1] if Xt is None else Xt
        try:
            out = tst.standin(self.cov, self.X, Y, self.Z, Xt, self.chunk_rows, self.jitter)
        except (np.linalg.LinAlgError, ValueError):
            out = None
        if out is None or not np.isfinite(out[0]):
            p, nt = len(Y), len(Xt)
            return (np.nan, np.full(self.nh, np.nan), np.full(p, np.nan), np.full((p, nt), np.nan), np.full(nt, np.nan),
                    np.full(self.Z.shape, np.nan))
        return out

    # -- the handle's own y
    def bound(self):
        self._eval(self.own)
        return self.own.row[0]

    def bound_grad(self):
        self._eval(self.own, True)
        return self.own.row[0], self.own.row[1].copy()

    def bound_grad_z(self):
        self._eval(self.own, True, True)
        return self.own.row[0], self.own.row[1].copy(), self.own.gz.copy()

    def _points(self, Xtest):
        return np.asarray(Xtest, dtype=np.float64).reshape(-1, self.d)

    def _predict(self, side, Xtest, with_noise):
        """means [p][nt] and the variance from the work area: the labels of whichever side wrote it last."""
        self._eval(side)
        out = self._standin(self.work, self._points(Xtest))
        return out[3], out[4] if with_noise else out[4] - float(self.cov.sn2)

    def predict(self, Xtest, with_noise=True):
        m, v = self._predict(self.own, Xtest, with_noise)
        return m[0], v

    @_quiet
    def _joint(self, Xtest):
        self._eval(self.own)
        Xt = self._points(Xtest)
        nan = (np.full((len(Xt), len(Xt)), np.nan), np.full(Xt.shape, np.nan), np.full(Xt.shape, np.nan))
        try:                                                         # (a side that is not `pd` predicts NaN)
            out = tsj.standin(self.cov, self.X, self.work[0], self.Z, Xt, self.chunk_rows, self.jitter)
        except (np.linalg.LinAlgError, ValueError):
            return nan
        return out if all(np.all(np.isfinite(v)) for v in out) else nan

    def predict_joint(self, Xtest, with_noise=True):
        mean = self.predict(Xtest, with_noise)[0]
        cov = self._joint(Xtest)[0]
        return mean, cov + float(self.cov.sn2) * np.eye(len(mean)) if with_noise else cov

    def sample_posterior(self, Xtest, nsamples, with_noise=False, jitter=None, rng=None, normals=None):
        m, cov = self.predict_joint(Xtest, with_noise)
        try:
            Cf = np.linalg.cholesky(cov + float(jitter or 0.0) * np.eye(len(m)))
        except np.linalg.LinAlgError:
            return np.full((int(nsamples), len(m)), np.nan)
        return m[None, :] + np.asarray(normals, dtype=np.float64).reshape(int(nsamples), len(m)) @ Cf.T

    def predict_grad(self, Xtest, with_noise=True, want_var_grad=True):
        m, v = self.predict(Xtest, with_noise)
        _, dm, dv = self._joint(Xtest)
        return m, v, dm, dv

    # -- the targets' side
    def bound_targets(self):
        self._eval(self.tg)
        return self.tg.row[0], self.tg.row[2].copy()

    def bound_grad_targets(self):
        self._eval(self.tg, True)
        return self.tg.row[0], self.tg.row[1].copy(), self.tg.row[2].copy()

    def bound_grad_z_targets(self):
        self._eval(self.tg, True, True)
        return self.tg.row[0], self.tg.row[1].copy(), self.tg.gz.copy(), self.tg.row[2].copy()

    def predict_targets(self, Xtest, with_noise=True):
        return self._predict(self.tg, Xtest, with_noise)

    # -- optimisers
    def _solve(self, side, budget, inducing):
        self._eval(side)                                             # (the refusals come first)
        nh, shape = self.nh, self.Z.shape

        def fn(v):
            self.set_loghyperparam(v[:nh])
            if inducing and not np.array_equal(v[nh:].reshape(shape), self.Z):
                self.set_inducing(v[nh:].reshape(shape))
            self._eval(side, True, inducing)
            g = np.concatenate([side.row[1], side.gz.ravel()]) if inducing else side.row[1]
            return -side.row[0], g
        start = np.concatenate([self.theta, self.Z.ravel()]) if inducing else self.theta.copy()
        end, trace = _cg(fn, start, budget)
        if inducing and not np.array_equal(end[nh:].reshape(shape), self.Z):
            self.set_inducing(end[nh:].reshape(shape))
        self.set_loghyperparam(end[:nh])
        return np.concatenate([trace[:, :nh], trace[:, -1:]], axis=1)

    def cg_solve(self, budget=100, inducing=False):
        return self._solve(self.own, budget, inducing)

    def cg_solve_targets(self, budget=100, inducing=False):
        return self._solve(self.tg, budget, inducing)


# ================================================================================================ BCM
class BCM:
    """Experts are Covsum stand-ins of the common padded size; the sums of an evaluation are kept until a call makes them
    stale.  An evaluation of the model drops every expert's factor and evaluates all of them from their data."""

    def __init__(self, rows, d, device=0, devices=None, kernel="se", ard=False):
        self.rows, self.d = [int(r) for r in rows], int(d)
        self._kind, self.ard = _spec(kernel, ard)
        self.nh = self.d + 2 if self.ard else 3
        self.mut = frozenset(ACTIVE)
        self.experts = [Covsum(r, d, npad_min=max(self.rows), ard=ard, kernel=kernel) for r in self.rows]
        self.hp = np.zeros(self.nh)
        self.sum_valid, self.sums = False, None

    def close(self):
        pass

    def expert(self, k):
        return self.experts[k]

    def set_expert_data(self, k, X, y):
        self.experts[k].set_data(X, y)
        if "expert_data_keeps_sum" not in self.mut:
            self.sum_valid = False

    def set_BCM_log_hyperparam(self, hp):
        hp = np.asarray(hp, dtype=np.float64)
        if not _same_hp(hp, self.hp):
            self.sum_valid = False
        self.hp = hp.copy()
        for e in self.experts:
            e.set_loghyperparam(hp)

    def get_loghyperparam(self):
        return self.hp.copy()

    @_quiet
    def _evaluate(self):
        if self.sum_valid:
            return
        for e in self.experts:
            if "view_taken_for_group" in self.mut and e.inverse_valid:
                continue                                             # (the expert's own evaluation stands for the group's)
            e._eval(True)
        rows = np.array([np.concatenate([[e.last_ll], e.last_g]) for e in self.experts])
        ll, g = 0.0, None
        for r in rows:                                               # the host sum runs in expert order
            ll = ll + r[0]
            g = r[1:].copy() if g is None else g + r[1:]
        self.sums, self.sum_valid = (ll, g, rows), True

    def loglik_grad(self):
        self._evaluate()
        return self.sums[0], self.sums[1].copy(), self.sums[2][:, 0].copy()

    def loglik_grad_rows(self):
        self._evaluate()
        return self.sums[2].copy()

    def _refresh(self):
        if not all(e.inverse_valid for e in self.experts):
            self.sum_valid = False
            self._evaluate()

    def _experts_at(self, Xt, latent):
        self._refresh()
        out = [e._predict(Xt, latent) for e in self.experts]
        return np.array([o[3] for o in out]), np.array([o[4] for o in out]), out

    @_quiet
    def compute_BCM_test_means_and_var(self, Xt):
        m, v, _ = self._experts_at(Xt, False)
        sp = spm = np.zeros(m.shape[1])
        for k in range(len(m)):                                      # truth.poe's sums, in expert order
            sp, spm = sp + 1 / v[k], spm + m[k] / v[k]
        return spm / sp, 1 / sp

    @_quiet
    def predict(self, Xt, combine=None, with_noise=True):
        if combine is None:
            return self.compute_BCM_test_means_and_var(Xt)
        m, v, _ = self._experts_at(Xt, True)
        c = self.experts[0].cov
        mean, var = tpm.combine(m, v, combine, c.sf2)
        return mean, var + c.sn2 if with_noise else var

    @_quiet
    def predict_grad(self, Xt, combine=None, with_noise=True):
        mean, var = self.predict(Xt, combine, with_noise)
        m, v, out = self._experts_at(Xt, combine is not None)
        c = self.experts[0].cov
        grads = tam.gradients if isinstance(c, tam.ARDMatern) else tpg.gradients
        dm, dv = zip(*[grads(c, o[0], e.X[:e.n], e.alpha, o[2] @ e.T) for e, o in zip(self.experts, out)])
        dmean, dvar = tpg.combine_grad(m, v, np.array(dm), np.array(dv), combine or "reference", c.sf2)
        return mean, var, dmean, dvar

    def cg_solve(self, budget=100):
        def fn(th):
            self.set_BCM_log_hyperparam(th)
            self.sum_valid = False
            ll, g, _ = self.loglik_grad()
            return -ll, g
        end, trace = _cg(fn, self.hp.copy(), budget)
        self.set_BCM_log_hyperparam(end)
        return trace
