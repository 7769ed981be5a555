/*
 * cugp.h -- C-ABI of the MI355X-native GP-regression hot path (libcugp.so).
 *
 * Drop-in boundary for the reference's GP objective.  Every entry
 * point names the reference interface it replaces (paths relative to the reference
 * checkout).  Two reference surfaces bind here:
 *   A. class Covsum            cpp_serial_gp/covkernel.h:3-38   (cugp_amd/host/covkernel.h wraps this ABI)
 *   B. the free functions over file-scope globals that main.cpp / cg_solver.cpp forward-declare,
 *      cuda_scalingdist/main.cpp:21-53                          (cugp_amd/host/gp_api.h wraps this ABI)
 * plus class BCM, distributed_gp/BCM.h:2-27.
 *
 * Conventions
 *   - plain pointers and sizes only; all arrays fp64; X is row-major n x d, caller-owned HOST memory
 *     unless a function says "device";
 *   - every function returns 0 (CUGP_OK) or a negative code and never exits the process
 *     (the reference exits on CUDA errors, cuda_scalingdist/cuda_gp.cu:98-107);
 *   - a covariance matrix that is not positive definite is NOT an error: results come back NaN,
 *     which the line search relies on (covkernel.cpp:509-524);
 *   - hyper-parameters are the reference's log-hyper vector [log l, log sigma_f, log sigma_n];
 *   - gradients are d(-LL)/d(theta), as Covsum::compute_gradient_loghyperparam returns them;
 *   - a handle may be used by one host thread at a time; all device work of a handle is ordered on
 *     its own HIP stream.
 */
#ifndef CUGP_H
#define CUGP_H

#ifdef __cplusplus
extern "C" {
#endif

#define CUGP_OK 0
#define CUGP_ERR_INVALID (-1)   /* bad argument / call order */
#define CUGP_ERR_NOMEM (-2)     /* host or device allocation failed */
#define CUGP_ERR_DEVICE (-3)    /* HIP runtime error; see cugp_last_error() */
#define CUGP_ERR_NODEVICE (-4)  /* no gfx950 device visible */
#define CUGP_ERR_BUSY (-5)      /* an evaluation of this handle / group is still in flight: fetch it first */

typedef struct cugp_gp cugp_gp;    /* one expert: Covsum / the cuda_gp.cu global state */
typedef struct cugp_bcm cugp_bcm;  /* a set of experts resident on one GPU: class BCM */

int cugp_version(void);
/* hash of the sources this library was built from (cugp_amd/build.py: source_hash); measurements kept as files carry
 * it, so a reader can tell which library they belong to (bench.py: roofline.traffic) */
const char *cugp_build_id(void);
const char *cugp_last_error(void);          /* thread-local text of the last failure */
int cugp_device_count(int *count);

/* ---- lifetime: Covsum::Covsum(n,d) covkernel.cpp:14-37 ; setup(numtrain,dim) cuda_scalingdist/cuda_gp.cu:587 ;
 *      ~Covsum covkernel.cpp:39-61 ; destruct_cublas_cusoler cuda_gp.cu ---- */
int cugp_create(int n, int d, int device, cugp_gp **out);
/* the same with the matrices padded (by identity rows: no result changes) to at least npad_min rows -- the
 * experts of a BCM get one common padded size so that they can share launches (distributed_gp/BCM.cpp:85-110
 * gives the last expert the remainder rows) */
int cugp_create_padded(int n, int d, int device, int npad_min, cugp_gp **out);
int cugp_destroy(cugp_gp *gp);
int cugp_dims(const cugp_gp *gp, int *n, int *d, int *npad);
/* A gradient evaluation builds L^-1 and K^-1 block row by block row on three further streams while the
 * factorisation is still running (its tail leaves most of the chip idle).  On by default; cugp_bcm_create
 * turns it off when several experts share the device.  No reference counterpart (the reference calls
 * cusolverDnDpotrf, then inverts: cuda_scalingdist/cuda_gp.cu:647-708). */
int cugp_set_overlap(cugp_gp *gp, int enable);

/* ---- data: the X,y arguments of every Covsum method ; copy_training_data_to_GPU cuda_gp.cu:510-518 ---- */
int cugp_set_data(cugp_gp *gp, const double *X, const double *y);
int cugp_set_data_device(cugp_gp *gp, const double *dX, const double *dy);   /* device pointers, same device */

/* ---- hyper-parameters: set_loghyperparam / get_loghyperparam / set_loghyper_eigen covkernel.cpp:266-274,325-329 ;
 *      set_loghyper_eigen / get_loghyperparam cuda_gp.cu:960-975 ---- */
int cugp_set_loghyper(cugp_gp *gp, const double hp[3]);
int cugp_get_loghyper(const cugp_gp *gp, double hp[3]);

/* ---- ARD: one length scale per input dimension (automatic relevance determination).  The reference has no
 *      counterpart (its Covsum has ONE length scale, covkernel.cpp:64-102); the convention is GPML's covSEard:
 *        theta = [log l_1 .. log l_d, log sigma_f, log sigma_n]     (nh = d + 2 entries: the order above, first entry widened)
 *        k(x, x') = sf2 exp(-1/2 sum_c ((x_c - x'_c) / l_c)^2) + sn2 delta,   sf2 = exp(2 theta_d), sn2 = exp(2 theta_{d+1})
 *      with 1 / l_c = exp(-theta_c) evaluated on the host and every DIFFERENCE x_c - x'_c weighted before it is squared.
 *      Gradients are of -LL: g_c = 1/2 sum_ij W_ij Kf_ij ((x_ic - x_jc) / l_c)^2 (W = K^-1 - alpha alpha', Kf = K - sn2 I),
 *      then the signal and the noise component as g[1], g[2] of the isotropic form.
 * A handle made by the create call below is ARD for life.  Data, overlap, the log-likelihood, the split enqueue, the
 * predictions (marginal, joint, draws), K, k_test, factor, inverse, alpha, profiling and tuning work on it unchanged; the
 * 3-entry calls (set / get of the hyper-parameters, the gradient calls, the optimisers, the squared-distance
 * intermediate) return CUGP_ERR_INVALID on it and name the call to use.  ARD handles are the experts of an ARD BCM
 * (cugp_bcm_create_ard below): evaluated as a group of shared launches like isotropic experts.
 * The calls below return CUGP_ERR_INVALID -- before any device call -- for a NULL argument, an isotropic handle, or
 * nh != d + 2.  A theta_c so large that 1 / l_c underflows simply drops dimension c (g_c = 0); one so small that it
 * overflows gives NaN results (the header's convention for a covariance that cannot be factored), not an error.
 * The number of hyper-parameters of any handle (3, or d + 2) is reported through *nh; set / get copy nh entries;
 * the combined and the fetch form return LL and the nh gradient components (fetch: g may be NULL). */
int cugp_create_ard(int n, int d, int device, cugp_gp **out);
/* the same with the matrices padded to at least npad_min rows (cugp_create_padded's rule): the experts of an ARD BCM, and an
 * ARD handle with room for cugp_append */
int cugp_create_ard_padded(int n, int d, int device, int npad_min, cugp_gp **out);
int cugp_num_hyper(const cugp_gp *gp, int *nh);
int cugp_set_loghyper_ard(cugp_gp *gp, const double *hp, int nh);
int cugp_get_loghyper_ard(const cugp_gp *gp, double *hp, int nh);
int cugp_loglik_grad_ard(cugp_gp *gp, double *ll, double *g, int nh);
int cugp_loglik_grad_fetch_ard(cugp_gp *gp, double *ll, double *g /* may be NULL */, int nh);

/* ---- covariance families: Matern 3/2 and 5/2 beside the squared exponential.  The reference has no counterpart; the
 *      convention is GPML's covMaterniso with d = 3 and d = 5.  The hyper-parameters are the isotropic three,
 *      theta = [log l, log sigma_f, log sigma_n], so every 3-entry call, the exchange rows and the optimisers carry over.
 *      With s = |x - x'|^2 / l^2, r = sqrt(s), sf2 = exp(2 theta_1), sn2 = exp(2 theta_2):
 *        CUGP_KERNEL_SE       k = sf2 exp(-s / 2) + sn2 delta                      (every other create call)
 *        CUGP_KERNEL_MATERN32 a = sqrt(3) r:  k = sf2 (1 + a) exp(-a) + sn2 delta,          dk/dtheta_0 = sf2 a^2 exp(-a)
 *        CUGP_KERNEL_MATERN52 a = sqrt(5) r:  k = sf2 (1 + a + a^2/3) exp(-a) + sn2 delta,  dk/dtheta_0 = sf2 (a^2/3)(1 + a) exp(-a)
 *      Gradients are of -LL as everywhere: g0 = 1/2 sum W o dK/dtheta_0, g1 = sum W o Kf, g2 = sn2 tr W
 *      (W = K^-1 - alpha alpha', Kf = K - sn2 I).  k(x, x) = sf2 + sn2 for every kind.  l -> inf (s = 0) gives exactly sf2;
 *      l^2 = 0 (s = +inf) and an exp(-a) that underflows give exactly 0 for k and dk/dtheta_0 off the diagonal.
 * The kind is fixed when the handle is created.  Kind 0 through cugp_create_kernel is cugp_create_padded's handle, bit for
 * bit; an unknown kind is CUGP_ERR_INVALID before any device call.  Every call that works on an isotropic handle works
 * on a Matern one: data, overlap, LL / gradient in all forms, the continuation from a valid factor, the predictions
 * (marginal, joint, draws), K, k_test, the squared-distance intermediate (which does not depend on the kind), factor,
 * inverse, alpha, profiling, tuning, the optimisers, groups and every cugp_bcm_* call.  cugp_create_ard stays SE;
 * cugp_create_ard_kernel below is ARD with a Matern kind.  Experts of one group (and so of one BCM) must have the same
 * kind; the ranks of a BCM
 * sharded one process per GPU must be created with the same kind -- the caller's duty, like passing the same Xt. */
#define CUGP_KERNEL_SE 0
#define CUGP_KERNEL_MATERN32 1
#define CUGP_KERNEL_MATERN52 2
int cugp_create_kernel(int n, int d, int device, int npad_min, int kernel, cugp_gp **out);
int cugp_kernel_kind(const cugp_gp *gp, int *kernel);

/* ---- ARD x covariance family: one length scale per input dimension with a Matern kind (GPML's covMaternard, the
 *      default kernel of BoTorch and scikit-optimize).  theta, its order and nh = d + 2 are the ARD handle's above.  With
 *      w_c = exp(-theta_c), u_c = (x_c - x'_c) w_c, s = sum_c u_c^2, a = sqrt(3 s) or sqrt(5 s), e = exp(-a):
 *        CUGP_KERNEL_MATERN32  Kf = sf2 (1 + a) e              dk/dtheta_c = H u_c^2,  H = 3 sf2 e
 *        CUGP_KERNEL_MATERN52  Kf = sf2 (1 + a + a^2/3) e      dk/dtheta_c = H u_c^2,  H = (5/3) sf2 (1 + a) e
 *      Gradients of -LL: g_c = 1/2 sum_ij W_ij H_ij u_c,ij^2, then g_d = sum W o Kf and g_{d+1} = sn2 tr W as for every
 *      handle.  H has no singularity at a = 0; equal length scales give the isotropic Matern handle's model; k(x, x) =
 *      sf2 + sn2.  An e that underflows gives exactly 0 for Kf and H.
 * Kind 0 is cugp_create_ard_padded's handle: the same launches, bit for bit.  An unknown kind is CUGP_ERR_INVALID
 * before any device call.  cugp_kernel_kind reports the kind; every call that works on an ARD handle works on these
 * unchanged
 * (the _ard calls, predictions and their input gradients, targets, cugp_append, groups, cugp_cg_solve_ard).  Experts of
 * one group must agree in kind and in the ARD flag. */
int cugp_create_ard_kernel(int n, int d, int device, int npad_min, int kernel, cugp_gp **out);

/* ---- rational quadratic covariance (GPML covRQiso / covRQard, scikit-learn's RationalQuadratic): a scale mixture of
 *      squared exponentials whose shape alpha is learned -- the first hyper-parameter that is neither a length scale nor
 *      a variance.  sigma_f and sigma_n stay the last two entries of theta.
 *      ard = 1:  nh = d + 3, theta = [log l_1 .. log l_d, log alpha, log sigma_f, log sigma_n]
 *        w_c = exp(-theta_c),  u_c = (x_c - x'_c) w_c,  s = sum_c u_c^2   (differences weighted before squaring)
 *        alpha = exp(theta_d),  u = s / (2 alpha),  L = log1p(u)
 *        Kf = sf2 exp(-alpha L)                     (= sf2 (1 + u)^-alpha;  K = Kf + sn2 delta)
 *        H  = Kf / (1 + u)                          dK/dtheta_c = H u_c^2 (c < d),   dk/dx*_c = -H (x*_c - x_c) w_c^2
 *        A  = Kf alpha (u / (1 + u) - L)            dK/dtheta_d = A   (zero on the diagonal)
 *      Gradient of -LL with W = K^-1 - alpha alpha':  g_c = 1/2 sum W o H o u_c^2 (c < d),  g_d = 1/2 sum W o A,
 *        g_{d+1} = sum W o Kf,  g_{d+2} = sn2 tr W.
 *      s = 0 gives Kf = H = sf2 and A = 0 exactly; alpha -> inf approaches the SE-ARD entry (4e-14 apart at theta_alpha =
 *      30).  An alpha whose exp overflows gives NaN results with CUGP_OK, the convention of a covariance that cannot be
 *      factored: not an error.
 *      ard = 0:  nh = 4, theta = [log l, log alpha, log sigma_f, log sigma_n]: the form above with all d weights equal to
 *        exp(-theta_0).  g_0 = g_l1 + ... + g_ld added in index order (the chain rule at equal scales); LL, K, the
 *        predictions and the other three components are the ard = 1 handle's at equal scales, bit for bit.
 * cugp_kernel_kind reports CUGP_KERNEL_RQ, cugp_num_hyper 4 or d + 3.  Both forms are nh-wide handles: every call that
 * works on an ARD handle works on them unchanged with the handle's nh -- the _ard hyper-parameter, gradient and fetch
 * calls, cugp_loglik and the split enqueue, the marginal, latent and joint predictions and the draws, cugp_predict_grad,
 * cugp_set_targets and the _targets calls, cugp_append / cugp_capacity, cugp_loo, cugp_loo_predict, cugp_cg_solve_loo,
 * cugp_cg_solve_ard, cugp_cg_solve_targets, K, k_test, factor, inverse, alpha, profiling, tuning, groups and captured
 * graphs (a new alpha reaches a captured graph by the same one copy as new weights).  The 3-entry calls refuse them as
 * they refuse ARD handles and name the call to use.  Experts of one group must agree in kind AND in `ard`.
 * CUGP_ERR_INVALID before any device call, with "cugp_create_rq" in cugp_last_error: out NULL, n or d not positive,
 * npad_min negative, ard outside {0, 1}.  The kind is NOT accepted by cugp_create_kernel, cugp_create_ard_kernel, the
 * cugp_bcm_create*_kernel calls or cugp_sparse_create*: a sparse model with this kernel is not built. */
#define CUGP_KERNEL_RQ 3
int cugp_create_rq(int n, int d, int device, int npad_min, int ard, cugp_gp **out);

/* ---- objective ----
 * cugp_loglik       : Covsum::compute_loglikelihood covkernel.cpp:118-129 ; compute_log_likelihood cuda_gp.cu:838-855
 * cugp_loglik_grad  : the pair compute_loglikelihood + compute_gradient_loghyperparam (covkernel.cpp:162-263 ;
 *                     compute_gradient_log_hyperparams cuda_gp.cu:885-957) that cg_solve always calls together,
 *                     from ONE factorisation
 * cugp_grad         : gradient alone (same device work as cugp_loglik_grad) */
int cugp_loglik(cugp_gp *gp, double *ll);
int cugp_loglik_grad(cugp_gp *gp, double *ll, double g[3]);
int cugp_grad(cugp_gp *gp, double g[3]);
/* split form, so several experts can be in flight at once: enqueue on the handle's stream, then fetch */
int cugp_loglik_grad_enqueue(cugp_gp *gp, int want_grad);
int cugp_loglik_grad_fetch(cugp_gp *gp, double *ll, double g[3] /* may be NULL */);
/* y' K^-1 y and log|K| of the last evaluation: compute_chol_and_det matrixops.cpp:232-234 */
int cugp_last_quad_logdet(const cugp_gp *gp, double *quad, double *logdet);

/* ---- prediction: Covsum::compute_test_means_and_variances covkernel.cpp:277-323 (variance includes the
 *      noise term, :316) ; compute_k_test :105-116 ; get_negative_log_predprob :649-659 ; testing_phase
 *      cuda_src/cuda_gp.cu:2063 ---- */
int cugp_predict(cugp_gp *gp, const double *Xt, int nt, double *mean, double *var);
/* the LATENT function at the test points (no reference counterpart): mean = cugp_predict's, bit for bit, by the same
 * launches; var = sf2 - |W_t|^2 (W = Ks L^-T), the variance of f without the noise term, computed directly -- never as
 * cugp_predict's variance minus sn2.  Works on every handle cugp_predict works on (SE, Matern, ARD, padded handles, BCM
 * experts); a stale handle is evaluated first.  CUGP_ERR_INVALID for a NULL argument or nt <= 0, before any device call. */
int cugp_predict_latent(cugp_gp *gp, const double *Xt, int nt, double *mean, double *var);
/* ---- gradients of the prediction with respect to the test inputs (what an acquisition function maximised by L-BFGS,
 *      active learning or a sensitivity analysis needs).  The reference has no counterpart: neither Covsum
 *      (cpp_serial_gp/covkernel.h) nor the CUDA code differentiates a prediction.  With k_i = k(x*, x_i), the noise term
 *      not entering, alpha = K^-1 y and v = K^-1 k* = (W L^-1)^T, W = Ks L^-T as cugp_predict forms it:
 *        mean(x*) = sum_i alpha_i k_i                    dmean / dx*_c = sum_i alpha_i dk_i / dx*_c
 *        var(x*)  = sf2 (+ sn2) - k*^T K^-1 k*           dvar / dx*_c  = -2 sum_i v_i dk_i / dx*_c
 *        dk_i / dx*_c = -G_i (x*_c - x_ic) s_c
 *          SE          G = k_i,                           s_c = 1 / l^2
 *          ARD         G = k_i,                           s_c = w_c^2 = 1 / l_c^2
 *          Matern 3/2  G = sf2 3 exp(-a),                 s_c = 1 / l^2        (a = sqrt(3) r)
 *          Matern 5/2  G = sf2 (5/3) (1 + a) exp(-a),     s_c = 1 / l^2        (a = sqrt(5) r)
 *      G is finite at r = 0 and nothing divides by r: at a test point that IS a training row that row contributes G * 0.
 *      The noisy and the latent variance have the same gradient.  The difference x*_c - x_ic is formed first, then
 *      multiplied (no cancellation where |x| >> |x - x'|); sums run in a fixed order without atomics: the same bits on
 *      every call, whatever nt is and whatever else the handle holds (v is always W L^-1, never Ks K^-1).
 * cugp_predict_grad: mean [nt] and var [nt] (either may be NULL) by cugp_predict's own launches -- with_noise != 0 they
 *      carry cugp_predict's bits, else cugp_predict_latent's; dmean and dvar [nt][d] row-major (either may be NULL; dvar
 *      NULL skips the second triangular product: the mean's gradient needs alpha alone).  Works on every handle
 *      cugp_predict works on (SE, Matern, ARD, padded handles, BCM experts); a stale handle is evaluated first, an
 *      evaluation in flight is fetched first.  CUGP_ERR_INVALID -- before any device call -- for a NULL gp or Xt, nt <= 0,
 *      or dmean and dvar both NULL.  Non-finite inputs propagate by IEEE with CUGP_OK (the header's convention).
 * Not built: gradients of the joint covariance or of draws, of multi-target means.  (The experts of a BCM run as one
 *      batched sequence of launches in cugp_bcm_predict_grad; the form across ranks is cugp_bcm_predict_grad_allgather.) */
int cugp_predict_grad(cugp_gp *gp, const double *Xt, int nt, int with_noise,
                      double *mean /* nt, may be NULL */, double *var /* nt, may be NULL */,
                      double *dmean /* [nt][d], may be NULL */, double *dvar /* [nt][d], may be NULL */);
/* ---- joint predictive distribution: extends the marginal form of Covsum::compute_test_means_and_variances
 *      covkernel.cpp:277-323 (the noise term as at :316) to the covariance between the test points; the reference has
 *      no joint counterpart.  Both work on every handle cugp_predict works on (padded handles, BCM experts), at the
 *      current data and hyper-parameters (a stale handle is evaluated first, as for cugp_predict); an evaluation in
 *      flight is fetched first, as cugp_predict does.
 * cugp_predict_cov: joint predictive distribution at nt test points.
 *   mean : nt, the same bits as cugp_predict (may be NULL)
 *   cov  : nt x nt row-major, full symmetric (mirrored, exactly symmetric):
 *          k(Xt,Xt) - Ks K^-1 Ks^T, plus sigma_n^2 I when with_noise (then diag(cov) is cugp_predict's var up to rounding)
 * cugp_predict_sample: posterior draws: samples[s*nt + t] = mean[t] + sum_{k<=t} C[t][k] * normals[s*nt + k],
 *   C = lower Cholesky factor of (cov + jitter I), cov as above, computed by the library's blocked Cholesky;
 *   normals: caller-supplied standard normals [nsamples][nt] (the library has no RNG: results are reproducible);
 *   jitter >= 0; a matrix that is not positive definite gives NaN samples, not an error (header convention)
 * Errors: CUGP_ERR_INVALID for a NULL gp, Xt, cov, normals or samples, nt <= 0, nsamples <= 0, or a jitter that is
 * negative or not finite -- before any device call. */
int cugp_predict_cov(cugp_gp *gp, const double *Xt, int nt, int with_noise, double *mean, double *cov);
int cugp_predict_sample(cugp_gp *gp, const double *Xt, int nt, int with_noise, double jitter,
                        int nsamples, const double *normals, double *samples);
int cugp_nlpp(const double *actual, const double *mean, const double *var, int nt, double *nlpp);

/* ---- appending observations to a factored model (the last step of predict-with-gradients / observe / add; the reference
 *      has no counterpart: Covsum is rebuilt, cpp_serial_gp/covkernel.cpp:14-37).  A Cholesky factor grows by bordering, so
 *      everything a handle holds stays valid as the leading block of the larger problem.  With B = k(Xb, X), P = B L^-T,
 *      V = P L^-1, S = k(Xb, Xb) + sn2 I - P P^T, C = chol(S), Q = -C^-1 V, zb = C^-1 (yb - P z):
 *        L' = [L 0; P C]   L'^-1 = [L^-1 0; Q C^-1]   K'^-1 = [K^-1 + Q'Q, Q'C^-1; C^-T Q, C^-T C^-1]
 *        z' = [z; zb]   alpha' = [alpha + Q' zb; C^-T zb]   quad' = quad + zb'zb   log|K'| = log|K| + 2 sum log C_ii
 *      O(k N^2) per call instead of the N^3 of a fresh evaluation; every sum in a fixed order, no atomics.
 * cugp_capacity   : *cap <- the rows the handle can hold: its padded size (cugp_dims' npad), fixed when it is created --
 *                   cugp_create_padded / cugp_create_kernel / cugp_create_ard_padded take it as npad_min.
 * cugp_append     : k further rows Xnew [k][d], ynew [k] (host).  On a handle that holds its inverse quantities (a gradient
 *                   evaluation at the current data and hyper-parameters, nothing in flight) they are extended in place on
 *                   the handle's stream -- factor, inverse, K^-1, z, alpha, log-determinant -- LL and the gradient are
 *                   taken at the n + k rows, and every call (cugp_loglik_grad, cugp_predict*, cugp_predict_grad,
 *                   cugp_get_*) then answers for the larger model without further device work beyond its own.  On any
 *                   other handle (fresh data, changed hyper-parameters, a log-likelihood-only factor) only the data grows
 *                   and the next evaluation factors n + k rows: the same results, only the cost differs.  An evaluation in
 *                   flight is fetched first.  Works on SE, Matern and ARD handles.  cugp_set_data keeps taking the
 *                   handle's CURRENT number of rows.
 * cugp_append_plan: the passes of an append of k rows to n (pure arithmetic, no device): pass i covers the rows
 *                   [out[0], out[1]); no pass crosses a multiple of 128, the passes cover [n, n + k) once, ascending; returns
 *                   the number of passes, or CUGP_ERR_INVALID for a pass beyond the last.  Each pass is one bordering step:
 *                   its rows lie in one tile row and C inside one diagonal tile.
 * Refusals, all CUGP_ERR_INVALID before any device call with the reason in cugp_last_error, the handle unchanged: a NULL
 * argument; k <= 0; n + k beyond the capacity; no data yet; a handle with targets (cugp_set_targets); an expert of a
 * cugp_bcm, for good, or a handle that a group of shared launches holds, until that group is destroyed.
 * A Schur complement that is not positive definite (a duplicate row at vanishing noise, non-finite input) gives NaN
 * results with CUGP_OK (the header's convention); the data stays extended and the next evaluation starts afresh.
 * Not built: removing rows; append on BCM experts or across ranks; append with targets; an append that skips K^-1 for
 * callers who only predict; growing beyond the capacity. */
int cugp_capacity(const cugp_gp *gp, int *cap);
int cugp_append(cugp_gp *gp, const double *Xnew /* [k][d], host */, const double *ynew /* k */, int k);
int cugp_append_plan(int n, int k, int pass, int out[2]);

/* ---- intermediates (parity tests; each copies device -> host) ----
 * cugp_compute_K_train : Covsum::compute_K_train covkernel.cpp:64-102 -> full symmetric n x n
 * cugp_compute_squared_dist : Covsum::compute_squared_dist covkernel.cpp:130-157 -> |xi-xj|^2 / c, zero diagonal
 * cugp_compute_k_test  : Covsum::compute_k_test covkernel.cpp:105-116 -> nt x n
 * cugp_get_cholesky    : get_cholesky matrixops.cpp:68-108 -> lower factor of the last evaluation, upper zeroed
 * cugp_get_K_inverse   : compute_K_inverse matrixops.cpp:383-435 -> full symmetric (needs a gradient evaluation)
 * cugp_get_alpha       : vector_Kinvy_using_cholesky matrixops.cpp:264-316 (needs a gradient evaluation) */
int cugp_compute_K_train(cugp_gp *gp, double *K);
int cugp_compute_squared_dist(cugp_gp *gp, double c, double *S);
int cugp_compute_k_test(cugp_gp *gp, const double *Xt, int nt, double *Ks);
int cugp_get_cholesky(cugp_gp *gp, double *L);
int cugp_get_K_inverse(cugp_gp *gp, double *Kinv);
int cugp_get_alpha(cugp_gp *gp, double *alpha);

/* ---- multi-target regression: m target vectors y_t over the handle's inputs and hyper-parameters share ONE
 *      factorisation.  The reference has no counterpart (its Covsum holds one y); the model is scikit-learn's
 *      GaussianProcessRegressor with a 2-d y: independent outputs, shared kernel and theta.  Everything that costs N^3
 *      (K, its factor, L^-1, K^-1) depends on X and theta alone and is the handle's own evaluation, untouched; what
 *      depends on the targets is N^2 work per target behind it:
 *        z_t = L^-1 y_t,  alpha_t = L^-T z_t = K^-1 y_t,  LL_t = -1/2 (z_t'z_t + log|K| + n * 1.83787),  LL = sum_t LL_t
 *        gradient of -LL in the handle's convention, component order and nh:  W = m K^-1 - sum_t alpha_t alpha_t',
 *        g_theta = 1/2 sum_ij W_ij dK_ij/dtheta  (noise component sn2 tr W) -- each family's own per-entry formulas
 *        mean of target t at the test points: Ks alpha_t; the variance does not depend on the targets (cugp_predict's).
 *      log|K| is the handle's own (cugp_last_quad_logdet), LL_t are added in target order.
 * The targets are an ADDITIONAL data set on the handle: cugp_set_data is still required (it supplies X) and its y, with
 * every call above, is unchanged by and unrelated to them.  Targets persist until replaced; a second cugp_set_targets
 * may change m.  The calls work on an isotropic handle of any kernel kind and on an ARD handle.
 * cugp_set_targets        : Y is [m][n], target-major (row t = y_t), host memory
 * cugp_num_targets        : *m <- the number of targets, 0 before cugp_set_targets
 * cugp_loglik_grad_targets: *ll <- LL, g <- the nh gradient components (nh must equal cugp_num_hyper), ll_each <- the m
 *                           LL_t; any of the three may be NULL.  A stale handle is evaluated first (cugp_loglik_grad).
 * cugp_predict_targets    : mean [m][nt] target-major, var (may be NULL) nt -- cugp_predict's launches and bits
 * cugp_get_alpha_targets  : alpha [m][n], row t = K^-1 y_t
 * cugp_cg_solve_targets   : cugp_cg_minimize_n over the handle's nh entries on f = -LL; trace rows of 1 + nh doubles; the
 *                           end point stays set, as cugp_cg_solve leaves it
 * The results of one (data, theta, targets) are kept: a repeated call costs no device work.
 * Errors: CUGP_ERR_INVALID, with the call's name in cugp_last_error, for a NULL gp, Y, Xt, mean or alpha, m <= 0,
 * nt <= 0, an nh that is not the handle's, an evaluation or prediction before cugp_set_targets, cugp_set_targets before
 * cugp_set_data; argument errors come before any device call.  CUGP_ERR_NODEVICE without a GPU.  A covariance that is not
 * positive definite gives NaN results with CUGP_OK (the header's convention).
 * Not built: targets on BCM experts and groups, joint covariance and draws per target, an LL-only form. */
int cugp_set_targets(cugp_gp *gp, const double *Y /* [m][n], target-major, host */, int m);
int cugp_num_targets(const cugp_gp *gp, int *m);
int cugp_loglik_grad_targets(cugp_gp *gp, double *ll /* sum */, double *g /* nh, may be NULL */, int nh,
                             double *ll_each /* m, may be NULL */);
int cugp_predict_targets(cugp_gp *gp, const double *Xt, int nt, double *mean /* [m][nt] */,
                         double *var /* nt, may be NULL */);
int cugp_get_alpha_targets(cugp_gp *gp, double *alpha /* [m][n] */);
int cugp_cg_solve_targets(cugp_gp *gp, int budget, double *trace, int trace_cap, int *nevals);

/* ---- leave-one-out cross-validation (LOO) from the factored model (Rasmussen & Williams, GPML 5.10-5.13; GPML's infLOO).
 *      After an evaluation that forms the inverse the handle holds K^-1 and alpha; with kappa_i = [K^-1]_ii the LOO predictive
 *      distribution of training point i, from the other n - 1 points, is
 *        mu_i = y_i - alpha_i / kappa_i,   var_i = 1 / kappa_i   (the variance of y_i, noise included)
 *        logp_i = 1/2 log kappa_i - alpha_i^2 / (2 kappa_i) - 1/2 * 1.83787,   L_LOO = sum_i logp_i
 *      (1.83787: the literal LL uses for log 2 pi).  O(n) beyond the evaluation.  The gradient costs one symmetric N^3 tile
 *      product whatever the number of hyper-parameters:  a_i = alpha_i / kappa_i,  c_i = (1 + alpha_i^2 / kappa_i) / kappa_i,
 *      b = K^-1 a,  W_loo = K^-1 diag(c) K^-1 - b alpha' - alpha b',  d(-L_LOO)/dtheta_j = 1/2 tr(W_loo dK/dtheta_j) --
 *      the marginal likelihood's gradient pass with W_loo in the place of K^-1 - alpha alpha'.
 * cugp_loo          : *lpl <- L_LOO; g (may be NULL) <- the nh components of the gradient of -L_LOO, the convention, order
 *                     and nh of cugp_loglik_grad / cugp_loglik_grad_ard (nh must equal cugp_num_hyper).  g == NULL launches
 *                     the objective alone and allocates no N^2 scratch; the first call with g allocates two npad^2 matrices,
 *                     kept until cugp_destroy (CUGP_ERR_NOMEM, the handle as it was, when they do not fit).
 * cugp_loo_predict  : mean, var and logp (may be NULL) of every training row, n each, in cugp_set_data's row order
 * cugp_cg_solve_loo : the loop of cugp_cg_minimize_n on f = -L_LOO from the current hyper-parameters, for every family
 *                     (isotropic handles: nh = 3); the end point stays set.  trace (may be NULL): rows of nh + 1 doubles
 *                     [theta, f] as cugp_cg_solve_ard writes them, but of the ITERATES, not of every evaluation: the
 *                     start, then the point each line search ended at (the accepted step, or the best probe of a search
 *                     that failed), so f never rises along the trace and its last row is the end point; rejected
 *                     probes are not recorded.  The row behind the last one written is all NaN where trace_cap leaves
 *                     room for it.  *nevals <- evaluations made (at least the number of rows).
 * A stale handle (new data or hyper-parameters, or only cugp_loglik behind it) is evaluated first, as cugp_predict does;
 * a handle extended by cugp_append answers for all its rows.  Every call launches again: equal inputs give equal bits.
 * No result of any other call changes: the LOO passes write buffers of their own.
 * Errors: CUGP_ERR_INVALID with the call's name in cugp_last_error, before any launch, for a NULL gp, lpl, mean or var,
 * an nh that is not the handle's, budget <= 0, no data; CUGP_ERR_NODEVICE without a GPU; CUGP_ERR_DEVICE as everywhere.
 * A covariance that is not positive definite gives NaN results with CUGP_OK (the header's convention).
 * Not built: LOO over the m targets of cugp_set_targets (the calls read the handle's own y); a batched or sharded LOO
 * for a product of experts (cugp_bcm, cugp_group); a C++ Covsum method in cugp_amd/host/. */
int cugp_loo(cugp_gp *gp, double *lpl, double *g /* nh, may be NULL */, int nh);
int cugp_loo_predict(cugp_gp *gp, double *mean /* n */, double *var /* n */, double *logp /* n, may be NULL */);
int cugp_cg_solve_loo(cugp_gp *gp, int budget, double *trace, int trace_cap, int *nevals);

/* ---- sparse variational GP regression on M inducing inputs (SGPR: Titsias 2009, "Variational learning of inducing
 *      variables in sparse Gaussian processes"; GPML ch. 8 for the family; GPflow's SGPR).  No reference counterpart.
 *      Data X [N][d], y [N]; inducing inputs Z [M][d], given by the caller (cugp_sparse_cg_solve_z moves them); the hyper-parameters, their order
 *      and nh (3, ARD d + 2) and the five covariance families are those of a cugp_gp; s2 = exp(2 theta_n), sf2 =
 *      exp(2 theta_f); eps an absolute jitter fixed at creation (not a hyper-parameter, no gradient).  With
 *        Kuu = k(Z,Z) + eps I,  Kuf = k(Z,X),  Qff = Kfu Kuu^-1 Kuf
 *        F(theta) = -N/2 log 2 pi - 1/2 log|Qff + s2 I| - 1/2 y'(Qff + s2 I)^-1 y - (N sf2 - tr Qff) / (2 s2)
 *      a lower bound on the exact log marginal likelihood of all N rows (log 2 pi exactly here, not LL's literal), computed as
 *        Lu = chol(Kuu),  A = Lu^-1 Kuf / s,  B = I + A A',  LB = chol(B),  c = LB^-1 A y / s
 *        F = -N/2 log 2 pi - 1/2 log|B| - N/2 log s2 - y'y / (2 s2) + 1/2 c'c - N sf2 / (2 s2) + 1/2 tr(A A')
 *      in O(N M^2) time and O(M^2 + chunk_rows M) memory: the data is streamed in chunks of chunk_rows rows, A A' and A y
 *      are sums over the rows (a split-k Gram product on the MFMA tile, partial tiles added in a fixed order: equal inputs
 *      and chunk_rows give equal bits).  Prediction at x*, ks = k(Z, x*):
 *        mean = (Lu^-1 ks)' LB^-T c,   var_f = sf2 - |Lu^-1 ks|^2 + |LB^-1 Lu^-1 ks|^2   (+ s2 with noise)
 *      Gradient: with Phi = Kuf Kfu, v = Kuf y, Sigma = Kuu + Phi / s2, beta = Sigma^-1 v / s2,
 *        G_Phi = (Kuu^-1 - Sigma^-1 - beta beta') / (2 s2),  G_uu = Kuu^-1 / 2 - (Sigma^-1 + beta beta') / 2 - Kuu^-1 Phi Kuu^-1 / (2 s2)
 *        G_uf = 2 G_Phi Kuf + (beta / s2) y'   [M x N]
 *        dF/dtheta_j = sum G_uu o dKuu/dtheta_j + sum G_uf o dKuf/dtheta_j   (- N sf2 / s2 for theta_f)
 *        dF/dtheta_n = 2 s2 [-N / (2 s2) + tr(Sigma^-1 Phi) / (2 s2^2) + y'y / (2 s2^2) - v'beta / s2^2 + beta'Phi beta / (2 s2^2)
 *                            + (N sf2 - tr Kuu^-1 Phi) / (2 s2^2)]
 *      through Lu and LB (Sigma^-1 = Lu^-T B^-1 Lu^-1), one weight product and one rectangular trace pass per chunk for any nh.
 *      Gradient with respect to the inducing inputs: with H the factor of the input derivatives (SE and SE-ARD: k itself,
 *      Matern 3/2: 3 sf2 e^-a, Matern 5/2: (5/3) sf2 (1 + a) e^-a) and s_c = 1 / l^2 (ARD: w_c^2),
 *        dk(z_j, x) / dz_jc = -H(z_j, x) (z_jc - x_c) s_c
 *        dF/dz_jc = -s_c sum_i G_uf[j,i] H(z_j,x_i) (z_jc - x_ic) - s_c sum_b (2 G_uu)[j,b] H(z_j,z_b) (z_jc - z_bc)
 *      (row j and column j of Kuu both move with z_j: the symmetric 2 G_uu has weight 1 here, not the 1/2 of the trace; the
 *      diagonal of Kuu and the jitter have no derivative; H is finite at zero distance and the difference exactly zero
 *      there, so a z_j on a data row is no special case).  One more O(N M d) rectangular pass per chunk on the weights the
 *      hyper-parameter gradient forms, differences before products, every sum in a fixed order; no N M^2 product is added.
 * cugp_sparse_create      : kernel CUGP_KERNEL_*; ard != 0: one length scale per dimension; jitter > 0 (1e-6 is customary);
 *                           chunk_rows 0 (the library's choice, 16384) or a multiple of 128.  m <= CUGP_SPARSE_MAX_M: the padded
 *                           m^2 stays below 2^31, so every element offset of the inner factorisation's kernels fits an int.
 * cugp_sparse_dims        : any pointer may be NULL; chunk_rows as resolved
 * cugp_sparse_set_data    : X [n][d], y [n], host; kept on the device.  cugp_sparse_set_inducing: Z [m][d], host.
 * cugp_sparse_set_loghyper / _get_loghyper: nh entries (nh must equal cugp_sparse_num_hyper), all zero after creation
 * cugp_sparse_bound       : *F <- the bound.  cugp_sparse_bound_grad: also g <- the nh components of the gradient of -F, in
 *                           cugp_loglik_grad's convention and order.  The results of one (data, Z, theta) are kept.
 * cugp_sparse_predict     : mean and var at nt test points (host), with_noise != 0 adds s2; the test points are taken in
 *                           passes of whole 128-row tiles (cugp_sparse_predict_plan's); it reuses the state of the last bound evaluation and evaluates
 *                           first when that is stale.
 * cugp_sparse_cg_solve    : the loop of cugp_cg_minimize_n on f = -F from the current hyper-parameters; the end point stays
 *                           set.  trace (may be NULL): rows of nh + 1 doubles [theta, f] of the ITERATES, as
 *                           cugp_cg_solve_loo records them (f never rises along it; the row behind the last is NaN where
 *                           trace_cap leaves room).  *nevals <- evaluations made.
 * cugp_sparse_bound_grad_z: cugp_sparse_bound_grad -- *F and g carry ITS bits -- and gZ [m][d] <- the gradient of -F with respect
 *                           to the inducing inputs, in cugp_sparse_set_inducing's layout.  Kept like the other results.
 * cugp_sparse_get_inducing: Z [m][d] <- the inducing inputs as the handle holds them.
 * cugp_sparse_cg_solve_z  : cugp_sparse_cg_solve's loop over the nh + m d variables [theta, vec Z] from the current state; the
 *                           end point stays set, theta and Z (read Z back with cugp_sparse_get_inducing).  trace: rows
 *                           [theta, f] (nh + 1 doubles) of the iterates, under cugp_sparse_cg_solve's rules; a probe whose
 *                           Kuu or B is not positive definite is a NaN probe to the loop.  CUGP_ERR_NOMEM when the partial
 *                           blocks of the Z pass cannot be allocated: the handle stays as it was.
 * cugp_sparse_plan        : the schedule, pure arithmetic (no device): pass i streams the rows [out[0], out[0] + out[1]),
 *                           padded to out[2] (a multiple of 128); its Gram launch splits the k range [0, out[2]) of every
 *                           output tile out[3] ways, split s taking [s out[4], min((s + 1) out[4], out[2])); returns the
 *                           number of passes, CUGP_ERR_INVALID for a pass beyond the last.
 * cugp_sparse_predict_plan: the passes cugp_sparse_predict takes nt test points in against m inducing inputs, pure arithmetic
 *                           (no device): pass i takes the test rows [out[0], out[0] + out[1]).  Every pass but the last has
 *                           the same number of rows: whole 128-row tiles whose three [rows][mpad] matrices (Ks, Wt, Vt; mpad:
 *                           m rounded up to 128) stay within 1 GiB, at most 2^20 rows (349440 rows at mpad 128).  Returns the
 *                           number of passes, CUGP_ERR_INVALID for m < 1, m > CUGP_SPARSE_MAX_M, nt <= 0, a NULL out or a
 *                           pass beyond the last.
 * Refusals, all CUGP_ERR_INVALID with the call's name in cugp_last_error before any device work: a NULL argument; n, d or
 * m < 1; m > CUGP_SPARSE_MAX_M; an unknown kernel kind; chunk_rows negative or not a multiple of 128; a jitter that is not
 * positive and finite; an nh that is not the handle's; nt <= 0; budget <= 0; an evaluation, prediction or solve before the
 * data or the inducing inputs are set.  CUGP_ERR_NODEVICE from cugp_sparse_create without a GPU.  A Kuu or B that is not
 * positive definite gives NaN results with CUGP_OK (the header's convention).
 * Not built: gradients with respect to Z of the predictions (the bound's: cugp_sparse_bound_grad_z); gradients of the joint
 * covariance or of draws (cugp_sparse_predict_cov, _sample and _grad are below); data sharded across GPUs (A A' and A y are
 * sums over rows: one all-reduce); FITC; a C++ mirror in cugp_amd/host/.
 *
 * ---- multi-target regression over one set of inducing points (the sparse sibling of cugp_set_targets; GPflow's SGPR takes
 *      Y [N, R]).  p targets y_1 .. y_p share the rows X, the hyper-parameters, the inducing inputs Z and the jitter; the
 *      objective is F = sum_t F_t, F_t the bound above for y_t.  Everything that costs O(N M^2) -- W_c = k(X_c, Z) Lu^-T,
 *      P = sum_c W_c'W_c, B = I + P / s2, its factor and inverse, the weight product, both trace passes -- does not depend on
 *      y and runs ONCE for all targets.  With Q = [q_1 .. q_p], q_t = sum_c W_c'y_t,c, C' = LB^-1 Q, Gamma' = LB^-T C',
 *      Beta' = Lu^-T Gamma' (one column per target):
 *        F_t = ((((-N/2 log 2 pi - sum log LB_ii) - N/2 log s2) - y_t'y_t / (2 s2)) + c'_t'c'_t / (2 s2^2)) - (N sf2 - tr P) / (2 s2)
 *        F = sum_t F_t, summed in target order
 *        H = p (I - B^-1) - sum_t gamma'_t gamma'_t' / s2^2,  H2 = H - p P / s2,  R = Lu^-T H / s2,  2 G_uu = Lu^-T H2 Lu^-1
 *        G_c' = W_c R' + sum_t y_t,c (beta'_t / s2^2)'   per chunk: the rank-one part becomes rank p
 *        g_c = -(S_uf,c + S_uu,c / 2),  g_f = -(2 (S_uf,nl + S_uu,nl / 2) - p N sf2 / s2)
 *        g_n = -(((p sum_i (1 - [B^-1]_ii) - p N) + (((sum_t y_t'y_t - sum_t c'_t'c'_t / s2) + p (N sf2 - tr P)) / s2)) - sum_t gamma'_t'gamma'_t / s2^2)
 *        gZ: the pass of cugp_sparse_bound_grad_z over the same G_c and 2 G_uu
 *        mean_t = Vt c'_t / s2, one row per target; the variance does not depend on y
 *      (S_uf, S_uu: the trace sums of the rectangle and of the square, as for one target).  Every sum has a fixed order, over
 *      the targets always ascending: equal inputs give equal bits, and F_t and mean_t of a target do not depend on how many
 *      targets there are or where it stands.
 * cugp_sparse_set_targets        : Y [p][n] target-major, host; kept on the device.  cugp_sparse_set_data is still required: it
 *                                  supplies X, and its y is unrelated to the targets.  Targets persist until replaced; a
 *                                  second call may change p.  p has no cap other than memory (CUGP_ERR_NOMEM: the handle is
 *                                  left without targets).
 * cugp_sparse_num_targets        : *p <- the number of targets, 0 before cugp_sparse_set_targets
 * cugp_sparse_bound_targets      : *F <- sum_t F_t, F_each (may be NULL) <- the p values F_t
 * cugp_sparse_bound_grad_targets : also g <- the nh components of the gradient of -F.  cugp_sparse_bound_grad_z_targets:
 *                                  also gZ [m][d] <- the gradient of -F with respect to the inducing inputs.
 * cugp_sparse_predict_targets    : mean [p][nt] target-major and var [nt] (may be NULL) at nt test points, in
 *                                  cugp_sparse_predict_plan's passes; var has the bits of cugp_sparse_predict at the same
 *                                  theta, Z and data: it reads nothing of y.
 * cugp_sparse_cg_solve_targets   : cugp_sparse_cg_solve (inducing == 0) or cugp_sparse_cg_solve_z (inducing != 0) on f = -F of
 *                                  the targets: the same loop, trace and end point.
 *      The single-target calls are untouched, in bits and in launches.  A targets evaluation writes the shared factor of B, so
 *      it makes the single-target results stale and the reverse: each is evaluated again when next asked for, with the same
 *      bits.  cugp_sparse_set_loghyper, _set_inducing, _set_data and _set_targets make the targets' results stale.
 *      Refusals, all CUGP_ERR_INVALID with the call's name in cugp_last_error before any device work: a NULL handle, Y or F;
 *      p < 1; cugp_sparse_set_targets before cugp_sparse_set_data; any targets call before cugp_sparse_set_targets or
 *      cugp_sparse_set_inducing; an nh that is not the handle's; nt <= 0; budget <= 0; a NULL Xt, mean, g or gZ where one is
 *      required.  A Kuu or B that is not positive definite gives NaN results with CUGP_OK.
 *      Not built for the targets: per-target hyper-parameters; leave-one-out over targets; reusing B between a single-target
 *      and a targets evaluation at equal theta; input gradients and draws per target (the joint covariance reads no y, so
 *      cugp_sparse_predict_cov's cov serves every target already).
 *
 * ---- joint predictive covariance, posterior draws and input gradients of the sparse model (the sparse siblings of
 *      cugp_predict_cov, cugp_predict_sample and cugp_predict_grad).  With Wt = k(Xt,Z) Lu^-T, Vt = Wt LB^-T, s2, sf2 as above,
 *      c' = LB^-1 q, gamma' = LB^-T c', beta' = Lu^-T gamma':
 *        mean = cugp_sparse_predict's, bit for bit (the same launch)
 *        cov  = k(Xt,Xt) - Wt Wt^T + Vt Vt^T   (+ s2 I with noise)     nt x nt row-major, the lower triangle mirrored:
 *               exactly symmetric; diag(cov) equals cugp_sparse_predict's variance up to rounding, not bit for bit (the
 *               summation orders differ).  The jitter eps of Kuu enters Lu alone: nothing of it is added to cov.
 *        samples[s nt + t] = mean[t] + sum_{k <= t} C[t][k] normals[s nt + k],  C = chol(cov + jitter I) by the library's
 *               blocked Cholesky (cugp_predict_sample's definition and launches); the normals are the caller's; a matrix
 *               that is not positive definite gives NaN with CUGP_OK.
 *        dk(x*, z_j) / dx*_c = -G_j (x*_c - z_jc) s_c,  G and s_c per family exactly as stated above cugp_predict_grad;
 *        a = beta' / s2                       (mean = sum_j a_j k_j -- the same number as Vt c' / s2)
 *        U = (Wt - Vt LB^-1) Lu^-1            (row t = Lu^-T (I - B^-1) Lu^-1 ks_t;  var_f = sf2 - ks_t^T U_t)
 *        dmean / dx*_c = -s_c sum_j a_j G_j (x*_c - z_jc)
 *        dvar  / dx*_c = +2 s_c sum_j U_tj G_j (x*_c - z_jc)
 *      a replaces the exact model's alpha and U its V; the tile pass and its finish are cugp_predict_grad's own kernels over
 *      (Z, m).  The noisy and the latent variance have the same gradient.  Sums run in a fixed order without atomics: the
 *      same bits on every call, and a row's gradient does not depend on nt.
 * cugp_sparse_predict_cov_plan: pure arithmetic, no device: out = {nt rounded up to 128, the product's tile edge (64 or
 *      128), the number of k ranges a tile's product is split into, their length} at the process's current tuning.
 *      CUGP_ERR_INVALID for m < 1, m > CUGP_SPARSE_MAX_M, nt <= 0, nt > CUGP_SPARSE_MAX_M (the padded nt^2 must fit an int
 *      in the factor handle's kernels, the reason m is capped), an nt beyond the first pass of cugp_sparse_predict_plan(m,
 *      nt, ..) (Wt and Vt must be whole), a NULL out.
 * cugp_sparse_predict_cov   : mean [nt] (may be NULL) and cov [nt][nt], host.  cugp_sparse_predict_sample: samples
 *      [nsamples][nt] from normals [nsamples][nt].  Both refuse exactly where the plan does.
 * cugp_sparse_predict_grad  : mean and var [nt] (either may be NULL; cugp_sparse_predict's bits for the same with_noise),
 *      dmean and dvar [nt][d] row-major (either may be NULL, not both; a NULL dvar skips U and its two triangular
 *      products); the test points go in cugp_sparse_predict_plan's passes: any nt.
 *      All three reuse the state of the last evaluation of the handle's own y and evaluate first when it is stale (new
 *      theta, Z or data, or a targets evaluation in between).  A Kuu or B that is not positive definite gives NaN outputs
 *      with CUGP_OK.  Refusals, all CUGP_ERR_INVALID with the call's name in cugp_last_error before any device work: those
 *      of cugp_sparse_predict; a jitter that is negative or not finite; nsamples <= 0; dmean and dvar both NULL. */
#define CUGP_SPARSE_MAX_M 32768
typedef struct cugp_sparse cugp_sparse;
int cugp_sparse_create(int n, int m, int d, int device, int kernel, int ard, double jitter, int chunk_rows, cugp_sparse **out);
int cugp_sparse_destroy(cugp_sparse *sp);
int cugp_sparse_dims(const cugp_sparse *sp, int *n, int *m, int *d, int *mpad, int *chunk_rows);
int cugp_sparse_num_hyper(const cugp_sparse *sp, int *nh);
int cugp_sparse_set_data(cugp_sparse *sp, const double *X /* [n][d], host */, const double *y /* n */);
int cugp_sparse_set_inducing(cugp_sparse *sp, const double *Z /* [m][d], host */);
int cugp_sparse_set_loghyper(cugp_sparse *sp, const double *hp, int nh);
int cugp_sparse_get_loghyper(const cugp_sparse *sp, double *hp, int nh);
int cugp_sparse_bound(cugp_sparse *sp, double *F);
int cugp_sparse_bound_grad(cugp_sparse *sp, double *F, double *g /* nh */, int nh);
int cugp_sparse_predict(cugp_sparse *sp, const double *Xt, int nt, int with_noise, double *mean /* nt */, double *var /* nt */);
int cugp_sparse_cg_solve(cugp_sparse *sp, int budget, double *trace, int trace_cap, int *nevals);
int cugp_sparse_plan(int n, int m, int chunk_rows, int pass, int out[5]);
int cugp_sparse_predict_plan(int m, int nt, int pass, int out[2]);
int cugp_sparse_bound_grad_z(cugp_sparse *sp, double *F, double *g /* nh */, int nh, double *gZ /* [m][d] */);
int cugp_sparse_get_inducing(const cugp_sparse *sp, double *Z /* [m][d] */);
int cugp_sparse_cg_solve_z(cugp_sparse *sp, int budget, double *trace, int trace_cap, int *nevals);
int cugp_sparse_set_targets(cugp_sparse *sp, const double *Y /* [p][n], target-major, host */, int p);
int cugp_sparse_num_targets(const cugp_sparse *sp, int *p);          /* 0 before set_targets */
int cugp_sparse_bound_targets(cugp_sparse *sp, double *F, double *F_each /* p, may be NULL */);
int cugp_sparse_bound_grad_targets(cugp_sparse *sp, double *F, double *g /* nh */, int nh, double *F_each);
int cugp_sparse_bound_grad_z_targets(cugp_sparse *sp, double *F, double *g, int nh, double *gZ /* [m][d] */, double *F_each);
int cugp_sparse_predict_targets(cugp_sparse *sp, const double *Xt, int nt, int with_noise,
                                double *mean /* [p][nt] */, double *var /* nt, may be NULL */);
int cugp_sparse_cg_solve_targets(cugp_sparse *sp, int budget, int inducing, double *trace, int trace_cap, int *nevals);
int cugp_sparse_predict_cov_plan(int m, int nt, int out[4]);
int cugp_sparse_predict_cov(cugp_sparse *sp, const double *Xt, int nt, int with_noise,
                            double *mean /* nt, may be NULL */, double *cov /* nt x nt */);
int cugp_sparse_predict_sample(cugp_sparse *sp, const double *Xt, int nt, int with_noise, double jitter,
                               int nsamples, const double *normals, double *samples);
int cugp_sparse_predict_grad(cugp_sparse *sp, const double *Xt, int nt, int with_noise,
                             double *mean /* nt, may be NULL */, double *var /* nt, may be NULL */,
                             double *dmean /* [nt][d], may be NULL */, double *dvar /* [nt][d], may be NULL */);

/* ---- stand-alone dense LA on a caller matrix (common/matrixops.h:5-25) ----
 * cugp_potrf        : get_cholesky            (L lower, upper zeroed)
 * cugp_potri        : compute_K_inverse
 * cugp_chol_and_det : compute_chol_and_det    (y'K^-1y, log|K|)
 * cugp_potrs_vec    : vector_Kinvy_using_cholesky */
int cugp_potrf(int n, const double *K, double *L, int device);
int cugp_potri(int n, const double *K, double *Kinv, int device);
int cugp_chol_and_det(int n, const double *K, const double *y, double *quad, double *logdet, int device);
int cugp_potrs_vec(int n, const double *K, const double *y, double *x, int device);

/* ---- timing: per-phase HIP-event times of the last evaluation (profiling must be on) ----
 * phases: 0 kernel build, 1 Cholesky, 2 triangular inverse, 3 K^-1 product, 4 vectors+traces+finalize, 5 total;
 * cugp_get_kernel_stats: HIP-event time of every launch of the Cholesky trailing update (MFMA SYRK) in the
 * evaluations since the last reset: sum of durations (ms), launches, algorithmic flop */
int cugp_set_profiling(cugp_gp *gp, int level /* 0 off, 1 phases, 2 phases + HIP events around a rotating sample of the
                                                 MFMA kernels' launches, 3 phases + events around every such launch,
                                                 4 phases + every such launch timed by its OWN start / stop events
                                                 (hipExtLaunchKernelGGL; the start event still sits in front of the
                                                 dispatch gap and the evaluation runs 3 % slower), 5 phases + every
                                                 such launch and the covariance build timed by its own workgroups:
                                                 first start / last end on the chip's 100 MHz clock in a device
                                                 buffer -- no events, the untimed schedule */);
int cugp_get_phase_ms(cugp_gp *gp, double ms[6]);
int cugp_get_kernel_stats(cugp_gp *gp, double *sum_ms, long long *launches, double *flop, int reset);
/* the same per kernel, as rocprofv3 names them: kind 0 = k_syrk_step (near-window update + next diagonal block,
 * K = 128; timed one launch in 16, rotating), 1 = k_syrk_wide (the far trailing matrix once per panel, K = 128 * panel
 * width), 2 / 3 = k_trtri_border<4> / <2> (bordering steps of L^-1) and 4 / 5 = k_lauum<4> / <2> (shares of K^-1):
 * timed for every fourth block of inverse rows, 6 / 7 = k_trtri_level<4> / <2> (doubling inside a block of rows; timed
 * one launch in 16), 8 = k_trtri_block (a hand-over block's own inverse in one launch; every fourth block), 9 =
 * k_predict_gemm (W = Ks L^-T of cugp_predict; levels 3 to 5 only), 10 = k_build (level 5 only; its `flop` is BYTES: the
 * lower 64x64 tiles of K written once + X read), 12 = k_predict_cov<4> / <2> (W W^T of cugp_predict_cov and
 * cugp_predict_sample; levels 3 to 5 only; flop: every launched output tile over the whole k range), 13 = k_predict_grad
 * (the tile pass of cugp_predict_grad; levels 3 and 4 only; its `flop` is BYTES: the tiles of Ks and, with dvar, V it reads).
 * 14 = k_loo_product<4> / <2> (P = B B^T of cugp_loo's gradient; levels 2 to 4, every launch).
 * cugp_predict_grad's second triangular product V = W L^-1 (k_targets_alpha) is counted under kind 9 (levels 3 and 4).  The
 * sampling rates are those of level 2; levels 3 to 5 time every launch.  flop = algorithmic
 * (entries on or below the diagonal, a triangular k tile counted half), multiply + add */
int cugp_get_kernel_stats_kind(cugp_gp *gp, int kind, double *sum_ms, long long *launches, double *flop, int reset);
/* level 5 only: the durations of the same launches counted from the END of the launch directly in front of each on its
 * stream (kind 11 = k_trsm_inv64 -> [k_syrk_wide] -> k_syrk_step on the factorisation's stream), where rocprofv3
 * --kernel-trace puts the begin of an in-order dispatch -- the launch's wait for its first workgroup slot included;
 * launches without a stamped predecessor count from their first workgroup.  Read before a resetting call above. */
int cugp_get_kernel_stats_dispatch_ms(cugp_gp *gp, int kind, double *sum_ms);
void *cugp_get_stream(cugp_gp *gp);          /* hipStream_t of the handle */

/* ---- optimisers (host logic): Covsum::cg_solve covkernel.cpp:405-647 == cg_solve(BCM)
 *      distributed_gp/distributed_ver1.cpp:13-232 == cg_solve(char*) cuda_scalingdist/cg_solver.cpp:292-523 ;
 *      Covsum::rprop_solve covkernel.cpp:337-402 ----
 * fn fills f = -LL and g = d(-LL)/d(theta) at theta (both, at every probe, as the reference does).
 * trace (may be NULL): rows [theta0, theta1, theta2, f] per evaluation.  *nevals <- evaluations made. */
typedef void (*cugp_objective_fn)(void *ctx, const double theta[3], double *f, double g[3]);
int cugp_cg_minimize(cugp_objective_fn fn, void *ctx, double theta[3], int budget, double *trace, int trace_cap,
                     int *nevals);
int cugp_rprop_minimize(cugp_objective_fn fn, void *ctx, double theta[3], int iters, double *trace, int trace_cap,
                        int *nevals);
/* Opt-in, evaluation-sparing form of the same loop: the objective comes in two halves, the value
 * and -- only where the line search can use it -- the gradient at the point of the last value call.  A probe whose
 * value is above the line search's starting value (or NaN/Inf) never has its gradient read by covkernel.cpp:405-647,
 * so it is not computed: on the GPU that probe costs the factorisation only (N^3/3 instead of N^3).  *ngrads <-
 * gradient evaluations made.  The default entry points keep the reference's "both at every probe". */
typedef void (*cugp_value_fn)(void *ctx, const double theta[3], double *f);
typedef void (*cugp_gradient_fn)(void *ctx, const double theta[3], double g[3]);
int cugp_cg_minimize_sparing(cugp_value_fn value, cugp_gradient_fn gradient, void *ctx, double theta[3], int budget,
                             double *trace, int trace_cap, int *nevals, int *ngrads);
int cugp_cg_solve_sparing(cugp_gp *gp, int budget, double *trace, int trace_cap, int *nevals, int *ngrads);
/* The same conjugate-gradient loop over nh hyper-parameters (no reference counterpart; used for ARD handles, theta
 * ordered as GPML's covSEard above): same constants and control flow, every sum over the entries in index order, so
 * with nh == 3 it takes the 3-entry trajectory bit for bit.  The objective fills f = -LL and the nh entries of g.
 * trace (may be NULL): rows of nh + 1 doubles [theta_0 .. theta_{nh-1}, f].  CUGP_ERR_INVALID for a NULL fn or theta,
 * nh <= 0 or budget < 0.  The solve form below runs it on an ARD handle from its current hyper-parameters and leaves
 * the end point set (CUGP_ERR_INVALID on an isotropic handle). */
typedef void (*cugp_objective_n_fn)(void *ctx, const double *theta, int nh, double *f, double *g);
int cugp_cg_minimize_n(cugp_objective_n_fn fn, void *ctx, double *theta, int nh, int budget, double *trace,
                       int trace_cap, int *nevals);
int cugp_cg_solve_ard(cugp_gp *gp, int budget, double *trace, int trace_cap, int *nevals);
int cugp_cg_solve(cugp_gp *gp, int budget, double *trace, int trace_cap, int *nevals);
int cugp_rprop_solve(cugp_gp *gp, int iters, double *trace, int trace_cap, int *nevals);

/* ---- BCM / product of experts on one GPU: class BCM distributed_gp/BCM.h:2-27 ----
 * The experts given to one cugp_bcm are the ones resident on this process's GPU; their evaluations run
 * concurrently on separate HIP streams.  Sums over the experts of OTHER GPUs are the caller's all-reduce
 * (cugp_amd.bcm does it over RCCL; the reference: cuda_scalingdist/cg_solver.cpp:72-213).
 * cugp_bcm_create_split : BCM::BCM(X,y,N,D,K) BCM.cpp:85-110 (contiguous floor(N/K) rows, remainder to the last)
 * cugp_bcm_loglik_grad  : get_BCM_loglikelihood BCM.cpp:182-198 + get_BCM_gradient_hyper :153-180 -> sums in
 *                         expert order; per_expert_ll may be NULL
 * cugp_bcm_predict_partial : per-expert compute_test_means_and_variances, reduced to the two PoE sums
 *                         sum_k 1/v_k and sum_k mu_k/v_k (BCM.cpp:45-62); cugp_poe_finish turns (all-reduced)
 *                         sums into mean / variance */
int cugp_bcm_create(int nexperts, const int *rows, int d, int device, cugp_bcm **out);
/* the same over several GPUs of ONE process: expert k on devices[k mod ndev] (chunk i -> worker i mod W,
 * cuda_scalingdist/cg_solver.cpp:93), all devices in flight at once, sums in expert order on the host -- the
 * C++ class BCM (cugp_amd/host/BCM.h) uses the whole node through this.  Listing a device twice is allowed. */
int cugp_bcm_create_multi(int ndev, const int *devices, int nexperts, const int *rows, int d, cugp_bcm **out);
int cugp_bcm_create_split_multi(const double *X, const double *y, int N, int D, int K, int ndev, const int *devices,
                                cugp_bcm **out);
int cugp_bcm_create_split(const double *X, const double *y, int N, int D, int K, int device, cugp_bcm **out);
/* the two _multi forms with every expert of covariance family `kernel` (CUGP_KERNEL_*; 0 = the calls above, bit for
 * bit; an unknown kind: CUGP_ERR_INVALID before any device call); cugp_bcm_kernel_kind reports it */
int cugp_bcm_create_kernel(int ndev, const int *devices, int nexperts, const int *rows, int d, int kernel, cugp_bcm **out);
int cugp_bcm_create_split_kernel(const double *X, const double *y, int N, int D, int K, int ndev, const int *devices,
                                 int kernel, cugp_bcm **out);
int cugp_bcm_kernel_kind(const cugp_bcm *b, int *kernel);
int cugp_bcm_destroy(cugp_bcm *b);
int cugp_bcm_num_experts(const cugp_bcm *b, int *k);
int cugp_bcm_expert(cugp_bcm *b, int k, cugp_gp **gp);
int cugp_bcm_set_expert_data(cugp_bcm *b, int k, const double *X, const double *y);
int cugp_bcm_set_loghyper(cugp_bcm *b, const double hp[3]);      /* BCM::set_BCM_log_hyperparam BCM.cpp:123-130 */
int cugp_bcm_get_loghyper(const cugp_bcm *b, double hp[3]);
int cugp_bcm_loglik_grad(cugp_bcm *b, double *ll, double g[3], double *per_expert_ll);
/* rows[k][4] = {LL_k, dLL_k/dtheta (as gradients of -LL)} per expert of this device: the payload a multi-device
 * BCM sums across devices (the two gathers of cuda_scalingdist/cg_solver.cpp:72-213 in one buffer) */
int cugp_bcm_loglik_grad_rows(cugp_bcm *b, double *rows);
/* the same rows left in DEVICE memory for a collective that stays on the device (RCCL all-reduce): row slot[k] of
 * dev_rows ([.][4] doubles on the handle's device) receives local expert k's {LL, g}; single-device handles */
int cugp_bcm_loglik_grad_rows_device(cugp_bcm *b, double *dev_rows, const int *slot);
/* ---- the same exchange done by the library, one process per GPU (RCCL over xGMI) ----
 * replaces: the master's worker-by-worker collection of log-likelihoods and gradients over TCP,
 * cuda_scalingdist/cg_solver.cpp:72-213 (and the hyper-parameter broadcast :245-279, which is not needed: every rank
 * runs the same deterministic optimiser on identical sums).  Expert k lives on rank k mod W (cg_solver.cpp:93).
 * cugp_comm_unique_id: rank 0 obtains the 128-byte id and hands it to the other ranks by any means (the Python layer
 * broadcasts it through torch.distributed, tests/cpp/rccl_driver.cpp through a file); cugp_comm_create: collective
 * over all ranks (id == NULL with world == 1: no communicator, nothing to exchange).  RCCL is opened at run time
 * (librccl.so.1): CUGP_ERR_NODEVICE when it cannot be.
 * cugp_bcm_loglik_grad_allgather: evaluate this rank's experts (b; NULL on a rank that owns none) and gather
 * everybody's rows: rows_out[world * per][4], rank r's i-th expert (global expert r + i * world) in row r * per + i as
 * {LL, g[3]}, zeros in slots beyond a rank's experts; per >= the largest number of experts on a rank.  Evaluation,
 * ncclAllGather and the copy to the host are one in-order sequence on the evaluation's stream: one host wait. */
typedef struct cugp_comm cugp_comm;
int cugp_comm_unique_id(void *id, int bytes);        /* bytes must be 128 */
int cugp_comm_create(const void *id, int bytes, int rank, int world, int device, cugp_comm **out);
int cugp_comm_destroy(cugp_comm *c);
int cugp_bcm_loglik_grad_allgather(cugp_bcm *b, cugp_comm *c, int per, double *rows_out);
int cugp_bcm_predict_partial(cugp_bcm *b, const double *Xt, int nt, double *sum_prec, double *sum_prec_mean);
int cugp_poe_finish(const double *sum_prec, const double *sum_prec_mean, int nt, double *mean, double *var);
int cugp_bcm_predict(cugp_bcm *b, const double *Xt, int nt, double *mean, double *var); /* BCM.cpp:64-83 */
/* cugp_bcm_predict_allgather: product-of-experts prediction of a BCM sharded one process per GPU --
 * distributed_gp/BCM.cpp:45-83 (sum_k 1/v_k and sum_k mu_k/v_k in expert order k = 0..nexperts-1, then v = 1/sum,
 * mu = v * sum) across ranks; the reference never runs it multi-process (cuda_scalingdist/main.cpp:309 comments its
 * testing_phase out).  b: this rank's experts (global experts rank, rank + W, ... in that order; NULL on a rank that
 * owns none), all on c's device.  Every rank predicts its experts (one group of batched launches where their shapes
 * allow it; stale experts first brought up to date by one evaluation) and sends {status, local expert count,
 * [per][2][nt] rows} by ONE ncclAllGather on a stream the communicator owns; the product of experts is taken on the
 * device and copied to mean[nt], var[nt] with one host wait.  Bit-identical to cugp_bcm_predict over the same experts in
 * one process.  A world of one without an id: no RCCL.
 * Callers MUST pass the same per, nexperts, nt and Xt on every rank: the library cannot check that without a collective.
 * Errors:
 *  - c NULL, nt <= 0, Xt / mean / var NULL, per <= 0, nexperts <= 0 or per * world < nexperts: CUGP_ERR_INVALID on
 *    every rank alike, before any collective;
 *  - every other failure of a rank (a local expert count that is not ceil((nexperts - rank) / world), a BCM on another
 *    device, an evaluation or HIP error) still joins the collective with a nonzero status word and NaN rows; every rank
 *    reads every rank's status word and the sum of the local counts, and ALL ranks return the same code (the first
 *    failing rank's), with mean / var set to NaN and cugp_last_error naming the failing rank;
 *  - only a failure to allocate the exchange buffers themselves (first call, or a larger nt / per) returns at once,
 *    without joining the collective. */
int cugp_bcm_predict_allgather(cugp_bcm *b, cugp_comm *c, int per, int nexperts, const double *Xt, int nt,
                               double *mean, double *var);
int cugp_bcm_cg_solve(cugp_bcm *b, int budget, double *trace, int trace_cap, int *nevals);
/* ---- the sparse variational model (cugp_sparse_*) with its DATA ROWS sharded over ranks: K shards hold disjoint row
 *      blocks (X_k, y_k), n_k >= 1 each and unequal where the caller likes, of ONE data set of N = sum n_k rows; Z, the
 *      hyper-parameters, kernel, ard, jitter and m are the same on every shard.  Shard k lives on rank k mod W in slot k / W
 *      of that rank (per = ceil(K / W) slots; K >= W: every rank owns a shard).  The objective is the bound F of all N rows
 *      and the gradients of -F: what cugp_sparse_bound_grad_z returns for the concatenated data -- one coherent model, not a
 *      product of experts.  Own y only: no targets.
 * One evaluation is cugp_sparse_bound*'s sequence cut at the two points where the shards meet:
 *   1  every local shard's chunk loop writes P_k = sum W_c'W_c, q_k = sum W_c'y_c, y_k'y_k and n_k into its slot;
 *      ONE ncclAllGather of [header | per slots] on the evaluation's stream; the slots are summed in GLOBAL SHARD ORDER
 *      k = 0 .. K - 1 (first term copied, then a = a + b; no atomics, never ncclAllReduce): every rank holds P, q, y'y and N
 *      with the same bits, and those depend on (data, K), not on W or per.  Then B, its factorisation and the small solves
 *      as cugp_sparse_bound's, on every rank alike.
 *   2  (what >= 1) every local shard's trace passes give its row [S_uf,k (nh - 1) | gZ_uf,k (m d; what == 2)]; ONE
 *      ncclAllGather of the rows, the same sum in shard order, the square's passes and the final sums.
 * With K = 1 every sum hands the one shard's numbers on: F, g, gZ and the predictions are bit for bit cugp_sparse_bound*'s
 * and cugp_sparse_predict*'s of an ordinary handle over the same data.  No host wait beyond those two of
 * cugp_sparse_bound_grad.
 * The header of exchange 1 carries the rank's status, its shard count, m, d, kernel, ard, nh, K, per, what, the bits of the
 * jitter and a fingerprint of the bits of the hyper-parameters and of Z.  A rank's own failure still joins exchange 1
 * (nonzero status, all-ones slots); behind the wait in front of B's factorisation every rank reads every rank's header, and
 * on a nonzero status, a mismatch or shard counts that do not add up to K ALL ranks return the same error naming the rank
 * and none enters exchange 2.  Everything later is decided from bits every rank holds alike: Kuu or B not positive
 * definite (NaN results with CUGP_OK, every rank), a NaN in one shard's data (P is NaN everywhere: NaN results, every rank).
 * cugp_sparse_create_shard : cugp_sparse_create for shard `shard` of `nshards` with n_local rows.  On such a handle
 *      set_data, set_inducing, set_loghyper, the get_ calls, dims and plan work as they stand; cugp_sparse_bound*,
 *      cugp_sparse_cg_solve*, cugp_sparse_set_targets and the _targets calls return CUGP_ERR_INVALID and name
 *      cugp_sparse_sharded_bound_grad.  After a sharded evaluation the FIRST local shard (the lead) holds the global M
 *      side: cugp_sparse_predict, _predict_cov, _predict_sample and _predict_grad run on it as they stand and add nothing
 *      to the collectives.  On another shard, or on a lead whose state is stale (the hyper-parameters, Z or the data of any
 *      local shard changed since), they return CUGP_ERR_INVALID: they never evaluate -- the local rows alone would be a
 *      different model.  (A change on another rank's shard cannot be seen from here: evaluate on every rank alike.)
 * cugp_sparse_shard_info   : membership; nshards = 0 (shard = -1, rows_total = 0) on an ordinary handle.  rows_total: N
 *      of the last sharded evaluation the handle took part in, 0 before.
 * cugp_sparse_sharded_bound_grad : one evaluation.  shards[nlocal]: this rank's shards in slot order (global shards rank,
 *      rank + W, ...), all on comm's device; comm: cugp_comm_create's, a world of one without an id included (no RCCL);
 *      what: 0 F, 1 F and g[nh], 2 F, g[nh] and gZ[m d].  Every rank passes the same per, nshards and what.
 *      CUGP_ERR_INVALID on every rank alike, before any collective: comm / shards / F NULL, g (what >= 1) or gZ (what == 2)
 *      NULL, nlocal < 1, per < 1, nshards < world, per * world < nshards, what outside 0..2.  A first handle that is NULL or
 *      no shard handle returns at once too (the rank cannot size its block).  Everything else -- an ordinary or NULL handle
 *      further down the list, local shards that disagree in m, d, kernel, ard, jitter, the bits of the hyper-parameters
 *      or of Z (refused before any launch), a wrong local count or shard index, missing data, nh not the handle's, a
 *      failure to allocate one of the handles' buffers, a HIP error of the evaluation -- is the rank's status.
 *      What the header cannot turn into a clean error: (a) per and the PADDED m (m rounded up to 128) size the block a rank
 *      sends, and ncclAllGather with counts that differ between ranks is undefined (a hang, or a write beyond the receive
 *      block) -- callers MUST pass the same per and m everywhere; the header catches a per or m that differs only where the
 *      counts happen to agree, and d, kernel, ard, nh, K, what, the jitter, the hyper-parameters and Z always; (b) a failure
 *      to allocate the COMMUNICATOR's own exchange blocks (first call, or a larger per / m / what), or of hipSetDevice,
 *      returns at once without joining exchange 1, and the other ranks wait: as cugp_bcm_predict_allgather's.
 * cugp_sparse_sharded_cg_solve : cugp_sparse_cg_solve's (inducing == 0) or cugp_sparse_cg_solve_z's (otherwise) loop on the
 *      sharded objective, run by every rank on identical numbers: identical trajectories by construction.  The start is
 *      the first local shard's state and is written nowhere: local shards that disagree in the hyper-parameters or Z are
 *      refused as cugp_sparse_sharded_bound_grad refuses them.  An evaluation that fails gives the loop NaN and the loop goes
 *      on (the ranks stay in step), but the call then returns that first failure's code and text -- a failed rank, a
 *      mismatch between ranks -- and writes nothing into the shards; not positive definite is no failure (NaN, CUGP_OK).
 *      Otherwise the end point and a moved Z are written into every local shard; trace, trace_cap and nevals as there. */
int cugp_sparse_create_shard(int n_local, int m, int d, int device, int kernel, int ard, double jitter, int chunk_rows,
                             int shard, int nshards, cugp_sparse **out);
int cugp_sparse_shard_info(const cugp_sparse *sp, int *shard, int *nshards, long long *rows_total);
int cugp_sparse_sharded_bound_grad(cugp_sparse *const *shards, int nlocal, cugp_comm *comm, int per, int nshards, int what,
                                   double *F, double *g, int nh, double *gZ);
int cugp_sparse_sharded_cg_solve(cugp_sparse *const *shards, int nlocal, cugp_comm *comm, int per, int nshards, int budget,
                                 int inducing, double *trace, int trace_cap, int *nevals);
/* ---- combination rules for the experts' predictions.  The reference has no counterpart: cugp_bcm_predict keeps its plain
 *      product of the experts' NOISY predictive distributions (BCM.cpp:45-62), whose variance falls to prior / K away from
 *      the data and below sn2 near it.  The rules below combine the experts' LATENT distributions N(m_k, var_f,k),
 *      var_f,k = sf2 - |W_t|^2 (cugp_predict_latent), with p_k = 1 / var_f,k and the latent prior variance sf2 = exp(2 theta_f)
 *      (k(x, x) - sn2 = sf2 for every family):
 *        CUGP_COMBINE_POE   beta_k = 1,                   prec = sum p_k                      product of experts
 *        CUGP_COMBINE_GPOE  beta_k = 1 / K,               prec = sum beta_k p_k               Cao & Fleet 2014, generalised PoE
 *        CUGP_COMBINE_BCM   beta_k = 1,                   prec = sum p_k + (1 - K) / sf2      Tresp 2000, Bayesian committee machine
 *        CUGP_COMBINE_RBCM  beta_k = 1/2 log(sf2 p_k),    prec = sum beta_k p_k + (1 - sum beta_k) / sf2
 *                                                                                             Deisenroth & Ng 2015, robust BCM
 *        var_f = 1 / prec,  mean = var_f sum beta_k p_k m_k,  var = var_f (+ sn2 when with_noise)
 *      CUGP_COMBINE_POE therefore combines LATENT distributions and differs from cugp_bcm_predict, which keeps the
 *      reference's noisy product.  Arithmetic, per test point, experts in global order, every operation rounded on its own
 *      (no contraction): sp += beta_k p_k; spm += beta_k pm_k (pm_k = p_k m_k, rounded when the row is made); sb += beta_k;
 *      prec = sp, or sp + (1 - sb) / sf2; tv = 1 / prec; mean = tv spm; the gPoE weight is RN(1 / K), computed once.
 *      var_f,k <= sf2, so beta_k >= 0 and prec >= 1 / sf2 for BCM and rBCM.  A var_f,k that is not positive, or NaN,
 *      propagates by IEEE: NaN / inf results with CUGP_OK (the header's convention).
 * cugp_poe_combine: the rule on caller rows [K][2][nt] (expert k: p_k at rows[k][0][t], pm_k at rows[k][1][t]); pure host
 *      code, no device.  It is the twin of the device kernel k_poe_reduce_mode: the same operations in the same order, so
 *      modes POE, GPOE and BCM (no transcendental) agree with the device bit for bit; RBCM uses each side's own log and
 *      agrees to rounding.
 * cugp_bcm_predict_mode: all experts of b at Xt.  Stale experts are refreshed as cugp_bcm_predict refreshes them.  One
 *      device set: latent rows by one group of batched launches, the rule on the device, one copy, one host wait.
 *      Several device sets of one process: the experts' latent predictions into pinned host memory, then cugp_poe_combine.
 * cugp_bcm_predict_allgather_mode: cugp_bcm_predict_allgather (above: same arguments, same ONE ncclAllGather, one host
 *      wait, same status protocol and error rules) with latent rows and the rule on the device.  sf2 and sn2 are arguments
 *      because a rank that owns no expert has no BCM to read them from: every rank passes exp(2 theta_f), exp(2 theta_n).
 * All work for isotropic BCMs of every kernel kind and for ARD BCMs.  CUGP_ERR_INVALID -- before any device call or
 * collective -- for an unknown mode, a NULL argument, K <= 0 or nt <= 0. */
#define CUGP_COMBINE_POE 0
#define CUGP_COMBINE_GPOE 1
#define CUGP_COMBINE_BCM 2
#define CUGP_COMBINE_RBCM 3
int cugp_poe_combine(const double *rows /* [K][2][nt] */, int K, int nt, int mode, double sf2, double sn2, int with_noise,
                     double *mean, double *var);
int cugp_bcm_predict_mode(cugp_bcm *b, const double *Xt, int nt, int mode, int with_noise, double *mean, double *var);
int cugp_bcm_predict_allgather_mode(cugp_bcm *b, cugp_comm *c, int per, int nexperts, const double *Xt, int nt, int mode,
                                    int with_noise, double sf2, double sn2, double *mean, double *var);
/* ---- gradients of the combined prediction with respect to the test inputs (one process; the reference has no
 *      counterpart).  The chain rule of the rules above, per test point and input dimension, experts in order, every
 *      operation rounded on its own, with p = 1 / v:
 *        dp = -dv / v^2;  dbeta = 0 (POE, GPOE, BCM) | -1/2 dv / v (RBCM)
 *        dprec = sum (dbeta p + beta dp) - [BCM, RBCM] (sum dbeta) / sf2,      dvar = -dprec / prec^2
 *        dS = sum (dbeta p m + beta dp m + beta p dm),   S = sum beta p m,      dmean = dvar S + dS / prec
 *      dmean is evaluated as the same expression with the difference m_k - mean formed first (dvar S and dS / prec cancel
 *      where the experts agree):  sum w_k dm_k + (sum a_k (m_k - mean)) / prec + [BCM, RBCM] mean ((sum dbeta) / sf2) / prec,
 *      a_k = dbeta p + beta dp,  w_k = beta_k p_k / prec,  mean = sum w_k m_k; one expert under POE returns its own gradients.
 * cugp_poe_combine_grad: pure host code, like cugp_poe_combine.  mean, var [K][nt]: the experts' means and variances
 *      (LATENT ones for the rules, as cugp_predict_grad returns them with with_noise = 0); dmean, dvar [K][nt][d] their
 *      gradients; out_dmean, out_dvar [nt][d].  CUGP_COMBINE_REFERENCE (-1): the reference's product of the experts' NOISY
 *      predictions (cugp_bcm_predict, BCM.cpp:45-62): POE's arithmetic on noisy variances, which the caller passes.
 *      CUGP_ERR_INVALID for a NULL argument, K <= 0, nt <= 0, d <= 0 or an unknown mode.
 * cugp_bcm_predict_grad: every expert's mean, variance and gradients, combined on the host.  Per device set the experts
 *      run as ONE group of batched launches (one launch per pass and kernel, the expert a grid dimension) where they can
 *      -- equal padded size, equal hyper-parameters, profiling below level 3 --, else expert by expert by
 *      cugp_predict_grad's own launches; either way every expert of every device set is in flight before the first wait,
 *      and the rows of a set reach pinned host memory by one copy (a BCM over several devices of one process works).
 *      Rows of one expert: [m nt | v nt | dmean nt*d | dvar nt*d], (2 + 2 d) nt doubles; m, v carry cugp_predict's bits
 *      (mode -1) or cugp_predict_latent's, the gradients cugp_predict_grad's.  mean, var (either may be NULL): from rows made
 *      as the device makes them, through cugp_poe_combine -- cugp_bcm_predict_mode's values, bit for bit except RBCM's log
 *      -- or, mode -1, through cugp_poe_finish: cugp_bcm_predict's bits (with_noise is then not read).  dmean, dvar [nt][d]
 *      (either may be NULL, not both; the experts' dvar is computed either way: the mean's gradient reads it).  The results
 *      do not depend on which of the two paths ran.  CUGP_ERR_INVALID -- before any device call -- for a NULL b or Xt,
 *      nt <= 0, dmean and dvar both NULL or an unknown mode.
 * cugp_bcm_predict_grad_form: how the last cugp_bcm_predict_grad (or cugp_bcm_predict_grad_allgather) on b ran: 0 no call
 *      yet, 1 expert by expert, 2 every device set as a group.  CUGP_ERR_INVALID for a NULL b or form.
 * cugp_bcm_predict_grad_allgather: the form across ranks, cugp_bcm_predict_allgather's sequence and rules (above) with
 *      gradient rows: every rank sends {status, local expert count, [per] slots of (2 + 2 d) nt doubles -- its i-th
 *      expert's rows [m nt | v nt | dmean nt*d | dvar nt*d] in slot i} by ONE ncclAllGather on the communicator's stream;
 *      the kernel k_poe_reduce_grad, device twin of the host path of cugp_bcm_predict_grad (one thread per test point and
 *      dimension, experts in GLOBAL order, the same operations in the same order), leaves [mean nt | var nt | dmean nt*d |
 *      dvar nt*d | world x {status, count}]; one copy, one host wait.  Modes CUGP_COMBINE_REFERENCE .. CUGP_COMBINE_RBCM;
 *      the results carry cugp_bcm_predict_grad's bits except RBCM's, whose log is the device's (agreement to rounding).
 *      d, sf2 = exp(2 theta_f) and sn2 = exp(2 theta_n) are arguments because a rank that owns no expert passes b == NULL.
 *      mean, var: nt each, either may be NULL; dmean, dvar: [nt][d], either may be NULL, not both -- and whether dvar is
 *      given must be the same on every rank (the caller's duty, like Xt).  A world of one without an id uses no RCCL.
 *      Refusals, CUGP_ERR_INVALID before any collective or device call with the call's name in cugp_last_error, for what
 *      every rank detects from the shared arguments: NULL c or Xt; nt, d, per or nexperts <= 0; per * world < nexperts; an
 *      unknown mode; dmean and dvar both NULL; d different from a non-NULL b's.  Every other failure is local: the rank
 *      still joins the collective with a nonzero status word and NaN rows, every rank reads every rank's status and ALL
 *      return the same code, with all four outputs NaN; BCM and communicator stay usable. */
#define CUGP_COMBINE_REFERENCE (-1)
int cugp_poe_combine_grad(const double *mean, const double *var,       /* [K][nt] each */
                          const double *dmean, const double *dvar,     /* [K][nt][d] each */
                          int K, int nt, int d, int mode, double sf2,
                          double *out_dmean, double *out_dvar);        /* [nt][d] each */
int cugp_bcm_predict_grad(cugp_bcm *b, const double *Xt, int nt, int mode, int with_noise,
                          double *mean, double *var, double *dmean, double *dvar);
int cugp_bcm_predict_grad_form(const cugp_bcm *b, int *form);
int cugp_bcm_predict_grad_allgather(cugp_bcm *b, cugp_comm *c, int per, int nexperts, const double *Xt, int nt, int d,
                                    int mode /* CUGP_COMBINE_REFERENCE .. CUGP_COMBINE_RBCM */, int with_noise,
                                    double sf2, double sn2,
                                    double *mean, double *var,     /* nt each, either may be NULL */
                                    double *dmean, double *dvar);  /* [nt][d], either may be NULL, not both */
/* ---- ARD BCM: every expert an ARD handle (squared exponential, or through the _ard_kernel calls a Matern kind; theta
 *      as cugp_create_ard's: nh = d + 2 entries shared by all experts).  The reference has no counterpart.  The experts
 *      run as groups of shared launches, over several
 *      devices of one process, or sharded one process per GPU, exactly like isotropic experts; only the rows of an
 *      evaluation are wider: {LL_k, g_k[nh]}, 1 + nh doubles, sums in expert order on the host.
 * An ARD BCM is ARD for life.  cugp_bcm_num_hyper reports nh (3, or d + 2) for any BCM.  Data, cugp_bcm_expert, the
 * three predict calls (their rows do not depend on nh) and cugp_bcm_kernel_kind work on it unchanged.  The _ard_kernel
 * create calls take the experts' kind directly in front of out (kind 0: the _ard calls; unknown: CUGP_ERR_INVALID).
 * cugp_bcm_cg_solve_ard: the loop of cugp_cg_minimize_n from the current hyper-parameters; trace rows of nh + 1 doubles.
 * cugp_bcm_loglik_grad_allgather_ard: rows_out[world * per][1 + nh]; nh is explicit because a rank that owns no expert
 *      passes b == NULL; still one all-gather on the evaluation's stream and one host wait.
 * Refusals, all CUGP_ERR_INVALID before any device call, with the call to use in cugp_last_error: the 3-entry calls
 * (set / get of the hyper-parameters, cugp_bcm_loglik_grad, the rows calls, the all-gather, cugp_bcm_cg_solve) on an ARD
 * BCM; the _ard calls on an isotropic BCM; a NULL argument; nh != d + 2.  The BCM stays usable after each of them. */
int cugp_bcm_create_ard(int ndev, const int *devices, int nexperts, const int *rows, int d, cugp_bcm **out);
int cugp_bcm_create_split_ard(const double *X, const double *y, int N, int D, int K, int ndev, const int *devices,
                              cugp_bcm **out);
int cugp_bcm_create_ard_kernel(int ndev, const int *devices, int nexperts, const int *rows, int d, int kernel,
                               cugp_bcm **out);
int cugp_bcm_create_split_ard_kernel(const double *X, const double *y, int N, int D, int K, int ndev,
                                     const int *devices, int kernel, cugp_bcm **out);
/* every expert a rational quadratic handle (cugp_create_rq; ard as there): nh = d + 3 or 4, rows {LL, g[nh]}, every
 * cugp_bcm_*_ard call, the four combination rules, cugp_bcm_predict_grad and the three all-gather exchanges with the BCM's
 * nh.  cugp_bcm_kernel_kind reports CUGP_KERNEL_RQ.  CUGP_ERR_INVALID before any device call, the call's name in
 * cugp_last_error: a NULL argument, a count that is not positive, K > N, ard outside {0, 1}. */
int cugp_bcm_create_rq(int ndev, const int *devices, int nexperts, const int *rows, int d, int ard, cugp_bcm **out);
int cugp_bcm_create_split_rq(const double *X, const double *y, int N, int D, int K, int ndev, const int *devices,
                             int ard, cugp_bcm **out);
int cugp_bcm_num_hyper(const cugp_bcm *b, int *nh);
int cugp_bcm_set_loghyper_ard(cugp_bcm *b, const double *hp, int nh);
int cugp_bcm_get_loghyper_ard(const cugp_bcm *b, double *hp, int nh);
int cugp_bcm_loglik_grad_ard(cugp_bcm *b, double *ll, double *g, int nh, double *per_expert_ll /* may be NULL */);
int cugp_bcm_loglik_grad_rows_ard(cugp_bcm *b, double *rows, int nh);
int cugp_bcm_loglik_grad_rows_device_ard(cugp_bcm *b, double *dev_rows, const int *slot, int nh);
int cugp_bcm_loglik_grad_allgather_ard(cugp_bcm *b, cugp_comm *c, int per, int nh, double *rows_out);
int cugp_bcm_cg_solve_ard(cugp_bcm *b, int budget, double *trace, int trace_cap, int *nevals);

/* ---- test / bench hooks ---- */
int cugp_test_gemm_nt(int m, int n, int k, const double *A, const double *B, double *C, int device);
int cugp_mfma_peak_tflops(int device, double *tflops);
/* stand-alone LA timings on a device-built SPD matrix (ms, best of reps): op 0 Cholesky (cuda_src/
 * cholesky_cu_solver.cpp), 1 triangular inverse of the factor (tmi_cu_solver.cpp), 2 K^-1 from it, 3 all three,
 * 4 plain C = K K^T with uniform tiles (cublas_matrix_multiply.cpp), 5 the sparse model's Gram product of one chunk:
 * P = W^T W over the lower tiles for W [16384][n] (k_sparse_gram's split-k partial tiles and their fixed-order sum) */
int cugp_bench_la(int op, int n, int device, int reps, double *ms);
/* the same, and for ops 0 and 3 log|K| taken from the factor the timed launches produced (NaN otherwise) */
int cugp_bench_la_check(int op, int n, int device, int reps, double *ms, double *logdet);
/* launch-shape thresholds (kernels.h TUNE_*), for A/B runs.  cugp_set_tuning changes the PROCESS DEFAULT of a key
 * (thread-safe: a lock); every handle carries its own copy and takes the defaults over when it next starts to enqueue,
 * so an evaluation in flight keeps the shapes it was enqueued with.  cugp_set_handle_tuning sets a key for ONE handle
 * (own != 0: later cugp_set_tuning calls no longer change it; own == 0: back to the default), called by the thread that
 * owns the handle like every other call on it; cugp_get_handle_tuning reads the value the handle's next enqueue uses.
 * (The reference has no counterpart: its launch shapes are compile-time constants, cuda_scalingdist/cuda_gp.cu:20-60.) */
int cugp_set_tuning(int key, int value);
int cugp_set_handle_tuning(cugp_gp *gp, int key, int value, int own);
int cugp_get_handle_tuning(cugp_gp *gp, int key, int *value);
/* 1 where the handle's factorisation stream runs at the device's highest priority (kernels.h TUNE_STREAM_PRIO: a handle
 * evaluated alone, with the inverse beside the factorisation, of at least TUNE_PRIO_MIN_NT tile rows -- or the key's
 * explicit bit 0), else 0.  Decided when the handle is created and again by cugp_set_data, cugp_set_handle_tuning,
 * cugp_set_overlap and on joining a group or a BCM; results never depend on it. */
int cugp_chain_first(const cugp_gp *gp, int *on);
/* tile rows handed to the inverse streams at a time for a matrix of nt tile rows evaluated alone (TUNE_PIPE_BLOCK < 0):
 * 1 ... 16, non-decreasing in nt (pure arithmetic, no device) */
int cugp_pipe_block_for(int nt);
/* the launches of step kb of the two-speed Cholesky with panels of P steps and a near window of about `near_tiles`
 * tiles (pure arithmetic, no device): out = {wide k0, wide k tiles, wide columns [a0,a1), step-launch width in tile
 * columns from kb+1}; tests/test_host_logic.py replays it: every tile sees every k exactly once, ascending */
int cugp_potrf_plan(int nt, int P, int near_tiles, int kb, int out[5]);
/* the same with the near window in sub-panels of S steps (tuning key 17); out[5] = first k tile of the step launch's
 * pass: it subtracts the k tiles [out[5], kb] from the columns [kb+1, kb+1+out[4]) */
int cugp_potrf_plan_sub(int nt, int P, int near_tiles, int S, int kb, int out[6]);

#ifdef __cplusplus
}
#endif
#endif /* CUGP_H */
