// dense_features.cpp -- the optional features of a dense handle: appending observations, multi-target regression,
// leave-one-out cross-validation.  Their state: handle.h (Targets, Loo; append's stays flat in the handle).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>

#include "handle.h"

using namespace cugp;

// ---------------------------------------------------------------- appending observations
// The rows [n, n + k) in passes that never cross a multiple of 128 (include/cugp.h): pure arithmetic
int cugp_append_plan(int n, int k, int pass, int out[2])
{
    if (!out || n < 0 || k <= 0 || pass < 0 || (long long)n + k > 0x7fffffffLL)
        return fail(CUGP_ERR_INVALID, "cugp_append_plan: null out, n < 0, k <= 0, pass < 0 or n + k beyond int");
    const int end = n + k;
    int count = 0;
    bool found = false;
    for (int a = n; a < end; count++) {
        const int edge = (a / TILE + 1) * TILE, b = edge < end ? edge : end;
        if (count == pass) { out[0] = a; out[1] = b; found = true; }
        a = b;
    }
    if (!found) return fail(CUGP_ERR_INVALID, "cugp_append_plan: pass beyond the last one");
    return count;
}

int cugp_capacity(const cugp_gp* g, int* cap)
{
    if (!g || !cap) return fail(CUGP_ERR_INVALID, "cugp_capacity: null argument");
    *cap = g->npad;
    return CUGP_OK;
}

// One bordering step by the rows [r0, r1) (already in dX, dy) of a handle whose inverse quantities hold for its first r0
// rows -- DESIGN.md section 19.  Existing launches up to C and C^-1 in the factor handle, then the two append kernels.
static int append_pass(cugp_gp* g, cugp_gp* f, int r0, int r1)
{
    int rc;
    hipStream_t s = g->stream;
    const int kk = r1 - r0, npad = g->npad, d = g->d;
    const size_t strip = (size_t)TILE * npad;
    double *dKs = g->app.p, *dW = dKs + strip, *dV = dW + strip, *dQt = dV + strip;
    const double* Xb = g->dX + (size_t)r0 * d;
    CovFn cf;
    if ((rc = cov_fn(g, s, nullptr, &cf))) return rc;
    launch_kcross(g->dX, r0, d, npad, Xb, kk, TILE, cf, dKs, s);                    // B = k(Xb, X)
    launch_predict_gemm(dKs, g->dT, dW, npad, 1, g->nt, s);                         // P = B L^-T
    launch_targets_alpha(dW, g->dU, dV, npad, kk, s);                               // V = P L^-1 (whole 64-row tiles of the kk rows)
    const CovShape cs = predict_cov_shape(TILE, r0);
    if ((rc = g->cov.scr.grow((size_t)(cs.split - 1) * TILE * TILE, s))) return rc;
    launch_predict_cov(dW, npad, TILE, cs, f->dA, g->cov.scr.p, s);                 // P P^T
    launch_predict_cov_finish(Xb, kk, d, TILE, cf, true, 0.0, f->dA, g->cov.scr.p, cs.split - 1, nullptr, s);   // S
    launch_potf2(f->dA, TILE, 0, f->d16, f->d64, f->dlogdet, s);                    // C = chol(S)
    launch_trtri_diag(f->dA, TILE, 0, 1, f->d64, f->dT, f->dU, s);                  // C^-1
    launch_append_border(dW, dV, f->dA, f->dT, f->dlogdet, r0, kk, npad, g->dA, g->dT, g->dU, g->dKinv, g->dy, g->dz,
                         g->dalpha, g->dlogdet, dQt, s);
    launch_append_kinv(dQt, r0, kk, npad, g->dKinv, g->dz + r0, g->dalpha, s);
    HIPCHK(hipGetLastError());
    return CUGP_OK;
}

int cugp_append(cugp_gp* g, const double* Xnew, const double* ynew, int k)
{
    if (!g || !Xnew || !ynew) return fail(CUGP_ERR_INVALID, "cugp_append: null argument");
    if (k <= 0) return fail(CUGP_ERR_INVALID, "cugp_append: k must be positive");
    if (g->is_factor) return fail(CUGP_ERR_INVALID, "cugp_append: an internal factor handle takes no observations");
    if (g->bcm_expert)
        return fail(CUGP_ERR_INVALID, "cugp_append: the handle is an expert of a cugp_bcm (the experts' common padded size carries n)");
    if (g->groups > 0)
        return fail(CUGP_ERR_INVALID, "cugp_append: the handle is a member of a cugp_group (the group's device table carries n)");
    if (!g->have_data) return fail(CUGP_ERR_INVALID, "cugp_append: no training data set (cugp_set_data comes first)");
    if (g->tg.m > 0) return fail(CUGP_ERR_INVALID, "cugp_append: the handle has targets set (cugp_set_targets): targets have no new rows");
    if ((long long)g->n + k > g->npad) {
        char buf[256];
        snprintf(buf, sizeof buf, "cugp_append: %d + %d rows exceed the handle's capacity of %d; create it with a larger npad_min",
                 g->n, k, g->npad);
        return fail(CUGP_ERR_INVALID, buf);
    }
    int rc;
    if ((rc = use_device(g))) return rc;
    if ((rc = fetch_eval(g))) return rc;                             // an evaluation in flight is fetched first
    hipStream_t s = g->stream;
    const int n0 = g->n, d = g->d;
    if (!g->x_full) {                                                // dX: n rows until the first append, npad rows from then on
        double* nx = nullptr;
        HIPCHK(hipMalloc((void**)&nx, (size_t)g->npad * d * sizeof(double)));
        hipError_t e = hipMemcpyAsync(nx, g->dX, (size_t)n0 * d * sizeof(double), hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) { (void)hipFree(nx); return fail(CUGP_ERR_DEVICE, "cugp_append: growing X", e); }
        (void)hipFree(g->dX);
        g->dX = nx;
        g->x_full = true;
    }
    const bool update = g->inverse_valid;
    // from here on the handle holds n0 + k rows; it is stale until the passes and the trace have gone through
    g->cfg_epoch++;                                                  // captured graphs carry n (and X)
    g->factor_valid = g->inverse_valid = false;
    g->tg.valid = false;
    g->n = n0 + k;
    HIPCHK(hipMemcpyAsync(g->dX + (size_t)n0 * d, Xnew, (size_t)k * d * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(g->dy + n0, ynew, (size_t)k * sizeof(double), hipMemcpyHostToDevice, s));
    if (!update) {                                                   // no inverse to extend: the next evaluation factors n0 + k rows
        HIPCHK(hipStreamSynchronize(s));
        return CUGP_OK;
    }
    TuneScope ts(g);
    if (const int pe = prepare_kernels())
        return fail(CUGP_ERR_DEVICE, "hipFuncSetAttribute(MaxDynamicSharedMemorySize)", (hipError_t)pe);
    if ((rc = g->app.grow((size_t)4 * TILE * g->npad, s))) return rc;
    if ((rc = cov_factor_handle(g, 1))) return rc;
    cugp_gp* f = g->cov.f;
    f->nt = 1;                                                       // (one tile of the factor handle's buffers, ld = 128)
    f->npad = TILE;
    int rows[2];
    const int passes = cugp_append_plan(n0, k, 0, rows);
    for (int p = 0; p < passes; p++) {
        (void)cugp_append_plan(n0, k, p, rows);
        f->n = rows[1] - rows[0];
        if ((rc = append_pass(g, f, rows[0], rows[1]))) { (void)hipStreamSynchronize(s); return rc; }
    }
    // LL and the gradient at the new data: one k_trace launch, its last block finalises (enqueue_continue)
    HIPCHK(hipMemsetAsync(g->dtickets + 2 * g->nt, 0, sizeof(unsigned), s));
    CovFn cf;
    if ((rc = cov_fn(g, s, nullptr, &cf))) return rc;
    launch_trace(g->dX, g->n, d, g->npad, cf, g->dKinv, g->dalpha, g->dpart, s, {}, g->dz, g->dlogdet, g->dout, g->hout,
                 g->dtickets + 2 * g->nt);
    if ((rc = sync_or_fail(s, "cugp_append", hipGetLastError()))) return rc;
    g->pf.pev_valid = false;
    (void)read_result_row(g, g->hout, true);
    // a Schur complement that is not positive definite: NaN results, the data stays extended, and the next ordinary
    // evaluation factors all rows afresh
    if (!std::isfinite(g->last_ll)) discard_eval(g);
    return CUGP_OK;
}

// ---------------------------------------------------------------- multi-target regression
// m target vectors over the handle's inputs and hyper-parameters: everything that depends on the targets is N^2 work
// behind ONE factorisation and inverse (the handle's own evaluation, untouched).  Argument errors come first, then "no
// device" (a process without a GPU never looks into the handle), then what only the handle can tell.
namespace {
// the checks every evaluating call shares, behind its own argument checks
int tg_ready(const cugp_gp* g, const char* call)
{
    if (const int rc = need_device(call)) return rc;
    if (g->tg.m <= 0) return invalid_arg(call, "no targets set (cugp_set_targets)");
    return CUGP_OK;
}

// Z, A, the gradient of the summed objective and the final sums for the current (data, hp, targets): the handle's own
// evaluation first (whichever route cugp_loglik_grad takes; nothing of it is touched), then four launches on its stream
// and ONE host wait.
int eval_targets(cugp_gp* g)
{
    int rc;
    if ((rc = cugp_loglik_grad(g, nullptr, nullptr))) return rc;
    if (g->tg.valid && g->inverse_valid) return CUGP_OK;
    if ((rc = use_device(g))) return rc;
    TuneScope ts(g);
    hipStream_t s = g->stream;
    launch_predict_gemm(g->tg.y, g->dT, g->tg.z, g->npad, g->tg.mpad / TILE, g->nt, s);       // Z = Y L^-T
    launch_targets_alpha(g->tg.z, g->dU, g->tg.a, g->npad, g->tg.m, s);                        // A = Z L^-1
    CovFn cf;
    if ((rc = cov_fn(g, s, nullptr, &cf))) return rc;
    launch_trace_targets(g->dX, g->n, g->d, g->npad, cf, g->dKinv, g->tg.a, g->tg.m, g->tg.part, s);
    launch_finalize_targets(g->tg.z, g->npad, g->n, g->d, g->tg.m, g->last_logdet, g->tg.part, cf, g->tg.out, g->tg.hout, s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    g->tg.row.assign(g->tg.hout, g->tg.hout + 1 + g->nh + g->tg.m);
    g->tg.valid = true;
    return CUGP_OK;
}

// f = -sum_t LL_t and its gradient at th (NaN where the evaluation fails)
void targets_objective(void* ctx, const double* th, int nh, double* f, double* gr)
{
    cugp_gp* g = (cugp_gp*)ctx;
    const bool ok = set_theta(g, th) == CUGP_OK && eval_targets(g) == CUGP_OK;
    objective_result(ok, ok ? g->tg.row[0] : NAN, g->tg.row.data() + 1, nh, f, gr);
}
}  // namespace

int cugp_set_targets(cugp_gp* g, const double* Y, int m)
{
    const char* call = "cugp_set_targets";
    if (!g || !Y) return invalid_arg(call, "null argument");
    if (m <= 0) return invalid_arg(call, "m must be positive");
    int rc;
    if ((rc = need_device(call))) return rc;
    if (!g->have_data) return invalid_arg(call, "no training data set (cugp_set_data comes first: it supplies X)");
    if ((rc = use_device(g))) return rc;
    if ((rc = fetch_eval(g))) return rc;
    HIPCHK(hipStreamSynchronize(g->stream));
    g->tg.valid = false;
    const int mpad = (m + TILE - 1) / TILE * TILE;
    const size_t cnt = (size_t)mpad * g->npad, row = (size_t)1 + g->nh + mpad;
    if (mpad != g->tg.mpad) {
        g->tg.release();
        if ((rc = ensure(&g->tg.y, cnt)) || (rc = ensure(&g->tg.z, cnt)) || (rc = ensure(&g->tg.a, cnt)) ||
            (rc = ensure(&g->tg.out, row)))
            return rc;
        HIPCHK(hipHostMalloc((void**)&g->tg.hout, row * sizeof(double), hipHostMallocDefault));
        g->tg.mpad = mpad;
    }
    if ((rc = ensure(&g->tg.part, (size_t)g->nblocks_trace * g->ncol))) return rc;
    hipStream_t s = g->stream;
    HIPCHK(hipMemsetAsync(g->tg.y, 0, cnt * sizeof(double), s));
    HIPCHK(hipMemsetAsync(g->tg.z, 0, cnt * sizeof(double), s));
    HIPCHK(hipMemsetAsync(g->tg.a, 0, cnt * sizeof(double), s));
    HIPCHK(hipMemcpy2DAsync(g->tg.y, (size_t)g->npad * sizeof(double), Y, (size_t)g->n * sizeof(double),
                            (size_t)g->n * sizeof(double), m, hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    g->tg.m = m;
    return CUGP_OK;
}

int cugp_num_targets(const cugp_gp* g, int* m)
{
    if (!g || !m) return invalid_arg("cugp_num_targets", "null argument");
    *m = g->tg.m;
    return CUGP_OK;
}

int cugp_loglik_grad_targets(cugp_gp* g, double* ll, double* gr, int nh, double* ll_each)
{
    const char* call = "cugp_loglik_grad_targets";
    if (!g) return invalid_arg(call, "null handle");
    if (nh < 3) return invalid_arg(call, "nh is not the handle's (cugp_num_hyper)");
    int rc;
    if ((rc = tg_ready(g, call))) return rc;
    if (nh != g->nh) return invalid_arg(call, "nh is not the handle's (cugp_num_hyper)");
    if ((rc = eval_targets(g))) return rc;
    const double* r = g->tg.row.data();
    if (ll) *ll = r[0];
    if (gr) std::copy(r + 1, r + 1 + nh, gr);
    if (ll_each) std::copy(r + 1 + nh, r + 1 + nh + g->tg.m, ll_each);
    return CUGP_OK;
}

int cugp_get_alpha_targets(cugp_gp* g, double* alpha)
{
    const char* call = "cugp_get_alpha_targets";
    if (!g || !alpha) return invalid_arg(call, "null argument");
    int rc;
    if ((rc = tg_ready(g, call))) return rc;
    if ((rc = eval_targets(g))) return rc;
    HIPCHK(hipMemcpy2DAsync(alpha, (size_t)g->n * sizeof(double), g->tg.a, (size_t)g->npad * sizeof(double),
                            (size_t)g->n * sizeof(double), g->tg.m, hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));
    return CUGP_OK;
}

// Means of every target and (var given) the variance, which no target enters: cugp_predict's own k_cross, k_predict_gemm
// and k_predict_finish launches, unchanged, give it; the means are A Ks^T (launch_targets_mean).  One pass over the nt test
// points, as cugp_predict.
int cugp_predict_targets(cugp_gp* g, const double* Xt, int nt, double* mean, double* var)
{
    const char* call = "cugp_predict_targets";
    if (!g || !Xt || !mean) return invalid_arg(call, "null argument");
    if (nt <= 0) return invalid_arg(call, "nt must be positive");
    int rc;
    if ((rc = tg_ready(g, call))) return rc;
    if ((rc = eval_targets(g))) return rc;                          // (a stale handle is re-evaluated first)
    TuneScope ts(g);
    const int m = g->tg.m, ntpad = (nt + TILE - 1) / TILE * TILE, split = targets_mean_split(g->npad);
    const size_t nxt = (((size_t)nt * g->d + 15) / 16) * 16, nks = (size_t)ntpad * g->npad;
    const size_t np = (size_t)split * ((m + 63) / 64 * 64) * ntpad, nm = (size_t)m * nt;
    hipStream_t s = g->stream;
    if ((rc = g->tg.pred.grow(nxt + 2 * nks + 2 * (size_t)ntpad + np + nm, s))) return rc;
    double* dXt = g->tg.pred.p;
    double* dKs = dXt + nxt;
    double* dW = dKs + nks;
    double* dm1 = dW + nks;
    double* dv = dm1 + ntpad;
    double* dP = dv + ntpad;
    double* dM = dP + np;
    HIPCHK(hipMemcpyAsync(dXt, Xt, (size_t)nt * g->d * sizeof(double), hipMemcpyHostToDevice, s));
    CovFn cf;
    if ((rc = cov_fn(g, s, nullptr, &cf))) return rc;
    launch_kcross(g->dX, g->n, g->d, g->npad, dXt, nt, ntpad, cf, dKs, s);
    if (var) {
        launch_predict_gemm(dKs, g->dT, dW, g->npad, ntpad / TILE, g->nt, s);
        launch_predict_finish(dKs, dW, g->dalpha, g->n, g->npad, nt, cf.h, dm1, dv, s);
    }
    launch_targets_mean(g->tg.a, dKs, dP, g->npad, m, nt, ntpad, dM, s);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(mean, dM, nm * sizeof(double), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && var) e = hipMemcpyAsync(var, dv, (size_t)nt * sizeof(double), hipMemcpyDeviceToHost, s);
    return sync_or_fail(s, "cugp_predict_targets", e);
}

// conjugate gradients on the multi-target objective from the current hyper-parameters (cugp_cg_minimize_n over the handle's
// nh entries; trace rows of 1 + nh); the end point stays set, as cugp_cg_solve leaves it
int cugp_cg_solve_targets(cugp_gp* g, int budget, double* trace, int trace_cap, int* nevals)
{
    const char* call = "cugp_cg_solve_targets";
    if (!g) return invalid_arg(call, "null handle");
    int rc;
    if ((rc = tg_ready(g, call))) return rc;
    std::vector<double> th(g->theta);
    if ((rc = cugp_cg_minimize_n(targets_objective, g, th.data(), g->nh, budget, trace, trace_cap, nevals))) return rc;
    return set_theta(g, th.data());
}

// ---------------------------------------------------------------- leave-one-out cross-validation
// From K^-1 and alpha of the handle's own evaluation (untouched): the objective and the per-point predictions are two
// launches behind it, the gradient five more -- DESIGN.md section 24.  Argument errors come first, then "no device", then
// what only the handle can tell.  Nothing is kept between calls: every call launches, and equal inputs give equal bits.
namespace {
size_t loo_small_count(const cugp_gp* g)
{
    return (size_t)(LOO_PT_ROWS + 1 + g->npad / 64) * g->npad + (size_t)g->ncol * g->nblocks_trace;
}

// the evaluation that leaves K^-1 and alpha (a stale handle: re-evaluated, as predict_device does), then the LOO launches
// and ONE host wait.  The results row is in g->loo.hout ([0] L_LOO, [1 ..] the gradient when wanted); NaN where the
// covariance is not positive definite (the header's convention).
int loo_eval(cugp_gp* g, bool want_grad, const char* call)
{
    int rc;
    if (!g->have_data) return invalid_arg(call, "no training data set (cugp_set_data)");
    if ((rc = cugp_loglik_grad(g, nullptr, nullptr))) return rc;
    if ((rc = use_device(g))) return rc;
    const size_t nn = (size_t)g->npad * g->npad, row = (size_t)1 + g->nh;
    if ((rc = ensure(&g->loo.pt, loo_small_count(g))) || (rc = ensure(&g->loo.out, row))) return rc;
    if (!g->loo.hout) HIPCHK(hipHostMalloc((void**)&g->loo.hout, row * sizeof(double), hipHostMallocDefault));
    if (want_grad && !g->loo.P) {                                    // both or neither: a failure leaves the handle as it was
        if ((rc = ensure(&g->loo.B, nn))) return rc;
        if ((rc = ensure(&g->loo.P, nn))) { (void)hipFree(g->loo.B); g->loo.B = nullptr; return rc; }
    }
    for (size_t i = 0; i < row; i++) g->loo.hout[i] = NAN;
    if (!g->inverse_valid) return CUGP_OK;                           // (NaN evaluation: nothing to read K^-1 from)
    TuneScope ts(g);
    hipStream_t s = g->stream;
    double* pt = g->loo.pt;
    double* b = pt + (size_t)LOO_PT_ROWS * g->npad;
    double* bpart = b + g->npad;
    double* part = bpart + (size_t)(g->npad / 64) * g->npad;
    launch_loo_point(g->dKinv, g->dalpha, g->dy, g->n, g->npad, pt, g->loo.out, g->loo.hout, s);
    if (want_grad) {
        if (const int pe = prepare_kernels())
            return fail(CUGP_ERR_DEVICE, "hipFuncSetAttribute(MaxDynamicSharedMemorySize)", (hipError_t)pe);
        launch_loo_mirror_scale(g->dKinv, pt, g->n, g->npad, g->loo.B, bpart, b, s);
        {
            TimedLaunch tl(g, s, g->prof >= 2 && g->prof <= 4);      // (no stamp slot in k_loo_product: level 5 does not time it)
            launch_loo_product(g->loo.B, g->loo.P, g->npad, s);
            tl.done(KIND_LOO, (double)tri_tiles(g->nt) * 2.0 * TILE * TILE * g->npad);
        }
        CovFn cf;
        if ((rc = cov_fn(g, s, nullptr, &cf))) return rc;
        launch_trace_loo(g->dX, g->n, g->d, g->npad, cf, g->loo.P, g->dalpha, b, part, g->loo.out, g->loo.hout, s);
    }
    if ((rc = sync_or_fail(s, call, hipGetLastError()))) return rc;
    if (g->prof >= 2) drain_kernel_events(g);
    return CUGP_OK;
}

// f = -L_LOO and its gradient at th (NaN where the evaluation fails)
void loo_objective(void* ctx, const double* th, int nh, double* f, double* gr)
{
    cugp_gp* g = (cugp_gp*)ctx;
    const bool ok = set_theta(g, th) == CUGP_OK && loo_eval(g, true, "cugp_cg_solve_loo") == CUGP_OK;
    objective_result(ok, ok ? g->loo.hout[0] : NAN, g->loo.hout + 1, nh, f, gr);
}
}  // namespace

int cugp_loo(cugp_gp* g, double* lpl, double* gr, int nh)
{
    const char* call = "cugp_loo";
    if (!g) return invalid_arg(call, "null handle");
    if (!lpl) return invalid_arg(call, "lpl is NULL");
    if (nh < 3) return invalid_arg(call, "nh is not the handle's (cugp_num_hyper)");
    int rc;
    if ((rc = need_device(call))) return rc;
    if (nh != g->nh) return invalid_arg(call, "nh is not the handle's (cugp_num_hyper)");
    if ((rc = loo_eval(g, gr != nullptr, call))) return rc;
    *lpl = g->loo.hout[0];
    if (gr) std::copy(g->loo.hout + 1, g->loo.hout + 1 + nh, gr);
    return CUGP_OK;
}

int cugp_loo_predict(cugp_gp* g, double* mean, double* var, double* logp)
{
    const char* call = "cugp_loo_predict";
    if (!g) return invalid_arg(call, "null handle");
    if (!mean || !var) return invalid_arg(call, "mean or var is NULL");
    int rc;
    if ((rc = need_device(call))) return rc;
    if ((rc = loo_eval(g, false, call))) return rc;
    const size_t bytes = (size_t)g->n * sizeof(double);
    if (!g->inverse_valid) {
        std::fill(mean, mean + g->n, NAN);
        std::fill(var, var + g->n, NAN);
        if (logp) std::fill(logp, logp + g->n, NAN);
        return CUGP_OK;
    }
    hipStream_t s = g->stream;
    hipError_t e = hipMemcpyAsync(mean, g->loo.pt, bytes, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(var, g->loo.pt + g->npad, bytes, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && logp) e = hipMemcpyAsync(logp, g->loo.pt + 2 * (size_t)g->npad, bytes, hipMemcpyDeviceToHost, s);
    return sync_or_fail(s, call, e);
}

// conjugate gradients on -L_LOO from the current hyper-parameters: the loop of cugp_cg_minimize_n over the handle's nh
// entries; the end point stays set, as cugp_cg_solve leaves it.  The trace holds the ITERATES, rows of nh + 1: the start
// and the point each line search ended at -- the objective never rises along it; the row behind the last one written
// (when there is room) carries NaN in every entry, so a caller can count them.  *nevals: evaluations made.
int cugp_cg_solve_loo(cugp_gp* g, int budget, double* trace, int trace_cap, int* nevals)
{
    const char* call = "cugp_cg_solve_loo";
    if (!g) return invalid_arg(call, "null handle");
    if (budget <= 0) return invalid_arg(call, "budget must be positive");
    int rc;
    if ((rc = need_device(call))) return rc;
    if (!g->have_data) return invalid_arg(call, "no training data set (cugp_set_data)");
    std::vector<double> th(g->theta);
    if ((rc = cg_iterates(loo_objective, g, th.data(), g->nh, budget, trace, trace_cap, nevals))) return rc;
    return set_theta(g, th.data());
}
