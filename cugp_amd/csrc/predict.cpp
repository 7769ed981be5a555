// predict.cpp -- a dense handle's prediction, its gradients with respect to the test inputs, the joint predictive
// distribution, and the row producers the BCM layer enqueues (group.h).
#include <cmath>

#include "handle.h"

using namespace cugp;

// ---------------------------------------------------------------- prediction
int cugp_nlpp(const double* actual, const double* mean, const double* var, int nt, double* nlpp)
{
    if (!actual || !mean || !var || !nlpp || nt <= 0) return CUGP_ERR_INVALID;
    double acc = 0.0;   // covkernel.cpp:649-659, 2*pi truncated to 6.283185
    for (int i = 0; i < nt; i++)
        acc += 0.5 * std::log(6.283185 * var[i]) + std::pow((mean[i] - actual[i]), 2) / (2 * var[i]);
    *nlpp = acc / nt;
    return CUGP_OK;
}

// The prediction at nt test points on g's stream: of g alone (bt = {}), or of every expert of g's group by ONE sequence
// of batched launches (bt: the group's table; blockIdx.y = expert).  Xt goes into the scratch `scr` (test inputs, then
// Ks and W of one pass, [expert][cpad][npad] each), then per pass of `chunk` test points k_cross, k_predict_gemm and
// k_predict_finish.  rows null: means and variances into the scratch behind W (one pass, chunk >= nt; *pb).  Else
// product-of-experts rows: expert i's 1/v at rows[i * rstride + t], m/v at rows[i * rstride + nt + t].
// latent: the same launches with noise_var = 0 in the scalars k_predict_finish takes by value -- the variance of the
// latent function, sf2 - |W_t|^2, computed directly; nothing else reads them.
int cugp::predict_passes(cugp_gp* g, Batch bt, const double* Xt, int nt, int chunk, Scratch& scr, double* rows, size_t rstride,
                         PredBufs* pb, bool latent)
{
    int rc;
    const int cmax = chunk < nt ? chunk : nt, ntpad = ((cmax + TILE - 1) / TILE) * TILE;
    const size_t nxt = (((size_t)nt * g->d + 15) / 16) * 16, nks = (size_t)bt.count * ntpad * g->npad;
    if ((rc = scr.grow(nxt + 2 * nks + (rows ? 0 : 2 * (size_t)ntpad), g->stream))) return rc;
    double* dXt = scr.p;
    double* dKs = dXt + nxt;
    double* dW = dKs + nks;
    double* dm = rows ? nullptr : dW + nks;
    double* dv = rows ? nullptr : dm + ntpad;
    HIPCHK(hipMemcpyAsync(dXt, Xt, (size_t)nt * g->d * sizeof(double), hipMemcpyHostToDevice, g->stream));
    if (!bt.tab && (rc = reset_stamps(g))) return rc;
    for (int t0 = 0; t0 < nt; t0 += chunk) {
        const int c = nt - t0 < chunk ? nt - t0 : chunk;
        const int cpad = ((c + TILE - 1) / TILE) * TILE;
        // (batched: X, n, T, alpha come from the table; k_predict_finish reads rstride and its cpad only then)
        CovFn cf;
        if ((rc = cov_fn(g, g->stream, nullptr, &cf))) return rc;
        launch_kcross(g->dX, g->n, g->d, g->npad, dXt + (size_t)t0 * g->d, c, cpad, cf, dKs, g->stream, bt);
        {
            // W = Ks L^-T: test tile tt, row tile ti sums k <= ti (the diagonal k tile of T is triangular: counted half)
            TimedLaunch tl(g, g->stream, !bt.tab && g->prof >= 3);
            launch_predict_gemm(dKs, g->dT, dW, g->npad, cpad / TILE, g->nt, g->stream, bt);
            double kt = 0;
            for (int ti = 0; ti < g->nt; ti++) kt += ti + 0.5;
            tl.done(KIND_PREDICT, kt * (cpad / TILE) * 2.0 * TILE * TILE * TILE);
        }
        HyperScalars hf = cf.h;
        if (latent) hf.noise_var = 0.0;
        launch_predict_finish(dKs, dW, g->dalpha, g->n, g->npad, c, hf, dm, dv, g->stream, rows ? rows + t0 : nullptr,
                              rstride, nt, cpad, bt);
    }
    HIPCHK(hipGetLastError());
    if (pb) *pb = PredBufs{dXt, dW, dm, dv};
    return CUGP_OK;
}

// means and variances at the nt test points in one pass (*pb), a stale handle re-evaluated first
static int predict_device(cugp_gp* g, const double* Xt, int nt, PredBufs* pb, bool latent = false)
{
    int rc;
    if ((rc = cugp_loglik_grad(g, nullptr, nullptr))) return rc;     // factor, T, alpha for the current hp
    if ((rc = use_device(g))) return rc;                             // (a BCM over several devices predicts expert by expert)
    TuneScope ts(g);
    return predict_passes(g, {}, Xt, nt, ((nt + TILE - 1) / TILE) * TILE, g->pred, nullptr, 0, pb, latent);
}

static int predict_host(cugp_gp* g, const double* Xt, int nt, double* mean, double* var, bool latent)
{
    PredBufs pb;
    int rc = predict_device(g, Xt, nt, &pb, latent);
    if (rc == CUGP_OK) {
        hipError_t e = hipMemcpyAsync(mean, pb.mean, (size_t)nt * sizeof(double), hipMemcpyDeviceToHost, g->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(var, pb.var, (size_t)nt * sizeof(double), hipMemcpyDeviceToHost, g->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(g->stream);
        if (e != hipSuccess) rc = fail(CUGP_ERR_DEVICE, "cugp_predict copy", e);
        else if (g->prof >= 2) drain_kernel_events(g);
    }
    (void)hipStreamSynchronize(g->stream);
    return rc;
}

int cugp_predict(cugp_gp* g, const double* Xt, int nt, double* mean, double* var)
{
    if (!g || !Xt || !mean || !var || nt <= 0) return fail(CUGP_ERR_INVALID, "cugp_predict: bad argument");
    return predict_host(g, Xt, nt, mean, var, false);
}

// cugp_predict's launches with noise_var = 0 in the finish: the same mean bits, var = sf2 - |W_t|^2
int cugp_predict_latent(cugp_gp* g, const double* Xt, int nt, double* mean, double* var)
{
    if (!g || !Xt || !mean || !var || nt <= 0) return fail(CUGP_ERR_INVALID, "cugp_predict_latent: bad argument");
    return predict_host(g, Xt, nt, mean, var, true);
}

// ---------------------------------------------------------------- gradients with respect to the test inputs
// Test points per pass of cugp_predict_grad: tuning key TUNE_PRED_CHUNK in 64-row tiles, or (0) as many as keep Ks, W, V
// and the tiles' partial sums of one pass within 1 GiB, in whole 128-row tiles.  Every test row is computed on its own,
// so the bits do not depend on it.  count, tiles: the experts that share the pass (and the budget) and the most 64-row
// training tiles of any of them; one handle: 1 and its own.
static int grad_chunk_rows(const cugp_gp* g, int nt, int count, int tiles)
{
    long long rows = (long long)g->tune[TUNE_PRED_CHUNK] * 64;
    if (rows <= 0) {
        const size_t per_row = (size_t)count * ((size_t)3 * g->npad + (size_t)2 * tiles * g->d) * sizeof(double);
        rows = (long long)((((size_t)1 << 30) / per_row) / TILE) * TILE;
        if (rows < TILE) rows = TILE;
    }
    const long long ntr = ((long long)nt + 63) / 64 * 64;
    return (int)(rows < ntr ? rows : ntr);
}

// Mean, variance and their gradients with respect to the test inputs on g's stream, left on the device as ROWS
//   [m nt | v nt | dmean nt d | dvar nt d]      ((2 + 2 d) nt doubles; the dvar part untouched when !want_var)
// of g alone (bt = {}), or of every expert of g's group by ONE sequence of batched launches (bt: the group's table,
// blockIdx.y = expert; tiles: the most 64-row training tiles of any expert).  Per pass of test points: k_cross,
// k_predict_gemm and the finish exactly as predict_passes launches them (the mean's and the variance's bits are
// cugp_predict's / cugp_predict_latent's; batched: k_predict_finish_mv, the same sums), then -- want_var -- V = W L^-1
// (launch_targets_alpha), k_predict_grad (partial sums per training tile) and k_predict_grad_finish.  V is always W L^-1,
// never Ks K^-1.  rows null: one handle's rows in the scratch behind the partial sums (*rows_out); else expert i's at
// rows + i * row_stride.  No copy to the host and no host wait.
int cugp::predict_grad_passes(cugp_gp* g, Batch bt, int tiles, const double* Xt, int nt, bool with_noise, bool want_var,
                              Scratch& scr, double* rows, size_t row_stride, double** rows_out)
{
    int rc;
    hipStream_t s = g->stream;
    const int chunk = grad_chunk_rows(g, nt, bt.count, tiles), cmax = chunk < nt ? chunk : nt;
    const int ntpad = ((cmax + TILE - 1) / TILE) * TILE, d = g->d;
    const size_t nxt = (((size_t)nt * d + 15) / 16) * 16, nks = (size_t)bt.count * ntpad * g->npad, pstride = (size_t)cmax * d;
    const size_t npart = (size_t)bt.count * tiles * 2 * pstride, nout = (size_t)nt * d;
    if ((rc = scr.grow(nxt + 3 * nks + npart + (rows ? 0 : 2 * (size_t)nt + 2 * nout), s))) return rc;
    double* dXt = scr.p;
    double* dKs = dXt + nxt;
    double* dW = dKs + nks;
    double* dV = dW + nks;
    double* dP = dV + nks;
    if (!rows) rows = dP + npart;
    double* dm = rows;
    double* dv = dm + nt;
    double* dgm = dv + nt;
    double* dgv = dgm + nout;
    HIPCHK(hipMemcpyAsync(dXt, Xt, (size_t)nt * d * sizeof(double), hipMemcpyHostToDevice, s));
    if (!bt.tab && (rc = reset_stamps(g))) return rc;
    for (int t0 = 0; t0 < nt; t0 += chunk) {
        const int c = nt - t0 < chunk ? nt - t0 : chunk;
        const int cpad = ((c + TILE - 1) / TILE) * TILE;
        const double gemm_flop = (double)cpad * g->npad * g->npad;   // a triangular product: the diagonal k tile counted half
        CovFn cf;
        if ((rc = cov_fn(g, s, nullptr, &cf))) return rc;
        launch_kcross(g->dX, g->n, d, g->npad, dXt + (size_t)t0 * d, c, cpad, cf, dKs, s, bt);
        {
            TimedLaunch tl(g, s, !bt.tab && g->prof >= 3);
            launch_predict_gemm(dKs, g->dT, dW, g->npad, cpad / TILE, g->nt, s, bt);
            tl.done(KIND_PREDICT, gemm_flop);
        }
        HyperScalars hf = cf.h;
        if (!with_noise) hf.noise_var = 0.0;
        double* pgm = dgm + (size_t)t0 * d;
        double* pgv = want_var ? dgv + (size_t)t0 * d : nullptr;
        if (bt.tab) {                                     // the group: Ks, W, V [expert][cpad][npad], one launch each
            launch_predict_finish_mv(dKs, dW, g->npad, c, hf, dm + t0, dv + t0, row_stride, cpad, s, bt);
            if (want_var) launch_targets_alpha_batched(dW, dV, g->npad, cpad, s, bt);
            launch_predict_grad_batched(d, g->npad, dXt + (size_t)t0 * d, c, cf, dKs, want_var ? dV : nullptr,
                                        (size_t)cpad * g->npad, dP, pstride, tiles, s, bt);
            launch_predict_grad_finish_batched(dP, pstride, tiles, c, d, cf, pgm, pgv, row_stride, s, bt);
            continue;
        }
        launch_predict_finish(dKs, dW, g->dalpha, g->n, g->npad, c, hf, dm + t0, dv + t0, s);
        if (want_var) {
            // V = W L^-1 (row t = K^-1 k*_t): W is zero in its columns >= n and its rows >= c, U's padding is identity.
            // launch_targets_alpha takes no launch-own events: timed by an event pair around it (levels 3 and 4).
            const bool timed = (g->prof == 3 || g->prof == 4) && g->pf.kev_used + 2 <= (int)g->pf.kev.size() &&
                               hipEventRecord(g->pf.kev[g->pf.kev_used], s) == hipSuccess;
            launch_targets_alpha(dW, g->dU, dV, g->npad, cpad, s);
            if (timed && hipEventRecord(g->pf.kev[g->pf.kev_used + 1], s) == hipSuccess) {
                g->pf.kev_prev[g->pf.kev_used / 2] = -1;
                g->pf.kev_kind[g->pf.kev_used / 2] = KIND_PREDICT;
                g->pf.kev_flopv[g->pf.kev_used / 2] = gemm_flop;
                g->pf.kev_used += 2;
            }
        }
        {
            TimedLaunch tl(g, s, g->prof >= 3);
            launch_predict_grad(g->dX, g->n, d, g->npad, dXt + (size_t)t0 * d, c, cf, dKs, want_var ? dV : nullptr, g->dalpha,
                                dP, pstride, s);
            tl.done(KIND_PGRAD, (want_var ? 2.0 : 1.0) * ((c + 63) / 64 * 64) * (double)tiles * 64 * sizeof(double));
        }
        launch_predict_grad_finish(dP, pstride, g->n, c, d, cf, pgm, pgv, s);
    }
    HIPCHK(hipGetLastError());
    if (rows_out) *rows_out = rows;
    return CUGP_OK;
}

// mean, variance and their gradients with respect to the test inputs (include/cugp.h): predict_grad_passes on the
// handle's stream.  All results stay in the scratch until the copies and the one host wait at the end.
int cugp_predict_grad(cugp_gp* g, const double* Xt, int nt, int with_noise, double* mean, double* var, double* dmean,
                      double* dvar)
{
    if (!g || !Xt || nt <= 0 || (!dmean && !dvar))
        return fail(CUGP_ERR_INVALID, "cugp_predict_grad: null handle or Xt, nt <= 0, or neither dmean nor dvar given");
    int rc;
    if ((rc = cugp_loglik_grad(g, nullptr, nullptr))) return rc;     // (fetches an evaluation in flight; factor, T, U, alpha for the current hp)
    if ((rc = use_device(g))) return rc;
    TuneScope ts(g);
    hipStream_t s = g->stream;
    const size_t nout = (size_t)nt * g->d;
    double* dm = nullptr;
    if ((rc = predict_grad_passes(g, {}, predict_grad_tiles(g->n), Xt, nt, with_noise != 0, dvar != nullptr, g->pred, nullptr,
                                  0, &dm)))
        return rc;
    const double *dv = dm + nt, *dgm = dv + nt, *dgv = dgm + nout;
    hipError_t e = hipSuccess;
    if (mean) e = hipMemcpyAsync(mean, dm, (size_t)nt * sizeof(double), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && var) e = hipMemcpyAsync(var, dv, (size_t)nt * sizeof(double), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && dmean) e = hipMemcpyAsync(dmean, dgm, nout * sizeof(double), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && dvar) e = hipMemcpyAsync(dvar, dgv, nout * sizeof(double), hipMemcpyDeviceToHost, s);
    if ((rc = sync_or_fail(s, "cugp_predict_grad", e))) return rc;   // the one host wait
    if (g->prof >= 2) drain_kernel_events(g);
    return CUGP_OK;
}

// cugp_predict_grad's launches with the rows left on the device (drows: (2 + 2 d) nt doubles on the handle's device) and
// no host wait: the per-expert half of cugp_bcm_predict_grad and of the form across ranks.  latent != 0: noise_var = 0
// in the finish (cugp_predict_latent's variance).  *stream: the handle's; cugp_predict_fetch waits for it.
int cugp_predict_grad_rows_enqueue(cugp_gp* g, const double* Xt, int nt, double* drows, void** stream, int latent,
                                   int want_dvar)
{
    if (!g || !Xt || nt <= 0 || !drows || !stream)
        return fail(CUGP_ERR_INVALID, "cugp_predict_grad_rows_enqueue: bad argument");
    int rc;
    if ((rc = cugp_loglik_grad(g, nullptr, nullptr))) return rc;
    if ((rc = use_device(g))) return rc;
    TuneScope ts(g);
    if ((rc = predict_grad_passes(g, {}, predict_grad_tiles(g->n), Xt, nt, latent == 0, want_dvar != 0, g->pred, drows, 0)))
        return rc;
    *stream = (void*)g->stream;
    return CUGP_OK;
}

int cugp_has_inverse(const cugp_gp* g) { return g && !g->pending && g->inverse_valid ? 1 : 0; }

int cugp_predict_enqueue(cugp_gp* g, const double* Xt, int nt, double* host_mv)
{
    return cugp_predict_enqueue_form(g, Xt, nt, host_mv, 0);
}

int cugp_predict_enqueue_form(cugp_gp* g, const double* Xt, int nt, double* host_mv, int latent)
{
    if (!g || !Xt || !host_mv || nt <= 0) return fail(CUGP_ERR_INVALID, "cugp_predict_enqueue: bad argument");
    PredBufs pb;
    int rc = predict_device(g, Xt, nt, &pb, latent != 0);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(host_mv, pb.mean, (size_t)nt * sizeof(double), hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipMemcpyAsync(host_mv + nt, pb.var, (size_t)nt * sizeof(double), hipMemcpyDeviceToHost, g->stream));
    return CUGP_OK;
}

int cugp_predict_fetch(cugp_gp* g)
{
    if (!g) return CUGP_ERR_INVALID;
    int rc;
    if ((rc = use_device(g))) return rc;
    HIPCHK(hipStreamSynchronize(g->stream));
    if (g->prof >= 2) drain_kernel_events(g);
    return CUGP_OK;
}

// Test points per pass of a prediction that writes product-of-experts rows (cugp_predict_rows_enqueue,
// cugp_group_predict_enqueue): tuning key TUNE_PRED_CHUNK in 64-row tiles, or (0) as many as keep the Ks and W scratch
// of `count` experts within 1 GiB, in whole 128-row tiles.  Every test row is computed on its own, so the bits do not
// depend on the chunk.
int cugp::pred_chunk_rows(const cugp_gp* g, int count, int nt)
{
    long long rows = (long long)g->tune[TUNE_PRED_CHUNK] * 64;
    if (rows <= 0) {
        rows = (long long)((((size_t)1 << 30) / ((size_t)count * 2 * g->npad * sizeof(double))) / TILE) * TILE;
        if (rows < TILE) rows = TILE;
    }
    const long long ntr = ((long long)nt + 63) / 64 * 64;
    return (int)(rows < ntr ? rows : ntr);
}

// Fallback half of cugp_bcm_predict_allgather for an expert that cannot share launches: the expert's prediction on its
// own stream (returned in *stream), in passes of pred_chunk_rows test points, writing 1/v to drows[0, nt) and m/v to
// drows[nt, 2 nt) (device memory of the expert's device) instead of mean / variance.  The same kernels and arithmetic as
// cugp_predict.  cugp_predict_fetch waits for it.
int cugp_predict_rows_enqueue(cugp_gp* g, const double* Xt, int nt, double* drows, void** stream)
{
    return cugp_predict_rows_enqueue_form(g, Xt, nt, drows, stream, 0);
}

// latent != 0: the rows of the latent function, 1/var_f and m/var_f (the same launches, noise_var = 0 in the finish)
int cugp_predict_rows_enqueue_form(cugp_gp* g, const double* Xt, int nt, double* drows, void** stream, int latent)
{
    if (!g || !Xt || nt <= 0 || !drows || !stream) return fail(CUGP_ERR_INVALID, "cugp_predict_rows_enqueue: bad argument");
    int rc;
    if ((rc = cugp_loglik_grad(g, nullptr, nullptr))) return rc;     // factor, T, alpha for the current hp
    if ((rc = use_device(g))) return rc;
    TuneScope ts(g);
    if ((rc = predict_passes(g, {}, Xt, nt, pred_chunk_rows(g, 1, nt), g->pred, drows, 0, nullptr, latent != 0))) return rc;
    *stream = (void*)g->stream;
    return CUGP_OK;
}

// ---------------------------------------------------------------- joint predictive distribution
// The shared half of cugp_predict_cov and cugp_predict_sample: the marginal prediction (predict_device: the same launches
// as cugp_predict, a stale handle re-evaluated first), then on the handle's stream
//   Sigma = k(Xt,Xt) (+ sn2 I) + jitter I - W W^T,   W = Ks L^-T
// into the lower tiles of the factor handle's A (k_predict_cov: the product, split over k when the tiles are few;
// k_predict_cov_finish: the kernel function and the fixed-order sum of the chunks; it also zeroes the factor handle's
// arrival tickets).  *fout: the factor handle (nt test points as its rows), *dmean: the device mean.
static int predict_cov_device(cugp_gp* g, const double* Xt, int nt, bool with_noise, double jitter, double** dmean,
                              cugp_gp** fout)
{
    PredBufs pb;
    int rc;
    if ((rc = predict_device(g, Xt, nt, &pb))) return rc;
    TuneScope ts(g);
    const int tiles = (nt + TILE - 1) / TILE, ntpad = tiles * TILE;
    if ((rc = cov_factor_handle(g, tiles))) return rc;
    if (!g->cov.ev) HIPCHK(hipEventCreateWithFlags(&g->cov.ev, hipEventDisableTiming));
    cugp_gp* f = g->cov.f;
    f->n = nt;                                                       // (a smaller problem in the handle's buffers)
    f->nt = tiles;
    f->npad = ntpad;
    const CovShape cs = predict_cov_shape(ntpad, g->n);
    if ((rc = g->cov.scr.grow((size_t)(cs.split - 1) * ntpad * ntpad, g->stream))) return rc;
    {
        TimedLaunch tl(g, g->stream, g->prof >= 3);
        launch_predict_cov(pb.w, g->npad, ntpad, cs, f->dA, g->cov.scr.p, g->stream);
        tl.done(KIND_COV, 2.0 * cs.tiles * (32.0 * cs.wm) * (32.0 * cs.wm) * cs.kend);
    }
    CovFn cf;
    if ((rc = cov_fn(g, g->stream, nullptr, &cf))) return rc;
    launch_predict_cov_finish(pb.xt, nt, g->d, ntpad, cf, with_noise, jitter, f->dA, g->cov.scr.p, cs.split - 1,
                              f->dtickets, g->stream);
    HIPCHK(hipGetLastError());
    *dmean = pb.mean;
    *fout = f;
    return CUGP_OK;
}

int cugp_predict_cov(cugp_gp* g, const double* Xt, int nt, int with_noise, double* mean, double* cov)
{
    if (!g || !Xt || !cov || nt <= 0) return fail(CUGP_ERR_INVALID, "cugp_predict_cov: bad argument");
    double* dm = nullptr;
    cugp_gp* f = nullptr;
    int rc = predict_cov_device(g, Xt, nt, with_noise != 0, 0.0, &dm, &f);
    if (rc) { (void)hipStreamSynchronize(g->stream); return rc; }
    hipError_t e = hipSuccess;
    if (mean) e = hipMemcpyAsync(mean, dm, (size_t)nt * sizeof(double), hipMemcpyDeviceToHost, g->stream);
    if (e == hipSuccess)
        e = hipMemcpy2DAsync(cov, (size_t)nt * sizeof(double), f->dA, (size_t)f->npad * sizeof(double),
                             (size_t)nt * sizeof(double), nt, hipMemcpyDeviceToHost, g->stream);
    if ((rc = sync_or_fail(g->stream, "cugp_predict_cov copy", e))) return rc;
    if (g->prof >= 2) drain_kernel_events(g);
    for (int i = 0; i < nt; i++)                                     // lower triangle, mirrored (cugp_get_K_inverse)
        for (int j = i + 1; j < nt; j++) cov[(size_t)i * nt + j] = cov[(size_t)j * nt + i];
    return CUGP_OK;
}

int cugp_predict_cov_device(cugp_gp* g, const double* Xt, int nt, int with_noise, const double** dcov, int* ld)
{
    if (!g || !Xt || !dcov || !ld || nt <= 0) return fail(CUGP_ERR_INVALID, "cugp_predict_cov_device: bad argument");
    double* dm = nullptr;
    cugp_gp* f = nullptr;
    int rc = predict_cov_device(g, Xt, nt, with_noise != 0, 0.0, &dm, &f);
    const hipError_t e = hipStreamSynchronize(g->stream);
    if (rc) return rc;
    if (e != hipSuccess) return fail(CUGP_ERR_DEVICE, "cugp_predict_cov_device", e);
    if (g->prof >= 2) drain_kernel_events(g);
    *dcov = f->dA;
    *ld = f->npad;
    return CUGP_OK;
}

// The draws behind a joint covariance, shared by cugp_predict_sample and cugp_sparse_predict_sample: Sigma (+ jitter I) of
// nt test points lies in the lower tiles of f, g's factor handle, enqueued on g's stream with the tickets zeroed; dm: the
// device mean.  C = chol(Sigma) by the library's blocked Cholesky on f's stream, F = normals C^T, samples = mean + F.
int cugp::sample_tail(cugp_gp* g, cugp_gp* f, const double* dm, int nt, int nsamples, const double* normals, double* samples,
                      const char* call)
{
    int rc;
    const int ntpad = f->npad, nspad = (nsamples + TILE - 1) / TILE * TILE;
    const size_t nz = (size_t)nspad * ntpad;
    if ((rc = g->cov.samp.grow(2 * nz + (size_t)nsamples * nt, g->stream))) return rc;
    double* dZ = g->cov.samp.p;
    double* dF = dZ + nz;
    double* dS = dF + nz;
    // the factor handle's stream goes on behind Sigma (an event, no host wait): C = chol(Sigma), F = Z C^T, + mean
    HIPCHK(hipEventRecord(g->cov.ev, g->stream));
    hipStream_t fs = f->stream;
    HIPCHK(hipStreamWaitEvent(fs, g->cov.ev, 0));
    {
        TuneScope tf(f);
        if ((rc = enqueue_potrf(f, false, false, f->dtickets))) { (void)hipStreamSynchronize(fs); return rc; }
    }
    launch_zero_upper_diag(f->dA, ntpad, f->nt, fs);
    HIPCHK(hipMemsetAsync(dZ, 0, nz * sizeof(double), fs));
    HIPCHK(hipMemcpy2DAsync(dZ, (size_t)ntpad * sizeof(double), normals, (size_t)nt * sizeof(double),
                            (size_t)nt * sizeof(double), nsamples, hipMemcpyHostToDevice, fs));
    launch_predict_gemm(dZ, f->dA, dF, ntpad, nspad / TILE, f->nt, fs);     // F[s][t] = sum_{k <= t} Z[s][k] C[t][k]
    launch_sample_finish(dF, ntpad, dm, nt, nsamples, dS, fs);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess)
        e = hipMemcpyAsync(samples, dS, (size_t)nsamples * nt * sizeof(double), hipMemcpyDeviceToHost, fs);
    if (e == hipSuccess) e = hipStreamSynchronize(fs);                     // (behind everything of g->stream too)
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(fs);
        (void)hipStreamSynchronize(g->stream);
        return fail(CUGP_ERR_DEVICE, call, e);
    }
    if (g->prof >= 2) drain_kernel_events(g);
    return CUGP_OK;
}

int cugp_predict_sample(cugp_gp* g, const double* Xt, int nt, int with_noise, double jitter, int nsamples,
                        const double* normals, double* samples)
{
    if (!g || !Xt || !normals || !samples || nt <= 0 || nsamples <= 0 || !std::isfinite(jitter) || !(jitter >= 0.0))
        return fail(CUGP_ERR_INVALID, "cugp_predict_sample: bad argument");
    double* dm = nullptr;
    cugp_gp* f = nullptr;
    int rc = predict_cov_device(g, Xt, nt, with_noise != 0, jitter, &dm, &f);
    if (rc) { (void)hipStreamSynchronize(g->stream); return rc; }
    return sample_tail(g, f, dm, nt, nsamples, normals, samples, "cugp_predict_sample");
}
