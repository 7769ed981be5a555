// group.cpp -- the BCM layer's groups of experts (group.h): create / destroy, the packing of result rows, the grouped
// prediction producers and the product-of-experts reductions.  The grouped EVALUATION is in cugp_capi.cpp.
#include <cstring>
#include <new>
#include <vector>

#include "handle.h"

using namespace cugp;

int cugp_group_create(cugp_gp* const* experts, int k, cugp_group** out)
{
    if (!experts || k <= 0 || !out) return CUGP_ERR_INVALID;
    for (int i = 0; i < k; i++)
        if (!experts[i] || experts[i]->npad != experts[0]->npad || experts[i]->d != experts[0]->d ||
            experts[i]->device != experts[0]->device)
            return CUGP_ERR_INVALID;
    for (int i = 0; i < k; i++)
        if (experts[i]->kernel != experts[0]->kernel)
            return fail(CUGP_ERR_INVALID, "cugp_group_create: the experts have different kernel kinds (one launch serves them all)");
    for (int i = 0; i < k; i++)
        if (experts[i]->ard != experts[0]->ard)
            return fail(CUGP_ERR_INVALID, "cugp_group_create: ARD and isotropic handles in one group (the experts of a group are all ARD or all isotropic)");
    for (int i = 0; i < k; i++)
        if (experts[i]->tied != experts[0]->tied)
            return fail(CUGP_ERR_INVALID, "cugp_group_create: rational quadratic handles with one length scale and with one per dimension in one group (their result rows differ in width)");
    cugp_group* gr = new (std::nothrow) cugp_group;
    if (!gr) return fail(CUGP_ERR_NOMEM, "host allocation");
    gr->experts.assign(experts, experts + k);
    for (cugp_gp* x : gr->experts) x->groups++;             // (cugp_append refuses them while the group lives: the table carries n)
    for (cugp_gp* x : gr->experts)                          // grouped experts run at default priorities (want_chain_first)
        if (hipSetDevice(x->device) != hipSuccess || fetch_eval(x) != CUGP_OK || apply_stream_prio(x) != CUGP_OK) {
            cugp_group_destroy(gr);
            return fail(CUGP_ERR_DEVICE, "cugp_group_create: the experts' streams");
        }
    const int nt = experts[0]->nt;
    const bool ard = experts[0]->ard;
    const size_t row = ard ? (size_t)ARD_ROW_GRAD + experts[0]->nh : 8;
    gr->ctx.row = (int)row;
    hipError_t e = hipSetDevice(experts[0]->device);
    if (e == hipSuccess) e = hipMalloc((void**)&gr->dtab, (size_t)k * sizeof(ExpertPtrs));
    if (e == hipSuccess) e = hipMalloc((void**)&gr->ctx.tickets, (size_t)k * ticket_count(nt) * sizeof(unsigned));
    if (e == hipSuccess) e = hipMalloc((void**)&gr->ctx.dout, (size_t)k * row * sizeof(double));
    if (e == hipSuccess) e = hipHostMalloc((void**)&gr->ctx.hout, (size_t)k * 8 * sizeof(double), hipHostMallocDefault);
    if (e == hipSuccess) memset(gr->ctx.hout, 0, (size_t)k * 8 * sizeof(double));   // (entry 6 of a row: status word)
    if (e == hipSuccess && ard) e = hipHostMalloc((void**)&gr->ctx.hrows, (size_t)k * row * sizeof(double), hipHostMallocDefault);
    if (e == hipSuccess && ard) memset(gr->ctx.hrows, 0, (size_t)k * row * sizeof(double));
    if (e != hipSuccess) {
        cugp_group_destroy(gr);
        return fail(e == hipErrorOutOfMemory ? CUGP_ERR_NOMEM : CUGP_ERR_DEVICE, "cugp_group_create", e);
    }
    gr->ctx.bt.tab = gr->dtab;
    gr->ctx.bt.count = k;
    *out = gr;
    return CUGP_OK;
}

void cugp_group_destroy(cugp_group* gr)
{
    if (!gr) return;
    if (!gr->experts.empty()) {
        (void)hipSetDevice(gr->experts[0]->device);
        (void)hipStreamSynchronize(gr->experts[0]->stream);
    }
    for (hipGraphExec_t x : gr->gexec)
        if (x) (void)hipGraphExecDestroy(x);
    if (gr->dtab) (void)hipFree(gr->dtab);
    if (gr->ctx.tickets) (void)hipFree(gr->ctx.tickets);
    if (gr->ctx.dout) (void)hipFree(gr->ctx.dout);
    if (gr->ctx.hout) (void)hipHostFree(gr->ctx.hout);
    if (gr->ctx.hrows) (void)hipHostFree(gr->ctx.hrows);
    gr->pred.release();
    for (cugp_gp* x : gr->experts) x->groups--;             // (the experts outlive their group; their streams stay as they are: apply_stream_prio)
    delete gr;
}

// rows [count][4] <- the first four of every 8-double result row of src, on `stream` (one 2D copy: a group's
// results packed for a collective)
int cugp_pack_result_rows(double* dst, const double* src, int count, void* stream)
{
    if (count <= 0) return CUGP_OK;
    HIPCHK(hipMemcpy2DAsync(dst, 4 * sizeof(double), src, 8 * sizeof(double), 4 * sizeof(double), (size_t)count,
                            hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return CUGP_OK;
}

// the nh-wide form: rows [count][1 + nh] <- {LL, g[nh]} of every result row of src.  nh = 3: the isotropic [8] rows (the
// call above); else ARD rows of ARD_ROW_GRAD + nh doubles -- LL from entry 0, the gradient from entry ARD_ROW_GRAD, two 2D
// copies on `stream`
int cugp_pack_result_rows_n(double* dst, const double* src, int count, int nh, int ard, void* stream)
{
    if (!ard) return nh == 3 ? cugp_pack_result_rows(dst, src, count, stream) : CUGP_ERR_INVALID;
    if (count <= 0) return CUGP_OK;
    const size_t dp = (size_t)(1 + nh) * sizeof(double), sp = (size_t)(ARD_ROW_GRAD + nh) * sizeof(double);
    HIPCHK(hipMemcpy2DAsync(dst, dp, src, sp, sizeof(double), (size_t)count, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    HIPCHK(hipMemcpy2DAsync(dst + 1, dp, src + ARD_ROW_GRAD, sp, (size_t)nh * sizeof(double), (size_t)count,
                            hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return CUGP_OK;
}

int cugp_copy_device_row(double* dst, const double* src, void* stream)
{
    HIPCHK(hipMemcpyAsync(dst, src, 4 * sizeof(double), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return CUGP_OK;
}

int cugp_copy_result_row(cugp_gp* g, double* dst)
{
    if (!g || !dst || !g->pending) return CUGP_ERR_INVALID;
    int rc;
    if ((rc = use_device(g))) return rc;
    if (g->ard) return cugp_pack_result_rows_n(dst, g->dout, 1, g->nh, 1, g->stream);
    return cugp_copy_device_row(dst, g->dout, g->stream);
}

// The prediction of every expert of the group by ONE sequence of launches on the lead expert's stream (returned in
// *stream): Xt copied to the device once, then per pass of pred_chunk_rows test points k_cross, k_predict_gemm and
// k_predict_finish, each one launch for all experts (blockIdx.y = expert).  Expert i's rows go to drows + i * row_stride:
// 1/v at [t], m/v at [nt + t].  Returns CUGP_ERR_INVALID without touching anything when the experts cannot predict as a
// group right now (an inverse missing or stale, different hyper-parameters, profiling level >= 3): the caller then
// enqueues them one by one (cugp_predict_rows_enqueue).
int cugp_group_predict_enqueue(cugp_group* gr, const double* Xt, int nt, double* drows, size_t row_stride, void** stream)
{
    return cugp_group_predict_enqueue_form(gr, Xt, nt, drows, row_stride, stream, 0);
}

int cugp_group_predict_enqueue_form(cugp_group* gr, const double* Xt, int nt, double* drows, size_t row_stride,
                                    void** stream, int latent)
{
    if (!gr || !Xt || nt <= 0 || !drows || !stream) return CUGP_ERR_INVALID;
    cugp_gp* lead = gr->experts[0];
    const int k = (int)gr->experts.size();
    int rc;
    if (gr->pending) return fail(CUGP_ERR_BUSY, "cugp_group_predict_enqueue: an evaluation is in flight");
    if (!same_loghyper(gr)) return CUGP_ERR_INVALID;
    for (cugp_gp* e : gr->experts)
        if (!cugp_has_inverse(e) || e->prof >= 3) return CUGP_ERR_INVALID;
    if ((rc = use_device(lead))) return rc;
    TuneScope ts(lead);                                       // the group runs on the lead expert's tuning
    if (!gr->tab_valid && (rc = write_group_table(gr))) return rc;
    if ((rc = predict_passes(lead, gr->ctx.bt, Xt, nt, pred_chunk_rows(lead, k, nt), gr->pred, drows, row_stride, nullptr,
                             latent != 0)))
        return rc;
    *stream = (void*)lead->stream;
    return CUGP_OK;
}

// The test-input gradients of every expert of the group by ONE sequence of batched launches on the lead expert's stream
// (returned in *stream): predict_grad_passes with the group's table.  Expert i's rows [m nt | v nt | dmean nt d | dvar nt d]
// go to drows + i * row_stride.  cugp_group_predict_enqueue_form's preconditions and contract: CUGP_ERR_INVALID without
// touching anything when the experts cannot run as a group right now -- the caller then goes expert by expert
// (cugp_predict_grad_rows_enqueue).
int cugp_group_predict_grad_enqueue(cugp_group* gr, const double* Xt, int nt, double* drows, size_t row_stride,
                                    void** stream, int latent, int want_dvar)
{
    if (!gr || !Xt || nt <= 0 || !drows || !stream) return CUGP_ERR_INVALID;
    cugp_gp* lead = gr->experts[0];
    int rc;
    if (gr->pending) return fail(CUGP_ERR_BUSY, "cugp_group_predict_grad_enqueue: an evaluation is in flight");
    if (!same_loghyper(gr)) return CUGP_ERR_INVALID;
    int tiles = 0;
    for (cugp_gp* e : gr->experts) {
        if (!cugp_has_inverse(e) || e->prof >= 3) return CUGP_ERR_INVALID;
        if (predict_grad_tiles(e->n) > tiles) tiles = predict_grad_tiles(e->n);
    }
    if ((rc = use_device(lead))) return rc;
    TuneScope ts(lead);                                       // the group runs on the lead expert's tuning
    if (!gr->tab_valid && (rc = write_group_table(gr))) return rc;
    if ((rc = predict_grad_passes(lead, gr->ctx.bt, tiles, Xt, nt, latent == 0, want_dvar != 0, gr->pred, drows, row_stride)))
        return rc;
    *stream = (void*)lead->stream;
    return CUGP_OK;
}

int cugp_poe_reduce_grad_enqueue(const double* gathered, size_t rstride, int world, int nexperts, int nt, int d, int mode,
                                 double sf2, double sn2, int with_noise, int want_dvar, double* dout, void* stream)
{
    launch_poe_reduce_grad(gathered, rstride, world, nexperts, nt, d, mode, sf2, sn2, with_noise, want_dvar, dout,
                           (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return CUGP_OK;
}

int cugp_poe_reduce_enqueue(const double* gathered, size_t rstride, int world, int nexperts, int nt, double* dout,
                            void* stream)
{
    launch_poe_reduce(gathered, rstride, world, nexperts, nt, dout, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return CUGP_OK;
}

int cugp_poe_reduce_mode_enqueue(const double* gathered, size_t rstride, int world, int nexperts, int nt, int mode,
                                 double sf2, double sn2, int with_noise, double* dout, void* stream)
{
    launch_poe_reduce_mode(gathered, rstride, world, nexperts, nt, mode, sf2, sn2, with_noise, dout, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return CUGP_OK;
}

// device side of the results of the evaluation in flight: [k][8] doubles, row i = {LL, g0, g1, g2, ...} of expert i (an
// ARD group: [k][8 + nh], LL at 0 and the gradient from entry 8), valid once everything enqueued on *stream so far has run
int cugp_group_device_results(cugp_group* gr, const double** dout, void** stream)
{
    if (!gr || !dout || !stream) return CUGP_ERR_INVALID;
    *dout = gr->ctx.dout;
    *stream = (void*)gr->experts[0]->stream;
    return CUGP_OK;
}
