// comm.cpp -- the per-evaluation exchange of a BCM sharded one process per GPU, on the library's OWN stream.
//
// The reference moves 1 (log-likelihood) or 3 (gradient) doubles per worker over TCP for every objective evaluation
// (cuda_scalingdist/cg_solver.cpp:72-213: the master collects them worker by worker).  Here expert k lives on rank
// k mod W (cg_solver.cpp:93), every rank evaluates its experts as one group of shared launches, and the rows
// {LL_k, g_k} of ALL experts reach every rank by ONE ncclAllGather -- enqueued on the stream the evaluation runs on,
// directly behind its last kernel, followed by the copy into pinned host memory; the host waits ONCE, for the whole
// sequence.  (Rounds 1-5 went through torch.distributed from Python: a host wait for the evaluation, a staging copy,
// the collective, a blocking copy back -- 45-80 us per evaluation measured at one rank, profiles/r06_rehearse_*.json,
// beside 0.68 ms of device time for the two 1500-row experts a rank of the 8-GPU si24000 run owns.)
//
// RCCL is opened at run time (dlopen librccl.so.1): libcugp.so itself has no link-time dependency on it, and inside a
// process that has torch loaded the handle is torch's own copy of the library (same SONAME).
#include <dlfcn.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>          // types and enums only

#include "../../include/cugp.h"
#include "group.h"

namespace {

struct Rccl {
    void* so = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    bool ok = false;
};
Rccl g_rccl;
std::once_flag g_rccl_once;

const Rccl& rccl()
{
    std::call_once(g_rccl_once, [] {
        for (const char* name : {"librccl.so.1", "librccl.so"}) {
            g_rccl.so = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
            if (g_rccl.so) break;
        }
        if (!g_rccl.so) return;
        auto sym = [](const char* n) { return dlsym(g_rccl.so, n); };
        g_rccl.GetUniqueId = (decltype(g_rccl.GetUniqueId))sym("ncclGetUniqueId");
        g_rccl.CommInitRank = (decltype(g_rccl.CommInitRank))sym("ncclCommInitRank");
        g_rccl.CommDestroy = (decltype(g_rccl.CommDestroy))sym("ncclCommDestroy");
        g_rccl.AllGather = (decltype(g_rccl.AllGather))sym("ncclAllGather");
        g_rccl.AllReduce = (decltype(g_rccl.AllReduce))sym("ncclAllReduce");
        g_rccl.GetErrorString = (decltype(g_rccl.GetErrorString))sym("ncclGetErrorString");
        g_rccl.ok = g_rccl.GetUniqueId && g_rccl.CommInitRank && g_rccl.CommDestroy && g_rccl.AllGather && g_rccl.AllReduce;
    });
    return g_rccl;
}

int nccl_fail(const char* what, ncclResult_t r)
{
    char buf[256];
    snprintf(buf, sizeof buf, "%s: %s", what, g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "RCCL error");
    return cugp_internal_fail(CUGP_ERR_DEVICE, buf);
}

int hip_fail(const char* what, hipError_t e)
{
    char buf[256];
    snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
    return cugp_internal_fail(e == hipErrorOutOfMemory ? CUGP_ERR_NOMEM : CUGP_ERR_DEVICE, buf);
}

}  // namespace

struct cugp_comm {
    ncclComm_t comm = nullptr;   // null: a world of one without a communicator (nothing to exchange)
    int rank = 0, world = 1, device = 0;
    Scratch dsend, drecv;                        // [per][w] this rank's rows, [world * per][w] everybody's; w = 1 + nh (4, or an ARD BCM's d + 3)
    size_t send_rows = 0, send_w = 0;            // shape dsend was last zeroed for
    Scratch hrecv{nullptr, 0, true};             // pinned copy of drecv
    // product-of-experts prediction (cugp_bcm_predict_allgather): this rank's block, everybody's, the reduced
    // [mean | var | status words] on the device and pinned, the pinned header {status, local count}
    hipStream_t stream = nullptr;                // the exchange's own stream on `device`
    Scratch pdsend, pdrecv, pdout, phout{nullptr, 0, true};
    double* phdr = nullptr;
};

extern "C" {

int cugp_comm_unique_id(void* id, int bytes)
{
    if (!id || bytes != NCCL_UNIQUE_ID_BYTES) return CUGP_ERR_INVALID;
    const Rccl& R = rccl();
    if (!R.ok) return cugp_internal_fail(CUGP_ERR_NODEVICE, "librccl.so.1 could not be opened (dlopen)");
    ncclUniqueId u;
    const ncclResult_t r = R.GetUniqueId(&u);
    if (r != ncclSuccess) return nccl_fail("ncclGetUniqueId", r);
    memcpy(id, &u, sizeof u);
    return CUGP_OK;
}

int cugp_comm_create(const void* id, int bytes, int rank, int world, int device, cugp_comm** out)
{
    if (!out || world < 1 || rank < 0 || rank >= world) return CUGP_ERR_INVALID;
    if (world > 1 && !id) return CUGP_ERR_INVALID;
    if (id && bytes != NCCL_UNIQUE_ID_BYTES) return CUGP_ERR_INVALID;
    cugp_comm* c = new (std::nothrow) cugp_comm;
    if (!c) return CUGP_ERR_NOMEM;
    c->rank = rank; c->world = world; c->device = device;
    if (id) {                                         // (a world of one WITH an id: a one-rank communicator, to rehearse the path)
        const Rccl& R = rccl();
        if (!R.ok) { delete c; return cugp_internal_fail(CUGP_ERR_NODEVICE, "librccl.so.1 could not be opened (dlopen)"); }
        hipError_t e = hipSetDevice(device);
        if (e != hipSuccess) { delete c; return hip_fail("hipSetDevice", e); }
        ncclUniqueId u;
        memcpy(&u, id, sizeof u);
        const ncclResult_t r = R.CommInitRank(&c->comm, world, u, rank);
        if (r != ncclSuccess) { delete c; return nccl_fail("ncclCommInitRank", r); }
    }
    *out = c;
    return CUGP_OK;
}

int cugp_comm_destroy(cugp_comm* c)
{
    if (!c) return CUGP_OK;
    (void)hipSetDevice(c->device);
    if (c->comm) (void)rccl().CommDestroy(c->comm);
    for (Scratch* b : {&c->dsend, &c->drecv, &c->hrecv}) b->release();
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (Scratch* b : {&c->pdsend, &c->pdrecv, &c->pdout, &c->phout}) b->release();
    if (c->phdr) (void)hipHostFree(c->phdr);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return CUGP_OK;
}

// grow-only; nothing of the exchange is in flight between calls
static int comm_buffers(cugp_comm* c, int per, int w)
{
    const size_t nsend = (size_t)per * w;
    int rc;
    if (nsend > c->dsend.cap || (size_t)w != c->send_w || (size_t)per != c->send_rows) {
        if ((rc = c->dsend.grow(nsend, nullptr))) return rc;
        // unused slots: exact zeros -- for good while the rows keep their shape (an ARD BCM's are wider)
        const hipError_t e = hipMemset(c->dsend.p, 0, nsend * sizeof(double));
        if (e != hipSuccess) { c->dsend.release(); c->send_w = c->send_rows = 0; return hip_fail("exchange buffers", e); }
        c->send_w = (size_t)w;
        c->send_rows = (size_t)per;
    }
    if ((rc = c->drecv.grow(c->world * nsend, nullptr)) || (rc = c->hrecv.grow(c->world * nsend, nullptr))) return rc;
    return CUGP_OK;
}

// One objective evaluation of a sharded BCM on this rank: evaluate the local experts (b; may be null on a rank that owns
// none), all-gather everybody's rows, -> rows_out[world * per][4]: rank r's i-th expert (global expert r + i * world)
// in row r * per + i, {LL, g0, g1, g2}; slots beyond a rank's experts are zero.  Everything between the first kernel of
// the evaluation and the pinned copy of the gathered rows is ONE in-order sequence on the evaluation's stream.
// nh: the gradient's entries -- rows of 1 + nh doubles (3 from the isotropic call, d + 2 from the _ard call)
static int allgather_rows(cugp_bcm* b, cugp_comm* c, int per, int nh, double* rows_out)
{
    int nlocal = 0;
    if (b && cugp_bcm_num_experts(b, &nlocal)) return CUGP_ERR_INVALID;
    if (nlocal > per) return CUGP_ERR_INVALID;
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return hip_fail("hipSetDevice", e);
    int rc = comm_buffers(c, per, 1 + nh);
    if (rc) return rc;
    hipStream_t s = nullptr;
    if (nlocal > 0) {
        void* sv = nullptr;
        if ((rc = cugp_bcm_enqueue_rows_packed(b, c->dsend.p, &sv))) return rc;   // rows packed behind the evaluation, on its stream
        s = (hipStream_t)sv;
    }
    const size_t nsend = (size_t)per * (1 + nh), nall = nsend * c->world;
    const double* src = c->drecv.p;
    if (c->comm) {
        const ncclResult_t r = rccl().AllGather(c->dsend.p, c->drecv.p, nsend, ncclDouble, c->comm, s);
        if (r != ncclSuccess) { if (nlocal > 0) (void)cugp_bcm_finish_rows(b); return nccl_fail("ncclAllGather", r); }
    } else {
        src = c->dsend.p;                              // a world of one: this rank's rows are all the rows
    }
    e = hipMemcpyAsync(c->hrecv.p, src, nall * sizeof(double), hipMemcpyDeviceToHost, s);
    if (e != hipSuccess) { if (nlocal > 0) (void)cugp_bcm_finish_rows(b); return hip_fail("hipMemcpyAsync (gathered rows)", e); }
    if (nlocal > 0) rc = cugp_bcm_finish_rows(b);      // waits for the stream: evaluation, collective and copy
    else {
        e = hipStreamSynchronize(s);
        if (e != hipSuccess) return hip_fail("hipStreamSynchronize", e);
    }
    if (rc) return rc;
    memcpy(rows_out, c->hrecv.p, nall * sizeof(double));
    return CUGP_OK;
}

int cugp_bcm_loglik_grad_allgather(cugp_bcm* b, cugp_comm* c, int per, double* rows_out)
{
    if (!c || per <= 0 || !rows_out) return CUGP_ERR_INVALID;
    if (cugp_bcm_is_ard(b))
        return cugp_internal_fail(CUGP_ERR_INVALID, "cugp_bcm_loglik_grad_allgather: the BCM is ARD (d + 2 hyper-parameters); use cugp_bcm_loglik_grad_allgather_ard");
    return allgather_rows(b, c, per, 3, rows_out);
}

// the same for an ARD BCM: rows {LL, g[nh]}.  nh is explicit because a rank that owns no expert passes b == NULL.
int cugp_bcm_loglik_grad_allgather_ard(cugp_bcm* b, cugp_comm* c, int per, int nh, double* rows_out)
{
    if (!c || per <= 0 || !rows_out || nh < 3)
        return cugp_internal_fail(CUGP_ERR_INVALID, "cugp_bcm_loglik_grad_allgather_ard: null argument, per <= 0 or nh < 3");
    if (b && !cugp_bcm_is_ard(b))
        return cugp_internal_fail(CUGP_ERR_INVALID, "cugp_bcm_loglik_grad_allgather_ard: the BCM is isotropic (3 hyper-parameters); use cugp_bcm_loglik_grad_allgather");
    if (b && cugp_bcm_nh(b) != nh) {
        char buf[160];
        snprintf(buf, sizeof buf, "cugp_bcm_loglik_grad_allgather_ard: nh = %d, the BCM has d + 2 = %d hyper-parameters", nh, cugp_bcm_nh(b));
        return cugp_internal_fail(CUGP_ERR_INVALID, buf);
    }
    return allgather_rows(b, c, per, nh, rows_out);
}

static int pred_buffers(cugp_comm* c, size_t rstride, size_t nout)
{
    hipError_t e = hipSuccess;
    if (!c->stream) e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e == hipSuccess && !c->phdr) e = hipHostMalloc((void**)&c->phdr, 2 * sizeof(double), hipHostMallocDefault);
    if (e != hipSuccess) return hip_fail("prediction exchange buffers", e);
    int rc;
    if (rstride > c->pdsend.cap) {
        if ((rc = c->pdsend.grow(rstride, c->stream))) return rc;
        e = hipMemset(c->pdsend.p, 0, rstride * sizeof(double));
        if (e != hipSuccess) { c->pdsend.release(); return hip_fail("prediction exchange buffers", e); }
    }
    if ((c->comm && (rc = c->pdrecv.grow((size_t)c->world * rstride, c->stream))) || (rc = c->pdout.grow(nout, c->stream)) ||
        (rc = c->phout.grow(nout, c->stream)))
        return rc;
    return CUGP_OK;
}

static void fill_nan(double* mean, double* var, int nt)
{
    for (int i = 0; i < nt; i++) mean[i] = var[i] = NAN;
}

// Product-of-experts prediction of a BCM sharded one process per GPU (include/cugp.h).  Every rank sends
// {status, local expert count, [per][2][nt] rows (1/v, m/v of its i-th expert in slot i)} -- the same count on every
// rank -- by ONE ncclAllGather on the communicator's own stream, which the prediction kernels' streams are ordered in
// front of by events; k_poe_reduce sums every test point over the experts in global order, one copy brings mean,
// variance and the ranks' status words into pinned memory, and the host waits ONCE.  A local failure still joins the
// collective (nonzero status, NaN rows), so every rank reads every rank's status and all return the same code.
// The body of both public calls (`call`: the name in the error texts).  mode < 0: cugp_bcm_predict_allgather -- noisy rows,
// k_poe_reduce.  mode >= 0 (CUGP_COMBINE_*): cugp_bcm_predict_allgather_mode -- latent rows (the same launches, noise_var
// = 0 in the finish), k_poe_reduce_mode with sf2, sn2, with_noise; everything else is the same sequence.
static int predict_allgather(const char* call, cugp_bcm* b, cugp_comm* c, int per, int nexperts, const double* Xt, int nt,
                             int mode, int with_noise, double sf2, double sn2, double* mean, double* var)
{
    char buf[512];
    // what every rank detects identically from the shared arguments: no collective
    if (!c || per <= 0 || nexperts <= 0 || nt <= 0 || !Xt || !mean || !var || (long long)per * c->world < nexperts) {
        snprintf(buf, sizeof buf, "%s: bad argument", call);
        return cugp_internal_fail(CUGP_ERR_INVALID, buf);
    }
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return hip_fail("hipSetDevice", e);
    const size_t rstride = 2 + (size_t)per * 2 * nt, nout = 2 * (size_t)nt + 2 * (size_t)c->world;
    int rc = pred_buffers(c, rstride, nout);
    if (rc) return rc;                                 // (no send buffer: this rank cannot take part)
    // ---- this rank's block; from here on every failure becomes the status word
    const int expect = c->rank < nexperts ? (nexperts - c->rank + c->world - 1) / c->world : 0;
    int nlocal = 0, status = CUGP_OK;
    bool enqueued = false;
    if (b && cugp_bcm_num_experts(b, &nlocal)) status = CUGP_ERR_INVALID;
    if (status == CUGP_OK && nlocal != expect) {
        snprintf(buf, sizeof buf, "%s: rank %d holds %d experts, %d of %d expected", call, c->rank,
                 nlocal, expect, nexperts);
        status = cugp_internal_fail(CUGP_ERR_INVALID, buf);
    }
    if (status == CUGP_OK && nlocal > 0) {
        enqueued = true;
        status = cugp_bcm_predict_rows_enqueue_form(b, c->device, Xt, nt, c->pdsend.p + 2, 2 * (size_t)nt, c->stream,
                                                    mode >= 0 ? 1 : 0);
    }
    if (status != CUGP_OK) {
        if (enqueued) (void)cugp_bcm_predict_rows_finish(b);   // nothing enqueued still writes into the send buffer
        e = hipMemsetAsync(c->pdsend.p + 2, 0xff, (rstride - 2) * sizeof(double), c->stream);   // all-ones: NaN rows
        (void)e;
    }
    c->phdr[0] = (double)status;                       // (pinned, read by the copy below before the host waits)
    c->phdr[1] = (double)nlocal;
    e = hipMemcpyAsync(c->pdsend.p, c->phdr, 2 * sizeof(double), hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess && status == CUGP_OK) status = hip_fail("hipMemcpyAsync (status word)", e);
    // ---- the exchange
    const double* src = c->pdsend.p;                   // a world of one without an id: this rank's block is all of them
    if (c->comm) {
        const ncclResult_t r = rccl().AllGather(c->pdsend.p, c->pdrecv.p, rstride, ncclDouble, c->comm, c->stream);
        if (r != ncclSuccess) {
            if (enqueued) (void)cugp_bcm_predict_rows_finish(b);
            (void)hipStreamSynchronize(c->stream);
            fill_nan(mean, var, nt);
            return nccl_fail("ncclAllGather", r);
        }
        src = c->pdrecv.p;
    }
    rc = mode < 0 ? cugp_poe_reduce_enqueue(src, rstride, c->world, nexperts, nt, c->pdout.p, c->stream)
                  : cugp_poe_reduce_mode_enqueue(src, rstride, c->world, nexperts, nt, mode, sf2, sn2, with_noise ? 1 : 0,
                                                 c->pdout.p, c->stream);
    if (rc == CUGP_OK) {
        e = hipMemcpyAsync(c->phout.p, c->pdout.p, nout * sizeof(double), hipMemcpyDeviceToHost, c->stream);
        if (e != hipSuccess) rc = hip_fail("hipMemcpyAsync (prediction)", e);
    }
    e = hipStreamSynchronize(c->stream);               // the one host wait: prediction, collective, reduction, copy
    if (e != hipSuccess && rc == CUGP_OK) rc = hip_fail("hipStreamSynchronize", e);
    if (enqueued && status == CUGP_OK) status = cugp_bcm_predict_rows_finish(b);   // (streams already done: closes them)
    if (rc) { fill_nan(mean, var, nt); return rc; }
    // ---- every rank reads every rank's status word: the same verdict everywhere
    const double* h = c->phout.p;
    long long total = 0;
    for (int r = 0; r < c->world; r++) {
        const int st = (int)h[2 * (size_t)nt + 2 * r];
        if (st != CUGP_OK) {
            if (r == c->rank) {
                const std::string last = cugp_last_error();
                snprintf(buf, sizeof buf, "%s: rank %d failed (%d): %s", call, r, st, last.c_str());
            } else snprintf(buf, sizeof buf, "%s: rank %d failed (%d)", call, r, st);
            fill_nan(mean, var, nt);
            return cugp_internal_fail(st, buf);
        }
        total += (long long)h[2 * (size_t)nt + 2 * r + 1];
    }
    if (total != nexperts) {
        snprintf(buf, sizeof buf, "%s: the ranks hold %lld experts, %d expected", call, total, nexperts);
        fill_nan(mean, var, nt);
        return cugp_internal_fail(CUGP_ERR_INVALID, buf);
    }
    if (status != CUGP_OK) { fill_nan(mean, var, nt); return status; }   // (a failure while closing this rank's streams)
    memcpy(mean, h, (size_t)nt * sizeof(double));
    memcpy(var, h + nt, (size_t)nt * sizeof(double));
    return CUGP_OK;
}

int cugp_bcm_predict_allgather(cugp_bcm* b, cugp_comm* c, int per, int nexperts, const double* Xt, int nt, double* mean,
                               double* var)
{
    return predict_allgather("cugp_bcm_predict_allgather", b, c, per, nexperts, Xt, nt, -1, 0, 0.0, 0.0, mean, var);
}

// the same exchange with latent rows and k_poe_reduce_mode; sf2, sn2 are arguments: a rank without experts has no BCM
int cugp_bcm_predict_allgather_mode(cugp_bcm* b, cugp_comm* c, int per, int nexperts, const double* Xt, int nt, int mode,
                                    int with_noise, double sf2, double sn2, double* mean, double* var)
{
    if (mode < CUGP_COMBINE_POE || mode > CUGP_COMBINE_RBCM)
        return cugp_internal_fail(CUGP_ERR_INVALID, "cugp_bcm_predict_allgather_mode: unknown mode");
    return predict_allgather("cugp_bcm_predict_allgather_mode", b, c, per, nexperts, Xt, nt, mode, with_noise, sf2, sn2,
                             mean, var);
}

}  // extern "C"
