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

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>          // types and enums only

#include "../../include/cugp.h"
#include "group.h"
#include "handle.h"

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
    Scratch pdsend, pdrecv, pdout, phout{nullptr, 0, true};   // (the gradient form's are the same buffers, wider)
    double* phdr = nullptr;
    // the sparse model with its rows sharded over ranks (cugp_sparse_sharded_bound_grad): this rank's block and everybody's
    // -- both exchanges use them in turn -- and the pinned headers [SHARD_HDR + per | world * SHARD_HDR]
    Scratch sdsend, sdrecv, shh{nullptr, 0, true};
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
    for (Scratch* b : {&c->pdsend, &c->pdrecv, &c->pdout, &c->phout, &c->sdsend, &c->sdrecv, &c->shh}) b->release();
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
// nh: the gradient's entries -- rows of 1 + nh doubles (3 from the isotropic call, the BCM's nh from the _ard call)
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

// the outputs of a failed call: NaN, every one that was asked for (grad: dmean / dvar of nd entries each)
struct PredOut {
    double *mean, *var, *dmean, *dvar;
    size_t nt, nd;
    void fill_nan() const
    {
        for (size_t i = 0; i < nt; i++) { if (mean) mean[i] = NAN; if (var) var[i] = NAN; }
        for (size_t i = 0; i < nd; i++) { if (dmean) dmean[i] = NAN; if (dvar) dvar[i] = NAN; }
    }
};

// Product-of-experts prediction of a BCM sharded one process per GPU (include/cugp.h).  Every rank sends
// {status, local expert count, [per] slots (its i-th expert's rows in slot i)} -- the same count on every
// rank -- by ONE ncclAllGather on the communicator's own stream, which the prediction kernels' streams are ordered in
// front of by events; the reduce kernel combines every test point over the experts in global order, one copy brings the
// results and the ranks' status words into pinned memory, and the host waits ONCE.  A local failure still joins the
// collective (nonzero status, NaN rows), so every rank reads every rank's status and all return the same code.
// The ONE body of the three public calls (`call`: the name in the error texts), parameterised by a PredForm: the slot
// width, how this rank's experts fill their slots, and the reduce launch.
//   cugp_bcm_predict_allgather        slots [2][nt] (1/v, m/v of the noisy prediction), k_poe_reduce
//   cugp_bcm_predict_allgather_mode   the same slots of the latent rows (the same launches, noise_var = 0 in the
//                                     finish), k_poe_reduce_mode with sf2, sn2, with_noise
//   cugp_bcm_predict_grad_allgather   slots [m nt | v nt | dmean nt d | dvar nt d] (latent for mode >= 0, noisy for
//                                     CUGP_COMBINE_REFERENCE), k_poe_reduce_grad; o.mean / o.var may be null
// The reduce kernel's output is [slot-independent results, `words` doubles | world x {status, count}].
// The caller has checked the arguments every rank checks alike.
struct PredForm {
    size_t slot;                                       // doubles per expert in a rank's block
    size_t words;                                      // doubles of results in front of the status words
    // this rank's experts' rows into dsend (slot i at dsend + i * slot), *stream (the communicator's own) ordered behind them
    std::function<int(cugp_bcm* b, int device, double* dsend, void** stream)> enqueue;
    // gathered [world][rstride] -> dout on stream
    std::function<int(const double* src, size_t rstride, int world, double* dout, void* stream)> reduce;
};

static int predict_allgather(const char* call, cugp_bcm* b, cugp_comm* c, int per, int nexperts, int nt,
                             const PredForm& f, const PredOut& o)
{
    char buf[512];
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return hip_fail("hipSetDevice", e);
    const size_t words = f.words, rstride = 2 + (size_t)per * f.slot, nout = words + 2 * (size_t)c->world;
    int rc = pred_buffers(c, rstride, nout);
    if (rc) return rc;                                 // (no send buffer: this rank cannot take part)
    // ---- this rank's block; from here on every failure becomes the status word
    const int expect = c->rank < nexperts ? (nexperts - c->rank + c->world - 1) / c->world : 0;
    int nlocal = 0, status = CUGP_OK;
    bool enqueued = false;
    void* sv = (void*)c->stream;                       // the exchange's stream: PredForm::enqueue orders it behind the rows
    if (b && cugp_bcm_num_experts(b, &nlocal)) status = CUGP_ERR_INVALID;
    if (status == CUGP_OK && nlocal != expect) {
        snprintf(buf, sizeof buf, "%s: rank %d holds %d experts, %d of %d expected", call, c->rank,
                 nlocal, expect, nexperts);
        status = cugp_internal_fail(CUGP_ERR_INVALID, buf);
    }
    if (status == CUGP_OK && nlocal > 0) {
        enqueued = true;
        status = f.enqueue(b, c->device, c->pdsend.p + 2, &sv);
    }
    const hipStream_t st = (hipStream_t)sv;
    if (status != CUGP_OK) {
        if (enqueued) (void)cugp_bcm_predict_rows_finish(b);   // nothing enqueued still writes into the send buffer
        e = hipMemsetAsync(c->pdsend.p + 2, 0xff, (rstride - 2) * sizeof(double), st);   // all-ones: NaN rows
        (void)e;
    }
    c->phdr[0] = (double)status;                       // (pinned, read by the copy below before the host waits)
    c->phdr[1] = (double)nlocal;
    e = hipMemcpyAsync(c->pdsend.p, c->phdr, 2 * sizeof(double), hipMemcpyHostToDevice, st);
    if (e != hipSuccess && status == CUGP_OK) status = hip_fail("hipMemcpyAsync (status word)", e);
    // ---- the exchange
    const double* src = c->pdsend.p;                   // a world of one without an id: this rank's block is all of them
    if (c->comm) {
        const ncclResult_t r = rccl().AllGather(c->pdsend.p, c->pdrecv.p, rstride, ncclDouble, c->comm, st);
        if (r != ncclSuccess) {
            if (enqueued) (void)cugp_bcm_predict_rows_finish(b);
            (void)hipStreamSynchronize(st);
            o.fill_nan();
            return nccl_fail("ncclAllGather", r);
        }
        src = c->pdrecv.p;
    }
    rc = f.reduce(src, rstride, c->world, c->pdout.p, st);
    if (rc == CUGP_OK) {
        e = hipMemcpyAsync(c->phout.p, c->pdout.p, nout * sizeof(double), hipMemcpyDeviceToHost, st);
        if (e != hipSuccess) rc = hip_fail("hipMemcpyAsync (prediction)", e);
    }
    e = hipStreamSynchronize(st);               // the one host wait: prediction, collective, reduction, copy
    if (e != hipSuccess && rc == CUGP_OK) rc = hip_fail("hipStreamSynchronize", e);
    if (enqueued && status == CUGP_OK) status = cugp_bcm_predict_rows_finish(b);   // (streams already done: closes them)
    if (rc) { o.fill_nan(); return rc; }
    // ---- every rank reads every rank's status word: the same verdict everywhere
    const double* h = c->phout.p;
    long long total = 0;
    for (int r = 0; r < c->world; r++) {
        const int st = (int)h[words + 2 * r];
        if (st != CUGP_OK) {
            if (r == c->rank) {
                const std::string last = cugp_last_error();
                snprintf(buf, sizeof buf, "%s: rank %d failed (%d): %s", call, r, st, last.c_str());
            } else snprintf(buf, sizeof buf, "%s: rank %d failed (%d)", call, r, st);
            o.fill_nan();
            return cugp_internal_fail(st, buf);
        }
        total += (long long)h[words + 2 * r + 1];
    }
    if (total != nexperts) {
        snprintf(buf, sizeof buf, "%s: the ranks hold %lld experts, %d expected", call, total, nexperts);
        o.fill_nan();
        return cugp_internal_fail(CUGP_ERR_INVALID, buf);
    }
    if (status != CUGP_OK) { o.fill_nan(); return status; }   // (a failure while closing this rank's streams)
    if (o.mean) memcpy(o.mean, h, (size_t)nt * sizeof(double));
    if (o.var) memcpy(o.var, h + nt, (size_t)nt * sizeof(double));
    if (o.dmean) memcpy(o.dmean, h + 2 * (size_t)nt, o.nd * sizeof(double));
    if (o.dvar) memcpy(o.dvar, h + 2 * (size_t)nt + o.nd, o.nd * sizeof(double));
    return CUGP_OK;
}

// what every rank detects identically from the shared arguments of the two prediction calls: no collective
static int predict_args(const char* call, const cugp_comm* c, int per, int nexperts, const double* Xt, int nt,
                        const double* mean, const double* var)
{
    if (!c || per <= 0 || nexperts <= 0 || nt <= 0 || !Xt || !mean || !var || (long long)per * c->world < nexperts) {
        char buf[160];
        snprintf(buf, sizeof buf, "%s: bad argument", call);
        return cugp_internal_fail(CUGP_ERR_INVALID, buf);
    }
    return CUGP_OK;
}

// the two prediction forms: slots [2][nt]; mode < 0 the noisy rows and k_poe_reduce, else latent rows and k_poe_reduce_mode
static PredForm rows_form(const double* Xt, int nt, int nexperts, int mode, int with_noise, double sf2, double sn2)
{
    PredForm f;
    f.slot = f.words = 2 * (size_t)nt;
    f.enqueue = [=](cugp_bcm* b, int device, double* dsend, void** ws) {
        return cugp_bcm_predict_rows_enqueue_form(b, device, Xt, nt, dsend, 2 * (size_t)nt, *ws, mode >= 0 ? 1 : 0);
    };
    f.reduce = [=](const double* src, size_t rstride, int world, double* dout, void* stream) {
        return mode < 0 ? cugp_poe_reduce_enqueue(src, rstride, world, nexperts, nt, dout, stream)
                        : cugp_poe_reduce_mode_enqueue(src, rstride, world, nexperts, nt, mode, sf2, sn2, with_noise ? 1 : 0,
                                                       dout, stream);
    };
    return f;
}

int cugp_bcm_predict_allgather(cugp_bcm* b, cugp_comm* c, int per, int nexperts, const double* Xt, int nt, double* mean,
                               double* var)
{
    if (const int rc = predict_args("cugp_bcm_predict_allgather", c, per, nexperts, Xt, nt, mean, var)) return rc;
    return predict_allgather("cugp_bcm_predict_allgather", b, c, per, nexperts, nt, rows_form(Xt, nt, nexperts, -1, 0, 0.0, 0.0),
                             PredOut{mean, var, nullptr, nullptr, (size_t)nt, 0});
}

// the same exchange with latent rows and k_poe_reduce_mode; sf2, sn2 are arguments: a rank without experts has no BCM
int cugp_bcm_predict_allgather_mode(cugp_bcm* b, cugp_comm* c, int per, int nexperts, const double* Xt, int nt, int mode,
                                    int with_noise, double sf2, double sn2, double* mean, double* var)
{
    if (mode < CUGP_COMBINE_POE || mode > CUGP_COMBINE_RBCM)
        return cugp_internal_fail(CUGP_ERR_INVALID, "cugp_bcm_predict_allgather_mode: unknown mode");
    if (const int rc = predict_args("cugp_bcm_predict_allgather_mode", c, per, nexperts, Xt, nt, mean, var)) return rc;
    return predict_allgather("cugp_bcm_predict_allgather_mode", b, c, per, nexperts, nt,
                             rows_form(Xt, nt, nexperts, mode, with_noise, sf2, sn2),
                             PredOut{mean, var, nullptr, nullptr, (size_t)nt, 0});
}

// The test-input gradients of the combined prediction across the ranks (include/cugp.h): the same exchange with gradient
// rows and k_poe_reduce_grad.  d, sf2 and sn2 are arguments: a rank without experts has no BCM.
int cugp_bcm_predict_grad_allgather(cugp_bcm* b, cugp_comm* c, int per, int nexperts, const double* Xt, int nt, int d,
                                    int mode, int with_noise, double sf2, double sn2, double* mean, double* var,
                                    double* dmean, double* dvar)
{
    const char* why = nullptr;
    if (!c || !Xt) why = "null communicator or Xt";
    else if (nt <= 0 || d <= 0 || per <= 0 || nexperts <= 0) why = "nt, d, per or nexperts <= 0";
    else if ((long long)per * c->world < nexperts) why = "per * world < nexperts";
    else if (mode < CUGP_COMBINE_REFERENCE || mode > CUGP_COMBINE_RBCM) why = "unknown mode";
    else if (!dmean && !dvar) why = "neither dmean nor dvar given";
    else if (b && cugp_bcm_dim(b) != d) why = "d is not the BCM's input dimension";
    if (why) {
        char buf[200];
        snprintf(buf, sizeof buf, "cugp_bcm_predict_grad_allgather: %s", why);
        return cugp_internal_fail(CUGP_ERR_INVALID, buf);
    }
    // The experts' dvar is always asked for: the chain rule reads it for the mean's gradient in every mode.  A NULL dvar
    // only keeps the reduce kernel from writing, and the call from returning, the combined one.
    PredForm f;
    f.slot = f.words = (2 + 2 * (size_t)d) * nt;
    const int want_out = dvar ? 1 : 0;
    f.enqueue = [=](cugp_bcm* bb, int device, double* dsend, void** ws) {
        return cugp_bcm_predict_grad_rows_enqueue(bb, device, Xt, nt, dsend, (2 + 2 * (size_t)d) * nt, *ws, mode >= 0 ? 1 : 0, 1);
    };
    f.reduce = [=](const double* src, size_t rstride, int world, double* dout, void* stream) {
        return cugp_poe_reduce_grad_enqueue(src, rstride, world, nexperts, nt, d, mode, sf2, sn2, with_noise ? 1 : 0, want_out,
                                            dout, stream);
    };
    return predict_allgather("cugp_bcm_predict_grad_allgather", b, c, per, nexperts, nt, f,
                             PredOut{mean, var, dmean, dvar, (size_t)nt, (size_t)nt * d});
}

// ---- the sparse variational model with its rows sharded over ranks (include/cugp.h).  The phases are
// sparse.cpp's (handle.h: ShardEval); here are the two exchanges between them, each ONE ncclAllGather on the evaluation's
// stream (a world of one without an id hands its own block on), and the order that keeps the ranks in step: a rank's own
// failure in front of exchange 1 rides in its header, every rank reads every header behind the wait sp_shard_solve makes
// anyway, and a failure behind that verdict (a HIP error: nothing the ranks could disagree about) still joins exchange 2
// with all-ones rows before it is returned.
static int shard_eval(const char* call, cugp_sparse* const* sh, int nlocal, cugp_comm* c, int per, int nshards, int what,
                      double* F, double* g, int nh, double* gZ)
{
    char buf[256];
    const char* why = nullptr;
    if (!c || !sh || !F) why = "comm, shards or F is NULL";
    else if (nlocal < 1 || per < 1) why = "nlocal < 1 or per < 1";
    else if (what < 0 || what > 2) why = "what must be 0 (F), 1 (F, g) or 2 (F, g, gZ)";
    else if ((what >= 1 && !g) || (what == 2 && !gZ)) why = "g (what >= 1) or gZ (what == 2) is NULL";
    else if (nshards < c->world) why = "nshards < world: a rank without a shard";
    else if ((long long)per * c->world < nshards) why = "per * world < nshards";
    if (why) {
        snprintf(buf, sizeof buf, "%s: %s", call, why);
        return cugp_internal_fail(CUGP_ERR_INVALID, buf);
    }
    cugp::ShardEval e;
    e.sh = sh; e.nlocal = nlocal; e.rank = c->rank; e.world = c->world; e.per = per; e.nshards = nshards; e.what = what;
    e.device = c->device; e.call = call;
    int rc = cugp::sp_shard_begin(e);
    if (rc) return rc;
    if (e.status == CUGP_OK && what >= 1 && nh != e.nh) {
        snprintf(buf, sizeof buf, "%s: nh is not the handles' (cugp_sparse_num_hyper)", call);
        e.status = cugp_internal_fail(CUGP_ERR_INVALID, buf);
    }
    hipError_t he = hipSetDevice(c->device);
    if (he != hipSuccess) return hip_fail("hipSetDevice", he);
    // ---- the exchange buffers.  A failure here (hipSetDevice above included) returns at once: without a send block the rank
    // cannot join exchange 1, and the other ranks wait for it -- the one failure of a rank that is not its status
    const size_t n1 = cugp::SHARD_HDR + (size_t)per * e.slot1, n2 = (size_t)per * e.slot2, nsend = n1 > n2 ? n1 : n2;
    if (nsend > c->sdsend.cap) {
        if ((rc = c->sdsend.grow(nsend, nullptr))) return rc;
        // initialised once, so that no allocator's leftovers travel: P's upper tiles and the slots beyond a rank's shards are
        // sent but never read.  They do not stay zero -- exchange 2 reuses the block from its start, failures fill it with ones
        he = hipMemset(c->sdsend.p, 0, nsend * sizeof(double));
        if (he != hipSuccess) { c->sdsend.release(); return hip_fail("shard exchange buffers", he); }
    }
    if ((c->comm && (rc = c->sdrecv.grow((size_t)c->world * nsend, nullptr))) ||
        (rc = c->shh.grow(cugp::SHARD_HDR + (size_t)per + (size_t)c->world * cugp::SHARD_HDR, nullptr)))
        return rc;
    e.hsend = c->shh.p;
    e.hall = c->shh.p + cugp::SHARD_HDR + per;
    double* send = c->sdsend.p;
    // ---- phase 1 and exchange 1
    cugp::sp_shard_stats(e, send);
    const double* src = send;
    if (c->comm) {
        const ncclResult_t r = rccl().AllGather(send, c->sdrecv.p, n1, ncclDouble, c->comm, e.stream);
        if (r != ncclSuccess) { (void)hipStreamSynchronize(e.stream); return nccl_fail("ncclAllGather", r); }
        src = c->sdrecv.p;
    }
    rc = cugp::sp_shard_solve(e, src, n1);
    if (rc && !e.agreed) return rc;                       // (every rank returns here alike, or the stream itself failed)
    // ---- phase 2 and exchange 2
    if (!e.done && what >= 1) {
        if (rc == CUGP_OK) rc = cugp::sp_shard_rows(e, send);
        if (rc) (void)hipMemsetAsync(send, 0xff, n2 * sizeof(double), e.stream);
        src = send;
        if (c->comm) {
            const ncclResult_t r = rccl().AllGather(send, c->sdrecv.p, n2, ncclDouble, c->comm, e.stream);
            if (r != ncclSuccess) { (void)hipStreamSynchronize(e.stream); return nccl_fail("ncclAllGather", r); }
            src = c->sdrecv.p;
        }
    }
    if (rc) { (void)hipStreamSynchronize(e.stream); return rc; }
    if (!e.done && (rc = cugp::sp_shard_finish(e, src, n2))) return rc;
    return cugp::sp_shard_results(e, F, g, gZ);
}

int cugp_sparse_sharded_bound_grad(cugp_sparse* const* shards, int nlocal, cugp_comm* comm, int per, int nshards, int what,
                                   double* F, double* g, int nh, double* gZ)
{
    return shard_eval("cugp_sparse_sharded_bound_grad", shards, nlocal, comm, per, nshards, what, F, g, nh, gZ);
}

namespace {
struct ShardObjective {
    cugp_sparse* const* sh;
    int nlocal, per, nshards, nh, md;
    cugp_comm* c;
    bool inducing;
    std::vector<double> z;                             // Z as the shards hold it
    bool first = true;                                 // the start point: nothing is written into the shards
    int rc = CUGP_OK;                                  // the first evaluation that failed
    std::string err;                                   // ... and its text
};

// f = -F of the sharded model and its gradient at v = [theta] or [theta, vec Z]: sp_objective / sp_objective_z over every
// local shard.  Every rank is handed the same v by the same loop, so the collectives inside line up.
void shard_objective(void* ctx, const double* v, int nv, double* f, double* gr)
{
    ShardObjective* o = (ShardObjective*)ctx;
    bool ok = true;
    // The start point is the first shard's own state.  It is not written into the others: local shards that disagree in theta
    // or Z are refused by the evaluation, as cugp_sparse_sharded_bound_grad refuses them, not brought into line in passing.
    // Behind the first failure nothing is written either: the call will return that failure and leave the shards as they were
    // (the evaluations go on, so that the ranks' collectives stay matched).
    const bool write = !o->first && o->rc == CUGP_OK;
    o->first = false;
    if (write && o->inducing && memcmp(o->z.data(), v + o->nh, (size_t)o->md * sizeof(double))) {
        for (int i = 0; i < o->nlocal && ok; i++) ok = cugp_sparse_set_inducing(o->sh[i], v + o->nh) == CUGP_OK;
        if (ok) o->z.assign(v + o->nh, v + o->nh + o->md);
    }
    for (int i = 0; i < o->nlocal && ok && write; i++) ok = cugp_sparse_set_loghyper(o->sh[i], v, o->nh) == CUGP_OK;
    double F = NAN;
    // (a rank whose own set_ call failed still evaluates: the others are on their way into the exchange)
    const int rc = shard_eval("cugp_sparse_sharded_cg_solve", o->sh, o->nlocal, o->c, o->per, o->nshards, o->inducing ? 2 : 1, &F,
                              gr, o->nh, gr + o->nh);
    if (rc != CUGP_OK && o->rc == CUGP_OK) {
        o->rc = rc;
        o->err = cugp_last_error();
    }
    ok = ok && rc == CUGP_OK;
    if (ok) *f = -1.0 * F;
    else {
        *f = NAN;
        std::fill(gr, gr + nv, NAN);
    }
}
}  // namespace

int cugp_sparse_sharded_cg_solve(cugp_sparse* const* sh, int nlocal, cugp_comm* c, int per, int nshards, int budget, int inducing,
                                 double* trace, int trace_cap, int* nevals)
{
    const char* call = "cugp_sparse_sharded_cg_solve";
    const char* why = nullptr;
    if (!c || !sh) why = "comm or shards is NULL";
    else if (nlocal < 1 || per < 1) why = "nlocal < 1 or per < 1";
    else if (budget <= 0) why = "budget must be positive";
    else if (nshards < c->world) why = "nshards < world: a rank without a shard";
    else if ((long long)per * c->world < nshards) why = "per * world < nshards";
    else if (!sh[0]) why = "the first shard handle is NULL";
    if (why) {
        char buf[200];
        snprintf(buf, sizeof buf, "%s: %s", call, why);
        return cugp_internal_fail(CUGP_ERR_INVALID, buf);
    }
    int rc, m = 0, d = 0, nh = 0, ns = 0;
    if ((rc = cugp_sparse_shard_info(sh[0], nullptr, &ns, nullptr)) || (rc = cugp_sparse_dims(sh[0], nullptr, &m, &d, nullptr, nullptr)) ||
        (rc = cugp_sparse_num_hyper(sh[0], &nh)))
        return rc;
    if (ns == 0) return cugp_internal_fail(CUGP_ERR_INVALID, "cugp_sparse_sharded_cg_solve: the first handle is an ordinary one (cugp_sparse_create)");
    ShardObjective o{sh, nlocal, per, nshards, nh, m * d, c, inducing != 0, {}};
    std::vector<double> v((size_t)nh);
    if ((rc = cugp_sparse_get_loghyper(sh[0], v.data(), nh))) return rc;
    // An evaluation that fails gives the loop NaN, as cugp_sparse_cg_solve's does, and the loop goes on -- the ranks stay in
    // step --; but the first failure is what the call returns, and then nothing is written into the shards: a failed rank, a
    // mismatch between ranks or local shards that disagree are errors here as in cugp_sparse_sharded_bound_grad.
    if (!o.inducing) {
        if ((rc = cugp::cg_iterates(shard_objective, &o, v.data(), nh, budget, trace, trace_cap, nevals))) return rc;
        if (o.rc) return cugp_internal_fail(o.rc, o.err.c_str());
    } else {
        // cugp_sparse_cg_solve_z's record: [theta, f] of the iterates, the NaN row behind the last one
        o.z.resize((size_t)o.md);
        if ((rc = cugp_sparse_get_inducing(sh[0], o.z.data()))) return rc;
        const int nv = nh + o.md, cap = trace ? std::max(trace_cap, 0) : 0;
        int nrows = 0;
        std::vector<double> rows((size_t)cap * (nv + 1), NAN);
        v.insert(v.end(), o.z.begin(), o.z.end());
        if ((rc = cugp::cg_iterates(shard_objective, &o, v.data(), nv, budget, cap ? rows.data() : nullptr, cap, nevals, &nrows)))
            return rc;
        for (int r = 0; r < nrows + (nrows < cap); r++) {
            std::copy(rows.begin() + (size_t)r * (nv + 1), rows.begin() + (size_t)r * (nv + 1) + nh, trace + (size_t)r * (nh + 1));
            trace[(size_t)r * (nh + 1) + nh] = rows[(size_t)r * (nv + 1) + nv];
        }
        if (o.rc) return cugp_internal_fail(o.rc, o.err.c_str());
        if (memcmp(o.z.data(), v.data() + nh, (size_t)o.md * sizeof(double)))
            for (int i = 0; i < nlocal; i++)
                if ((rc = cugp_sparse_set_inducing(sh[i], v.data() + nh))) return rc;
    }
    for (int i = 0; i < nlocal; i++)
        if ((rc = cugp_sparse_set_loghyper(sh[i], v.data(), nh))) return rc;
    return CUGP_OK;
}

}  // extern "C"
