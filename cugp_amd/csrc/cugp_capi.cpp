// cugp_capi.cpp -- the C-ABI (include/cugp.h) over the gfx950 kernels.
//
// One cugp_gp owns every device buffer of one expert (the reference keeps them as file-scope
// globals, cuda_scalingdist/cuda_gp.cu:20-95, or as Covsum members, covkernel.h:6-18) and one HIP
// stream on which all of its work is ordered.  Layout in HBM (npad = ceil(n/128)*128, row-major):
//   X     n x d              inputs as given
//   y     npad               labels, zero padded
//   A     npad x npad        K (lower tiles), overwritten by its Cholesky factor L
//   T     npad x npad        L^-1 (lower tiles; strictly-upper tiles are scratch of the inverse)
//   U     npad x npad        L^-T (upper tiles) -- the row-major operand of K^-1 = U U^T
//   Kinv  npad x npad        K^-1 (lower tiles, diagonal tiles complete)
// T, U, Kinv are allocated on first use (gradient / prediction), A on first evaluation.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/cugp.h"
#include "group.h"
#include "kernels.h"

using namespace cugp;

namespace {

thread_local std::string g_err;

int fail(int code, const char* what, hipError_t e = hipSuccess)
{
    char buf[512];
    if (e != hipSuccess) snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
    else snprintf(buf, sizeof buf, "%s", what);
    g_err = buf;
    return code;
}

#define HIPCHK(call)                                                        \
    do {                                                                    \
        hipError_t e_ = (call);                                             \
        if (e_ != hipSuccess) return fail(e_ == hipErrorOutOfMemory ? CUGP_ERR_NOMEM : CUGP_ERR_DEVICE, #call, e_); \
    } while (0)

constexpr int NPHASE = 6;
constexpr int MAX_KEV = 4096;   // per-launch event pairs kept between resets
static_assert(MAX_KEV / 2 == cugp::STAMP_STRIDE, "one stamp slot per timed launch");
constexpr int GRAPH_MAX_TILES = 24;   // evaluations up to 3072 rows are replayed as captured graphs
constexpr int PROF_STRIDE = 16; // profiling level 2 times every 16th step launch, rotating (an event pair costs ~5 us of device time);
                                // level 3 times EVERY launch of the MFMA kernels (bench.py's profiled pass: averages comparable with rocprofv3's)
// kinds of timed launches (cugp_get_kernel_stats_kind): the kernels as rocprofv3 names them
enum { KIND_STEP = 0, KIND_WIDE = 1, KIND_BORDER4 = 2, KIND_BORDER2 = 3, KIND_LAUUM4 = 4, KIND_LAUUM2 = 5,
       KIND_LEVEL4 = 6, KIND_LEVEL2 = 7, KIND_BLOCK = 8, KIND_PREDICT = 9, KIND_BUILD = 10, KIND_TRSM = 11, KIND_COV = 12,
       KIND_PGRAD = 13, KIND_LOO = 14, KIND_COUNT = 15 };

// One hardware queue per stream up to 16 (the runtime default is 4): the experts of a BCM on one device each
// drive their own stream, and 16 experts on 4 queues serialise (5.8 ms vs 4.6 ms per evaluation of 16 x 1500
// rows).  Only a default: an existing setting wins, and it has no effect once the HIP runtime is initialised.
struct QueueDefault {
    QueueDefault() { setenv("GPU_MAX_HW_QUEUES", "16", 0); }
} g_queue_default;

}  // namespace

int Scratch::grow(size_t count, void* stream)
{
    if (count <= cap) return CUGP_OK;
    if (stream) HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    release();
    double* q = nullptr;
    const hipError_t e = pinned ? hipHostMalloc((void**)&q, count * sizeof(double), hipHostMallocDefault)
                                : hipMalloc((void**)&q, count * sizeof(double));
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? CUGP_ERR_NOMEM : CUGP_ERR_DEVICE, "scratch allocation", e);
    p = q;
    cap = count;
    return CUGP_OK;
}

void Scratch::release()
{
    if (p) (void)(pinned ? hipHostFree(p) : hipFree(p));
    p = nullptr;
    cap = 0;
}

// set on the lead expert while a group evaluation is being enqueued: every launch then serves all experts
struct GroupCtx {
    Batch bt;                       // device table of the experts' buffers, expert count
    unsigned* tickets = nullptr;    // the experts' step tickets and block-inverse stage counters, contiguous [k][2 nt]
    double* dout = nullptr;         // results [k][row] on the device ...
    double* hout = nullptr;         // ... and pinned, [k][8]: what k_finalize / the fused k_trace write, and every status word
    // ARD groups: row = ARD_ROW_GRAD + nh, and hrows is the pinned [k][row] copy k_finalize_ard writes (gradient
    // evaluations).  The batched k_trtri_block and k_finalize address the pinned rows in 8s, so hout keeps that shape: it
    // holds the status words of every evaluation and the results of the LL-only ones.
    int row = 8;
    double* hrows = nullptr;
    bool overlap = false;           // hand the group's inverse blocks to the lead expert's other streams
    int gcap = 0;                   // barrier workgroups per expert of ONE batched k_trtri_block launch (the experts' smallest share; halved with the overlap)
};

struct cugp_gp {
    int n = 0, d = 0, npad = 0, nt = 0, device = 0;
    hipStream_t stream = nullptr;   // all device work of the handle is ordered here ...
    hipStream_t aux = nullptr;      // ... except the inverse blocks that run beside the factorisation (fork/join by events):
    hipStream_t aux2 = nullptr;     // aux = the large products, aux2 = each block's own small inverse,
    hipStream_t lq = nullptr;       // lq = each block's share of K^-1 (beside the next block's bordering)
    int prio_main = 0, prio_inv = 0;   // priorities the streams were created with (stream, the other three): apply_stream_prio
    bool chain_first = false;       // ... stream runs at the device's highest priority (cugp_chain_first)
    std::vector<hipEvent_t> bev;    // fork events, one per inverse block; last: "Wt of the last block rows complete" (aux -> main)
    std::vector<hipEvent_t> oev;    // "block's own inverse done" events (aux2 -> aux); last block: z, alpha done (aux2 -> main)
    std::vector<hipEvent_t> lev;    // "block's inverse rows final" events (aux -> lq / main -> aux2); last: K^-1 shares so far (-> main)
    double *dX = nullptr, *dy = nullptr, *dA = nullptr, *dT = nullptr, *dU = nullptr, *dKinv = nullptr;
    double *dz = nullptr, *dalpha = nullptr, *dw = nullptr, *d16 = nullptr, *dlogdet = nullptr, *dpart = nullptr, *d64 = nullptr;
    double* dout = nullptr;
    unsigned* dtickets = nullptr;  // [0, nt): one arrival counter per factorisation step (k_syrk_step); [nt, 2 nt): the stage
                                   // counter of the hand-over block that starts at that tile row (k_trtri_block)
    double* hout = nullptr;        // pinned, 8 doubles (ARD: 8 + d + 2)
    int nblocks_trace = 0;
    // the nh log hyper-parameters and the gradient of the last evaluation: {log l, log sigma_f, log sigma_n}, or on an ARD
    // handle (cugp_create_ard; for life) [log l_1 .. log l_d, log sigma_f, log sigma_n].  hhs / dhs then hold the
    // hyper-scalars FOLLOWED by the d weights exp(-theta_c); result rows are 8 + d + 2 doubles (kernels.h: ARD_ROW_GRAD)
    bool ard = false;
    int nh = 3;
    std::vector<double> theta = {0, 0, 0}, last_g = {NAN, NAN, NAN};
    // covariance family (cugp.h CUGP_KERNEL_*, kernels.h KERNEL_*), for life, ARD handles included.  Read wherever one of
    // the four passes that evaluate the kernel function is launched; nothing else depends on it.
    int kernel = KERNEL_SE;
    bool have_data = false;
    bool factor_valid = false;     // A holds L for (data, hp)
    bool inverse_valid = false;    // T, U, Kinv, alpha hold the inverse quantities for (data, hp)
    bool pending = false, pending_grad = false;
    bool zfuse = false;            // record_eval, LL-only: the forward substitution L z = y rides in the factorisation's launches
    bool vec_early = false;        // record_eval: z = L^-1 y, alpha = L^-T z go behind the last block's bordering
    bool vec_done = false;         // ... and were enqueued there
    const GroupCtx* grp = nullptr;  // non-null only inside cugp_group_eval
    Scratch pred;                   // prediction scratch (predict_passes: test inputs, cross-covariance, its product with L^-T, results)
    bool overlap = true;           // hand inverse blocks to the other streams while the factorisation runs
    // a single-stream evaluation is captured once as a HIP graph and replayed: one launch call instead of
    // ~60 (1500 rows) -- with 16 experts on a GPU the host's launch rate was the bound, not the device
    HyperScalars* dhs = nullptr;   // device copy of exp(2*theta): what the kernels of a captured evaluation read
    HyperScalars* hhs = nullptr;   // pinned staging for it (refreshed by a copy node at the head of the graph)
    hipGraphExec_t gexec[2] = {nullptr, nullptr};   // [0] log-likelihood only, [1] with gradient
    unsigned gepoch[2] = {0, 0};   // cfg_epoch the graph was captured under
    // launch-shape tuning of THIS handle (kernels.h TUNE_*): the process defaults as of the last sync_tuning(), except the
    // keys set for this handle alone (cugp_set_handle_tuning)
    int tune[TUNE_COUNT] = {};
    bool tune_own[TUNE_COUNT] = {};
    unsigned cfg_epoch = 1;        // bumped when a launch shape of this handle changed: captured graphs carry launch shapes
    bool counted = false;          // this handle is in g_live[device] (the budget of barrier grids, barrier_cap)
    int bar_quota = -1;            // barrier workgroups reserved for this handle from the device's pool; < 0: not yet asked for
    double last_ll = NAN, last_quad = NAN, last_logdet = NAN;
    // profiling
    int prof = 0;
    hipEvent_t pev[NPHASE + 1] = {};
    bool pev_valid = false;
    std::vector<hipEvent_t> kev;   // start/stop pairs around MFMA launches (profiling level 2)
    std::vector<int> kev_kind;     // per pair: KIND_* below
    std::vector<double> kev_flopv; // per pair: algorithmic flop of the launch
    int kev_used = 0;
    unsigned long long* dstamps = nullptr;   // level 5: [0, STAMP_STRIDE) first-workgroup starts, [STAMP_STRIDE, 2 STAMP_STRIDE) last-workgroup ends
    std::vector<unsigned long long> hstamps;
    unsigned eval_seq = 0;         // factorisations enqueued so far (rotates the launches that get timed)
    double kst_ms[KIND_COUNT] = {}, kst_flop[KIND_COUNT] = {};   // folded sums per kernel kind
    double kst_disp_ms[KIND_COUNT] = {};   // level 5: the same launches from the END of the launch in front of them on their stream
                                           // (= where rocprofv3 puts a back-to-back dispatch's begin) to their own end
    long long kst_launches[KIND_COUNT] = {};
    std::vector<int> kev_prev;     // level 5, per pair: the pair of the launch directly in front of it on the same stream, or -1
    int last_main = -1;            // ... the main stream's latest timed launch while the factorisation is being enqueued
    // joint predictive covariance (cugp_predict_cov / cugp_predict_sample), all created on first use
    cugp_gp* cov_f = nullptr;      // factor handle: its A receives Sigma (ld = its npad), its own stream factors it
    int cov_tiles = 0;             // ... tile rows it was created for (it serves any smaller count)
    hipEvent_t cov_ev = nullptr;   // "Sigma written" (this handle's stream -> cov_f's)
    Scratch cov_scr;               // split-k partial products of k_predict_cov
    Scratch samp;                  // draws: normals Z, F = Z C^T (both [ns pad][ntpad]), packed samples
    // multi-target regression (cugp_set_targets): m further target vectors over the same X and hyper-parameters, all
    // target-major [tg_mpad][npad] and zero beyond n and beyond m; tg_mpad = m rounded up to 128 (k_predict_gemm's tiles)
    int tg_m = 0, tg_mpad = 0;
    double *tg_y = nullptr, *tg_z = nullptr, *tg_a = nullptr;   // Y, Z = Y L^-T, A = Z L^-1 (row t = alpha_t)
    double *tg_part = nullptr;     // trace partials of the multi-target gradient pass (dpart's size)
    double *tg_out = nullptr, *tg_hout = nullptr;   // results row [LL, g (nh), LL_t (m)], device and pinned
    bool tg_valid = false;         // Z, A and tg_row hold for (data, hp, targets) -- read together with inverse_valid
    std::vector<double> tg_row;
    Scratch tg_pred;               // cugp_predict_targets: test inputs, Ks, W, variance, partial means, means
    // appending observations (cugp_append)
    bool bcm_expert = false;       // expert of a cugp_bcm (the experts' common padded size carries n)
    int groups = 0;                // the live cugp_groups that hold the handle (a group's device table carries n)
    bool is_factor = false;        // the internal factor handle (cov_f) of another handle
    bool x_full = false;           // dX holds npad rows (grown by the first append; n rows until then)
    Scratch app;                   // one pass: B = k(Xb, X), P = B L^-T, V = P L^-1 ([128][npad] each) and Qt ([npad][128])
    // leave-one-out cross-validation (cugp_loo): buffers of its own, created on first use -- no buffer any other call reads is written
    double *loo_pt = nullptr;      // [LOO_PT_ROWS][npad] per-point results, then b [npad], the tiles' shares of b [npad / 64][npad]
                                   // and the trace partials [nh][nblocks_trace]: one allocation
    double *loo_out = nullptr, *loo_hout = nullptr;   // results row [L_LOO, g (nh)], device and pinned
    double *loo_B = nullptr, *loo_P = nullptr;        // npad^2 each: K^-1 diag(sqrt c) and its product; first gradient call
};

namespace {

HyperScalars scalars(const cugp_gp* g)
{
    // covkernel.cpp:65-67 -- exp(2*theta) on the host; ARD: no single length scale (ell_sq = 1, not read by its kernels)
    const double* sf = &g->theta[g->nh - 2];
    return HyperScalars{g->ard ? 1.0 : std::exp(g->theta[0] * 2), std::exp(sf[0] * 2), std::exp(sf[1] * 2)};
}

size_t hs_bytes(const cugp_gp* g) { return sizeof(HyperScalars) + (g->ard ? (size_t)g->d * sizeof(double) : 0); }

// ARD: the pinned staging area always holds the current theta's scalars and weights (written where theta is set, with
// the handle's stream idle), so every user of the ARD kernels only has to enqueue the copy in front of its launches
void stage_ard(cugp_gp* g)
{
    *g->hhs = scalars(g);
    double* w = (double*)(g->hhs + 1);
    for (int c = 0; c < g->d; c++) w[c] = std::exp(-g->theta[c]);
}

int upload_hs(cugp_gp* g, hipStream_t s)
{
    HIPCHK(hipMemcpyAsync(g->dhs, g->hhs, hs_bytes(g), hipMemcpyHostToDevice, s));
    return CUGP_OK;
}

// g's covariance function for launches on s.  hd: the device-resident hyper-scalars the launches are to read, if any (a
// captured evaluation, a group's); an ARD handle always reads its own (scalars and weights).  Where they are read, the
// copy that refreshes them from the staging area goes onto s here, in front of the caller's launches.
int cov_fn(cugp_gp* g, hipStream_t s, const HyperScalars* hd, CovFn* cf)
{
    if (g->ard) hd = g->dhs;
    *cf = CovFn{g->kernel, g->ard, scalars(g), hd};
    return hd ? upload_hs(g, s) : CUGP_OK;
}

int refuse_ard(const cugp_gp* g, const char* call, const char* use)
{
    if (!g->ard) return CUGP_OK;
    char buf[256];
    snprintf(buf, sizeof buf, "%s: the handle is ARD (d + 2 hyper-parameters); use %s", call, use);
    return fail(CUGP_ERR_INVALID, buf);
}

int use_device(const cugp_gp* g)
{
    HIPCHK(hipSetDevice(g->device));
    return CUGP_OK;
}

int ensure(double** p, size_t count)
{
    if (*p) return CUGP_OK;
    HIPCHK(hipMalloc((void**)p, count * sizeof(double)));
    return CUGP_OK;
}

int ensure_factor_bufs(cugp_gp* g)
{
    const size_t nn = (size_t)g->npad * g->npad;
    int rc;
    if ((rc = ensure(&g->dA, nn))) return rc;
    if ((rc = ensure(&g->dT, nn))) return rc;   // diagonal-block inverses live in T's diagonal tiles
    if ((rc = ensure(&g->dU, nn))) return rc;
    return CUGP_OK;
}

int ensure_inverse_bufs(cugp_gp* g)
{
    return ensure(&g->dKinv, (size_t)g->npad * g->npad);
}

void drain_kernel_events(cugp_gp* g)
{
    // fold finished per-launch timings into the running sums (everything is on or joined to g->stream, already synchronised)
    const bool stamps = g->prof >= 5 && g->dstamps && g->kev_used > 0;
    if (stamps && hipMemcpy(g->hstamps.data(), g->dstamps, (size_t)2 * STAMP_STRIDE * sizeof(unsigned long long),
                            hipMemcpyDeviceToHost) != hipSuccess) { g->kev_used = 0; return; }
    for (int i = 0; i + 1 < g->kev_used; i += 2) {
        float ms = 0;
        if (stamps) {
            const unsigned long long t0 = g->hstamps[i / 2], t1 = g->hstamps[STAMP_STRIDE + i / 2];
            if (t1 <= t0) continue;                              // (the launch never ran)
            const int kd = g->kev_kind[i / 2];
            g->kst_ms[kd] += (double)(t1 - t0) * 1e-5;           // 100 MHz ticks -> ms
            g->kst_launches[kd] += 1;
            g->kst_flop[kd] += g->kev_flopv[i / 2];
            // dispatch begin .. end as rocprofv3 sees an in-order launch behind another: from the end of the launch in
            // front of it (its workgroups may then still wait for slots held by the other streams' tiles)
            const int pv = g->kev_prev[i / 2];
            const unsigned long long pe = pv >= 0 ? g->hstamps[STAMP_STRIDE + pv] : 0ull;
            g->kst_disp_ms[kd] += (double)(t1 - ((pe > 0 && pe < t1 && pe <= t0) ? pe : t0)) * 1e-5;
            continue;
        }
        if (hipEventElapsedTime(&ms, g->kev[i], g->kev[i + 1]) == hipSuccess) {
            const int kd = g->kev_kind[i / 2];
            g->kst_ms[kd] += ms;
            g->kst_launches[kd] += 1;
            g->kst_flop[kd] += g->kev_flopv[i / 2];
        }
    }
    g->kev_used = 0;
}

Batch B(const cugp_gp* g) { return g->grp ? g->grp->bt : Batch{}; }

// pinned host buffer the evaluation's results land in: the group's ([expert][8]) or the handle's.  Entries 0..5: LL, the
// three gradients, y'K^-1y, log|K| (k_finalize); entry 6: set by a kernel whose bounded wait ran out (k_trtri_block)
double* host_out(const cugp_gp* g) { return g->grp ? g->grp->hout : g->hout; }
// ... and the one a gradient evaluation's final sums land in: an ARD group's rows are wider than its status rows
double* host_grad_out(const cugp_gp* g) { return g->grp && g->grp->hrows ? g->grp->hrows : host_out(g); }

// ---- tuning: process defaults (cugp_set_tuning) under a lock, one copy per handle ----
std::mutex g_tune_mu;
int g_tune_default[TUNE_COUNT];
bool g_tune_default_init = false;

void tune_defaults_locked()
{
    if (!g_tune_default_init) {
        for (int k = 0; k < TUNE_COUNT; k++) g_tune_default[k] = g_tune_init[k];
        // CUGP_TUNE="key=value,key=value": process defaults from the environment (A/B runs of whole test suites)
        if (const char* e = getenv("CUGP_TUNE")) {
            while (*e) {
                char* end = nullptr;
                const long k = strtol(e, &end, 10);
                if (end == e || *end != '=') break;
                e = end + 1;
                const long v = strtol(e, &end, 10);
                if (end == e) break;
                if (k >= 0 && k < TUNE_COUNT) g_tune_default[k] = (int)v;
                e = *end == ',' ? end + 1 : end;
                if (*end != ',' ) break;
            }
        }
        g_tune_default_init = true;
    }
}

// Take the process defaults over into the handle (keys it owns excepted); called where an API call starts to
// enqueue.  A changed launch shape invalidates the handle's captured graphs.
void sync_tuning(cugp_gp* g)
{
    std::lock_guard<std::mutex> lk(g_tune_mu);
    tune_defaults_locked();
    bool changed = false;
    for (int k = 0; k < TUNE_COUNT; k++)
        if (!g->tune_own[k] && g->tune[k] != g_tune_default[k]) {
            if (k != TUNE_GRAPHS) changed = true;
            g->tune[k] = g_tune_default[k];
        }
    if (changed) g->cfg_epoch++;
}

// While an API call enqueues for handle g the launchers of kernels.hip read g's tuning (thread-local pointer).
struct TuneScope {
    const int* prev;
    explicit TuneScope(cugp_gp* g) : prev(t_tune) { sync_tuning(g); t_tune = g->tune; }
    ~TuneScope() { t_tune = prev; }
};

// ---- budget of barrier grids ----
// k_trtri_block is a grid whose workgroups wait for each other: every launch of it needs all G of its workgroups
// resident at once.  One launch is safe by construction (G <= 64, far below the 512 slots; workgroups of a launch are
// dispatched in order), but launches of DIFFERENT handles interleave on the device: 9 handles x 64 workgroups exceed the
// slots, every launch is partly resident and each waits for workgroups that cannot be dispatched (a stall of seconds,
// then NaN results).  So the handles of a device share a pool of 384 barrier workgroups, and a handle's share is
// RESERVED: taken from the pool at the handle's first barrier launch -- 384 / (live handles on the device at that
// moment), at most 64, at most what is left -- kept unchanged for the handle's lifetime and returned when it is destroyed.
// A fixed share is what a captured graph may bake in: graphs captured while few handles were alive keep their grids, and
// handles created later get what is left of the pool (none: their block inverses go launch by launch, k_trtri_diag +
// k_trtri_level, which wait for nothing -- the same bits).  A handle whose inverse blocks run beside its factorisation can
// have TWO barrier launches in flight (the block in front of the last on aux2, the last block's on the main stream):
// each takes half the share.  The sum over everything in flight therefore stays <= 384 of the 512 slots whatever the
// interleaving, so some launch always gets the workgroups it is missing.
// (Per process: handles of other processes on the same GPU are not seen.)
constexpr int BARRIER_POOL = 384;
std::atomic<int> g_live[64];
std::atomic<int> g_bar_used[64];
int barrier_share(cugp_gp* g)
{
    if (g->bar_quota >= 0) return g->bar_quota;
    const int dev = g->device >= 0 && g->device < 64 ? g->device : 63;
    int live = g_live[dev].load(std::memory_order_relaxed);
    if (live < 1) live = 1;
    int want = live > 24 ? 0 : BARRIER_POOL / live;
    if (want > TRTRI_BLOCK_MAXWG) want = TRTRI_BLOCK_MAXWG;
    int used = g_bar_used[dev].load(std::memory_order_relaxed), grant;
    do {
        grant = want < BARRIER_POOL - used ? want : BARRIER_POOL - used;
        if (grant < 8) grant = 0;                              // (not worth a barrier grid: launch by launch)
    } while (grant > 0 && !g_bar_used[dev].compare_exchange_weak(used, used + grant, std::memory_order_relaxed));
    g->bar_quota = grant;
    return grant;
}
void barrier_release(cugp_gp* g)
{
    if (g->bar_quota > 0) g_bar_used[g->device >= 0 && g->device < 64 ? g->device : 63].fetch_sub(g->bar_quota, std::memory_order_relaxed);
    g->bar_quota = -1;
}
// workgroups ONE barrier launch of this handle may hold; 0: none (launch by launch)
int barrier_cap(cugp_gp* g)
{
    if (g->grp) return g->grp->gcap;                           // (the group's: cugp_group_enqueue)
    const int share = barrier_share(g);
    return g->overlap && share >= 16 ? share / 2 : share;
}

// block rows per hand-over to the other streams, or as tuned; 0 = no hand-over (everything on the main stream after the
// factorisation).  A handle evaluated alone: by size, cugp_pipe_block_for.  Expert groups and the experts of a BCM (a
// lone BCM expert is a group of one, and an expert gives the same bits grouped or not): about a sixteenth of the
// matrix, at least 2 tiles, single tiles up to 8 tiles -- the rule their A/B runs were made under (16 x 1500,
// 8 x 3000, 4 x 6000 rows), left as it was.
int pipe_block(const cugp_gp* g, bool with_inverse)
{
    const bool overlap = g->grp ? g->grp->overlap : g->overlap;
    int w = (with_inverse && overlap) ? g->tune[TUNE_PIPE_BLOCK] : 0;
    if (w < 0) w = !g->grp && !g->bcm_expert ? cugp_pipe_block_for(g->nt)
                                            : g->nt <= 8 ? 1 : ((g->nt + 8) / 16 > 2 ? (g->nt + 8) / 16 : 2);
    return w >= g->nt ? 0 : w;
}

// ---- stream priorities ----
// The factorisation is a chain of ~2 nt launches, most of them small (k_trsm_inv64: 30 workgroups, 7 us alone); the
// inverse streams beside it launch 1000-2000 workgroups of 134 us each, and a chain launch that arrives behind one waits
// for a whole round of them to drain (8192 rows: a dozen times per evaluation, 140-190 us each).  With the chain's
// stream at the highest priority those waits get shorter and fewer, not none (k_trsm_inv64 3.05 -> 2.62 ms per
// evaluation, 14 -> 11 launches over 100 us), and the inverse launches longer.  That pays only where the chain competes with
// large launches of the same handle: not in expert groups or BCMs (prioritised streams share few hardware queues, which
// serialised the experts of a BCM evaluated on one device: 8 x 3000 rows 6.6 -> 17.4 ms), not without the hand-over,
// and not below TUNE_PRIO_MIN_NT tile rows.  Results never depend on it: the order on every stream is fixed.
bool want_chain_first(const cugp_gp* g)
{
    const int v = g->tune[TUNE_STREAM_PRIO];
    if (v != 0) return (v & 4) == 0 && (v & 1) != 0;
    return !g->bcm_expert && g->groups == 0 && !g->is_factor && g->overlap && g->tune[TUNE_PIPE_BLOCK] != 0 &&
           g->nt >= g->tune[TUNE_PRIO_MIN_NT];
}

// Create the handle's four streams, or re-create them where the priorities they were created with are no longer the
// ones the handle's tuning, membership and size ask for.  Called with no evaluation in flight and never from inside
// one (creation, cugp_set_data, cugp_set_handle_tuning, cugp_set_overlap, joining a group or a BCM, becoming another
// handle's factor handle); without a change it costs two comparisons.  Leaving a group (cugp_group_destroy) is NOT such a
// place: a former expert stays at default priorities until its next cugp_set_data.  Captured graphs are captured again (they replay on the stream they are launched into, but
// the epoch is the one rule for "the handle's launch set-up changed").
int apply_stream_prio(cugp_gp* g)
{
    const int v = g->tune[TUNE_STREAM_PRIO];
    const bool first = want_chain_first(g), inv_low = (v & 4) == 0 && (v & 2) != 0;
    int plo = 0, phi = 0;
    if (first || inv_low) HIPCHK(hipDeviceGetStreamPriorityRange(&plo, &phi));
    const int pmain = first ? phi : 0, pinv = inv_low ? plo : 0;
    hipStream_t* const all[4] = {&g->stream, &g->aux, &g->aux2, &g->lq};
    if (g->stream && pmain == g->prio_main && pinv == g->prio_inv) return CUGP_OK;
    // The new set is created first and the old one given up only when all four exist: a failure leaves the handle on
    // the streams it had (never on a null stream, which would be the device's default stream).
    hipStream_t fresh[4] = {nullptr, nullptr, nullptr, nullptr};
    hipError_t e = hipSuccess;
    for (int i = 0; i < 4 && e == hipSuccess; i++) {
        const int p = i == 0 ? pmain : pinv;
        // (default priorities everywhere: the plain call, as before there was a rule)
        e = pmain == 0 && pinv == 0 ? hipStreamCreateWithFlags(&fresh[i], hipStreamNonBlocking)
                                    : hipStreamCreateWithPriority(&fresh[i], hipStreamNonBlocking, p);
    }
    for (int i = 0; i < 4 && e == hipSuccess; i++)
        if (*all[i]) e = hipStreamSynchronize(*all[i]);
    if (e != hipSuccess) {
        for (hipStream_t s : fresh)
            if (s) (void)hipStreamDestroy(s);
        return fail(CUGP_ERR_DEVICE, "apply_stream_prio: the handle keeps the streams it had", e);
    }
    for (int i = 0; i < 4; i++) {
        if (*all[i]) (void)hipStreamDestroy(*all[i]);
        *all[i] = fresh[i];
    }
    g->prio_main = pmain;
    g->prio_inv = pinv;
    g->chain_first = first;
    g->cfg_epoch++;
    return CUGP_OK;
}

// one timed launch: event pair + bookkeeping.  Levels 2 and 3 record an event in front of and behind the launch on its
// stream; level 4 hands the pair to the launch itself (hipExtLaunchKernelGGL: the dispatch's own begin / end, no extra
// packets on the stream -- the schedule of the timed pass, and the durations rocprofv3 --kernel-trace reports)
// level 5: no events at all -- the launch's own workgroups stamp a slot of g->dstamps (kernels.hip LaunchStamp)
struct TimedLaunch {
    cugp_gp* g; hipStream_t s; bool on, ext;
    // chain: this launch goes out on the main stream directly behind the main stream's latest timed launch
    TimedLaunch(cugp_gp* g_, hipStream_t s_, bool want, bool chain = false)
        : g(g_), s(s_), on(want && g_->kev_used + 2 <= (int)g_->kev.size()), ext(g_->prof >= 4)
    {
        if (!on) { if (chain) g->last_main = -1; return; }       // an untimed launch breaks the chain
        g->kev_prev[g->kev_used / 2] = chain ? g->last_main : -1;
        if (chain) g->last_main = g->kev_used / 2;
        if (g->prof >= 5) stamp_next_launch(g->dstamps + g->kev_used / 2);
        else if (ext) time_next_launch(g->kev[g->kev_used], g->kev[g->kev_used + 1]);
        else if (hipEventRecord(g->kev[g->kev_used], s) != hipSuccess) on = false;
    }
    ~TimedLaunch() { if (on && ext && timing_pending()) { time_next_launch(nullptr, nullptr); stamp_next_launch(nullptr); } }   // the launch did not happen
    void done(int kind, double flop)
    {
        if (!on) return;
        if (ext) { if (timing_pending()) return; }            // (armed but not consumed: nothing was launched)
        else if (hipEventRecord(g->kev[g->kev_used + 1], s) != hipSuccess) return;
        g->kev_kind[g->kev_used / 2] = kind;
        g->kev_flopv[g->kev_used / 2] = flop;
        g->kev_used += 2;
    }
};

// is this launch one of the timed ones?  level 2: one in `every`, rotating with `phase`; levels 3 and 4: all
bool sampled(const cugp_gp* g, int phase, int every) { return g->prof >= 3 || (g->prof == 2 && phase % every == 0); }

// algorithmic flop of the inverse's tile products (multiply + add; a k tile that is triangular counts half).
// border step 1, one chunk: Wt(tj < c1, ti in [ra, ra+rw)) (+)= sum_{k in [max(tj,c0), c1)} U[tj][k] L[ti][k]
double border1_flop(int rw, int c0, int c1)
{
    double kt = 0;
    for (int tj = 0; tj < c1; tj++) kt += (c1 - (tj > c0 ? tj : c0)) - (tj >= c0 ? 0.5 : 0.0);   // U[tj][tj] is triangular
    return kt * rw * 2.0 * TILE * TILE * TILE;
}
// border step 2: T(ti in [a, a+w), tj < a) = -sum_{k in [a, ti]} T[ti][k] Wt[tj][k]   (T[ti][ti] triangular)
double border2_flop(int a, int w)
{
    double kt = 0;
    for (int i = 0; i < w; i++) kt += i + 0.5;
    return kt * a * 2.0 * TILE * TILE * TILE;
}
// K^-1 share of inverse rows [a, a+w): Kinv(ti,tj) (+)= sum_{k in [max(ti,a), a+w)} U[ti][k] U[tj][k]^T, tj <= ti < a+w
double lauum_flop(int a, int w)
{
    double kt = 0;
    for (int ti = 0; ti < a + w; ti++) {
        const double k = (a + w) - (ti > a ? ti : a);
        kt += (ti + 1) * k - (ti >= a ? 0.5 * (ti + 1) : 0.0) - (ti >= a ? 0.5 * k : 0.0);   // triangular k tile; diagonal output tile
    }
    return kt * 2.0 * TILE * TILE * TILE;
}
// one level of recursive doubling over nt tiles, blocks of s: both steps move |A| x |B| tiles with k ranges up to s
double level_flop(int nt, int s, int step)
{
    double kt = 0;
    for (int a0 = 0; a0 + s < nt; a0 += 2 * s) {
        int sb = nt - (a0 + s);
        if (sb > s) sb = s;
        if (step == 1) for (int ja = 0; ja < s; ja++) kt += (s - ja - 0.5) * sb;       // k from tj to the end of A
        else for (int ib = 0; ib < sb; ib++) kt += (ib + 0.5) * s;                     // k from b0 to ti
    }
    return kt * 2.0 * TILE * TILE * TILE;
}

// The block's own inverse: T and U of the diagonal block of rows [a, a + wb), on stream o.  One launch (k_trtri_block:
// diagonal-tile inverses + every doubling level, stage counter tickets[nt + a]) for hand-over blocks; the whole-matrix
// form (wb > TRTRI_BLOCK_MAX_TILES: large levels want 128x128 tiles and fill the chip) stays launch by launch.
int enqueue_block_own_inverse(cugp_gp* g, int a, int wb, hipStream_t o)
{
    const int ld = g->npad;
    const int gcap = barrier_cap(g);                         // this handle's share of the device's barrier workgroups; 0: none
    if (wb <= TRTRI_BLOCK_MAX_TILES && gcap > 0) {
        unsigned* base = g->grp ? g->grp->tickets : g->dtickets;
        TimedLaunch tl(g, o, sampled(g, (a / (wb > 0 ? wb : 1)) + (int)g->eval_seq, 4));
        launch_trtri_block(g->dA, g->d64, g->dT, g->dU, ld, a, wb, base + g->nt + a, g->dlogdet, g->nt + a, o, B(g), gcap,
                           host_out(g));
        double fl = 0;
        for (int s = 1; s < wb; s *= 2) fl += level_flop(wb, s, 1) + level_flop(wb, s, 2);
        tl.done(KIND_BLOCK, fl);
        return CUGP_OK;
    }
    const size_t off = (size_t)a * TILE * ld + (size_t)a * TILE;
    launch_trtri_diag(g->dA, ld, a, wb, g->d64, g->dT, g->dU, o, B(g));
    for (int s = 1; s < wb; s *= 2)
        for (int step = 1; step <= 2; step++) {
            TimedLaunch tl(g, o, sampled(g, a + s + step + (int)g->eval_seq, 16));  // small launches: one in sixteen
            const int wm = launch_trtri_level(g->dA, g->dT, g->dU, ld, wb, s, step, o, B(g), off);
            if (wm) tl.done(wm == 4 ? KIND_LEVEL4 : KIND_LEVEL2, level_flop(wb, s, step));
        }
    return CUGP_OK;
}

// Inverse quantities of block rows [a, b): T and U = T^T (diagonal-tile inverses, doubling inside the block,
// bordering against the finished rows [0, a)) and the block's share of K^-1 = T^T T (when Kinv is wanted).
// The block's own inverse is a chain of small launches; on its own stream `xs` (when given) it runs beside
// the large products of the previous block instead of in front of this block's.  The K^-1 share only needs
// the block's rows of U: on its own stream `lq` (when given) it runs beside the NEXT block's bordering -- two
// independent large launches in flight fill each other's last, partly empty round of workgroups.
int enqueue_inverse_block(cugp_gp* g, int a, int b, bool kinv, hipStream_t x, hipStream_t xs, hipEvent_t own_done,
                          hipStream_t lq = nullptr, hipEvent_t rows_final = nullptr, bool before_last = false)
{
    const int ld = g->npad, wb = b - a;
    hipStream_t o = xs ? xs : x;
    int rc0;
    if ((rc0 = enqueue_block_own_inverse(g, a, wb, o))) return rc0;
    if (xs) {
        HIPCHK(hipEventRecord(own_done, xs));
        HIPCHK(hipStreamWaitEvent(x, own_done, 0));
    }
    // rows [a, b): their Wt was accumulated chunk by chunk while the earlier blocks became final
    const bool timed2 = sampled(g, (a / (wb > 0 ? wb : 1)) + (int)g->eval_seq, 4);   // large launches: every fourth block
    if (a > 0) {
        TimedLaunch tl(g, x, timed2);
        const int wm = launch_trtri_border2(g->dA, g->dT, g->dU, ld, a, wb, x, B(g));
        if (wm) tl.done(wm == 4 ? KIND_BORDER4 : KIND_BORDER2, border2_flop(a, wb));
    }
    auto kinv_share = [&](hipStream_t st) {
        TimedLaunch tl(g, st, timed2);
        const int wm = launch_lauum(g->dU, g->dKinv, ld, a, wb, st, B(g));
        tl.done(wm == 4 ? KIND_LAUUM4 : KIND_LAUUM2, lauum_flop(a, wb));
    };
    if (kinv && lq) {
        HIPCHK(hipEventRecord(rows_final, x));
        HIPCHK(hipStreamWaitEvent(lq, rows_final, 0));
        kinv_share(lq);
        if (before_last) HIPCHK(hipEventRecord(g->lev.back(), lq));      // the shares of K^-1 so far (enqueue_last_block)
    }
    // ... and these rows, now final, go into the Wt of every row below them
    if (b < g->nt) {
        TimedLaunch tl(g, x, timed2);
        const int wm = launch_trtri_border1(g->dA, g->dT, g->dU, ld, b, g->nt - b, a, b, x, B(g));
        if (wm) tl.done(wm == 4 ? KIND_BORDER4 : KIND_BORDER2, border1_flop(g->nt - b, a, b));
    }
    if (before_last) HIPCHK(hipEventRecord(g->bev.back(), x));           // Wt of the last rows is complete
    if (b == g->nt && g->vec_early) {
        // L^-1 is complete: z = L^-1 y and alpha = L^-T z run BESIDE the last share of K^-1 (~130 us at N = 8192)
        // instead of after it on the main stream: on the stream of the block's own inverse (idle by now) when the
        // share follows on this one
        hipStream_t vs = x;
        if (kinv && !lq && xs && rows_final) {
            HIPCHK(hipEventRecord(rows_final, x));
            HIPCHK(hipStreamWaitEvent(xs, rows_final, 0));
            vs = xs;
        }
        launch_trmv_lower(g->dT, g->npad, g->npad, g->dy, g->dz, vs, B(g));
        launch_trmv_upper(g->dU, g->npad, g->npad, g->dz, g->dalpha, vs, B(g));
        g->vec_done = true;
        if (vs != x) {
            HIPCHK(hipEventRecord(own_done, xs));
            if (kinv && !lq) kinv_share(x);
            HIPCHK(hipStreamWaitEvent(x, own_done, 0));             // x's last event covers both again
            return CUGP_OK;
        }
    }
    if (kinv && !lq) {
        kinv_share(x);
        if (before_last) HIPCHK(hipEventRecord(g->lev.back(), x));
    }
    return CUGP_OK;
}

// The LAST block of inverse rows [a, nt) on the MAIN stream: behind the factorisation nothing else is left there, and
// the block's chain -- diagonal inverses, doubling, bordering, its share of K^-1, then the traces -- crosses no stream
// boundary any more (every hand-over cost ~10 us of the evaluation's serial tail: 3 of them are 5 % of a 1500-row
// evaluation).  The other streams are waited for exactly where their results are needed: Wt complete (bev.back(), recorded
// behind the previous block's border1 launches) before the bordering, the earlier shares of K^-1 (lev.back()) before this
// one -- so the bordering no longer queues behind the previous block's share.  z = L^-1 y and alpha = L^-T z run beside
// the share on aux2.
int enqueue_last_block(cugp_gp* g, int a, int idx)
{
    const int nt = g->nt, ld = g->npad, wb = nt - a;
    hipStream_t m = g->stream;
    int rc0;
    if ((rc0 = enqueue_block_own_inverse(g, a, wb, m))) return rc0;
    const bool timed2 = sampled(g, (a / (wb > 0 ? wb : 1)) + (int)g->eval_seq, 4);
    HIPCHK(hipStreamWaitEvent(m, g->bev.back(), 0));
    {
        TimedLaunch tl(g, m, timed2);
        const int wm = launch_trtri_border2(g->dA, g->dT, g->dU, ld, a, wb, m, B(g));
        if (wm) tl.done(wm == 4 ? KIND_BORDER4 : KIND_BORDER2, border2_flop(a, wb));
    }
    // z = L^-1 y, alpha = L^-T z: beside the share on aux2 when they are long enough to be worth two hand-overs
    // (~130 us at 8192 rows, ~90 us for 16 x 1500 rows against ~10 us per hand-over; 14 us at 1500 rows: in line there)
    const bool beside = g->vec_early && nt * (g->grp ? g->grp->bt.count : 1) > 24;
    if (g->vec_early) {
        hipStream_t vs = m;
        if (beside) {
            HIPCHK(hipEventRecord(g->lev[idx], m));
            HIPCHK(hipStreamWaitEvent(g->aux2, g->lev[idx], 0));
            vs = g->aux2;
        }
        launch_trmv_lower(g->dT, g->npad, g->npad, g->dy, g->dz, vs, B(g));
        launch_trmv_upper(g->dU, g->npad, g->npad, g->dz, g->dalpha, vs, B(g));
        if (beside) HIPCHK(hipEventRecord(g->oev[idx], g->aux2));
        g->vec_done = true;
    }
    HIPCHK(hipStreamWaitEvent(m, g->lev.back(), 0));
    {
        TimedLaunch tl(g, m, timed2);
        const int wm = launch_lauum(g->dU, g->dKinv, ld, a, wb, m, B(g));
        tl.done(wm == 4 ? KIND_LAUUM4 : KIND_LAUUM2, lauum_flop(a, wb));
    }
    if (beside) HIPCHK(hipStreamWaitEvent(m, g->oev[idx], 0));
    return CUGP_OK;
}

int phase_mark(cugp_gp* g, int i);
int fetch_eval(cugp_gp* g);

// level 5: the slots the timed launches enqueued from here on stamp (the sums of the ones before were drained by the
// fetch that synchronised them): starts to ~0, ends to 0, on the handle's stream in front of those launches
int reset_stamps(cugp_gp* g)
{
    if (g->prof < 5 || !g->dstamps) return CUGP_OK;
    HIPCHK(hipMemsetAsync(g->dstamps, 0xff, (size_t)STAMP_STRIDE * sizeof(unsigned long long), g->stream));
    HIPCHK(hipMemsetAsync(g->dstamps + STAMP_STRIDE, 0, (size_t)STAMP_STRIDE * sizeof(unsigned long long), g->stream));
    return CUGP_OK;
}


// The shares of K^-1 on a stream of their own (beside the next block's bordering) or behind their block's bordering:
// for a group of experts two large launches in flight fill each other's partly empty last rounds (-3...-6 % per
// evaluation at 16x1500, 8x3000, 4x6000); for a single matrix the extra hand-over costs what it gains or more
// (1500: +1.9 %, 6000: +3.3 %, 8192 / 10000: +-0.3 %, 16384: +0.7 %).  TUNE_LAUUM_STREAM: 0 never, 1 groups, 2 always.
bool kinv_stream(const cugp_gp* g)
{
    const int v = g->tune[TUNE_LAUUM_STREAM];
    return v >= 2 || (v == 1 && g->grp != nullptr);
}

// (the fork event bev[idx] was recorded by the caller, on the factorisation's stream behind the panel solve that made
//  the rows final)
int fork_inverse_block(cugp_gp* g, int a, int b, int idx, bool before_last)
{
    HIPCHK(hipStreamWaitEvent(g->aux, g->bev[idx], 0));
    HIPCHK(hipStreamWaitEvent(g->aux2, g->bev[idx], 0));
    const bool own = kinv_stream(g);
    return enqueue_inverse_block(g, a, b, true, g->aux, g->aux2, g->oev[idx], own ? g->lq : nullptr, g->lev[idx],
                                 before_last);
}

// What step kb of the two-speed factorisation launches (pure column arithmetic, shared with the test hook
// cugp_potrf_plan so the schedule can be replayed on a CPU: every tile must see every k exactly once, in order).
//
// Steps are grouped in panels of P.  The step launch (k_syrk_step, K = 128, with the next diagonal block
// factored inside it) updates only the NEAR window: the tile columns [kb+1, F_p), F_p fixed per panel and chosen
// so that the window holds about `near` tiles at the panel's first step -- enough to fill the chip for the
// ~45 us the diagonal block needs, so the latency-bound chain stays hidden exactly as in the classic form.
// The FAR columns [F_p, nt) get the whole panel at once, K = P*128, from k_syrk_wide when the panel's last
// column is solved (one pass over their C tiles instead of P: the tile product costs a fixed ~12 us per C tile
// + 30.5 us per 128 of K).  F_p never decreases, so a column is either inside every later window or was
// brought up to date by every earlier wide pass.  Once the window reaches the last column (small trailing
// matrices, where the chain is the bound anyway) this IS the classic right-looking form.
struct StepPlan {
    int wide_k0, wide_kw;      // k tiles of the wide update issued at this step (after its panel solve) ...
    int wa0, wa1;              // ... over the tile columns [wa0, wa1); empty: none
    int wcol;                  // step launch: columns [kb+1, kb+1+wcol) ...
    int ks;                    // ... receive the k tiles [ks, kb] in one pass (sub-panels; ks = kb: one k tile per step)
};

static int tri_tiles(int n) { return n * (n + 1) / 2; }

// far boundary of panel p: first tile column NOT in the near window
int far_boundary(int nt, int P, int near, int p)
{
    int F = 0;
    for (int q = 0; q <= p; q++) {                                    // monotone over the panels
        const int k0 = q * P, m = nt - k0 - 1;                        // trailing size at the panel's first step
        int wc = P;                                                   // at least the panel itself and one more column
        while (wc < m && (wc >= m ? tri_tiles(m) : tri_tiles(wc) + (m - wc) * wc) < near) wc++;
        int f = k0 + 1 + wc;
        if (f < (q + 1) * P + 1) f = (q + 1) * P + 1;
        if (f > nt) f = nt;
        // the far pass costs whole rounds of 512 tile slots (134 us each at K = 512): move the boundary up to three
        // columns out if that makes its tri(nt - f) tiles end close to a full round
        {
            int best = f;
            double bw = 2.0;
            for (int c = f; c <= f + 3 && c < nt; c++) {
                const int tiles = tri_tiles(nt - c), rem = tiles % 512;
                const double waste = rem == 0 ? 0.0 : (512.0 - rem) / 512.0 / (tiles / 512 + 1);   // idle share of the pass
                if (waste < bw - 0.02) { bw = waste; best = c; }
            }
            f = best;
        }
        if (f > F) F = f;
    }
    return F;
}

// Sub-panels (S > 1 steps, aligned from step 0; S divides P): the near window is right-looking from sub-panel to
// sub-panel and left-looking inside one.  The step launch of a sub-panel's LAST step updates the whole window with the
// sub-panel's S k tiles in one pass (K = 128 S: the fixed cost of a pass over a C tile -- 256 KB of C traffic, prologue,
// dispatch -- is paid once per S steps; K = 128 ran at 45 TF/s, 256 at 55, 512 at 59); the steps before it update only
// the column the chain needs next, with the k tiles of the sub-panel so far (K = 128 .. 128 (S - 1)).  A column inside
// sub-panel [s0, s0 + S) has then seen every k < s0 (earlier window and wide passes) and [s0, column) (its own step).
StepPlan plan_step(int nt, int P, int near, int kb, int S = 1)
{
    StepPlan sp{0, 0, 0, 0, nt - kb - 1, kb};
    if (S < 1 || S > SUBPANEL_MAX || (P > 1 && P % S != 0)) S = 1;
    int F = nt;
    if (P > 1) {
        const int p = kb / P, i = kb % P;
        F = far_boundary(nt, P, near, p);
        if (i == P - 1 && F < nt) {
            sp.wide_k0 = p * P;
            sp.wide_kw = P;
            sp.wa0 = F;
            sp.wa1 = nt;
        }
    }
    sp.ks = kb - kb % S;
    sp.wcol = (kb % S == S - 1) ? F - (kb + 1) : 1;
    return sp;
}

// panel width of the look-ahead factorisation for this handle (1 = classic right-looking, K = 128 per pass)
int panel_width(const cugp_gp* g)
{
    int P = g->tune[TUNE_PANEL];
    if (P < 2 || g->nt < g->tune[TUNE_PANEL_MIN_NT] || g->nt < 3 * P) return 1;
    return P > 32 ? 32 : P;
}

// algorithmic flop of a trailing update over the tile columns [ca, cb) of an nt-tile matrix with kw k tiles:
// entries on or below the diagonal only (a diagonal tile counts half), multiply + add
double trailing_flop(int nt, int ca, int cb, int kw)
{
    if (cb > nt) cb = nt;
    double entries = 0;
    for (int c = ca; c < cb; c++) entries += ((double)(nt - c) - 0.5) * TILE * TILE;
    return entries * kw * TILE * 2.0;
}

// Blocked right-looking Cholesky of A (lower).  Handle's stream, two launches per step:
//   panel solve(k)  ->  [trailing update(k) + factorisation of diagonal block k+1] in ONE launch
// (k_syrk_step: the latency-bound diagonal block runs inside the update launch), and in the two-speed form
// (panels of P > 1 steps, plan_step above; cpp_matrixalgebra/blocked_cholesky.cpp:221-262 is the b = 2 ancestor)
// one k_syrk_wide pass per panel over the far columns.  Every tile sees its updates in a fixed order whatever
// the timing: results are reproducible.
// with_inverse: L^-1 and K^-1 are built block row by block row on further streams as the rows of L become final.
int enqueue_continue(cugp_gp* g);

// zeroed_tickets: the arrival counters a launch already in front of this on the stream has zeroed (record_eval: the
// covariance build, launch_kbuild's `tickets` argument) -- it must be the very buffer the step launches count in, or
// the counters are cleared here (a stale counter means a diagonal block factored twice or never).
int enqueue_potrf(cugp_gp* g, bool with_inverse, bool mark = false, const unsigned* zeroed_tickets = nullptr)
{
    int rc;
    const int nt = g->nt, ld = g->npad;
    const int w = pipe_block(g, with_inverse);
    const int P = panel_width(g);
    const int near = g->tune[TUNE_NEAR_TILES];
    const int S = g->tune[TUNE_SUBPANEL];
    hipStream_t m = g->stream;                              // the whole factorisation is ordered on the handle's stream
    int nblk = 0, done = 0;                                 // blocks forked so far, block rows handed over
    struct Fork { int a, b; };
    std::vector<Fork> forks;
    const bool chain_first = nt * (g->grp ? g->grp->bt.count : 1) <= 24;
    // (Round 2 handed the first nt - 2w block rows of small matrices over in ONE late block: every hand-over cost the
    //  main stream a bubble the ~50-us chain steps could not afford.  With the round-3 chain -- ~32 us per step -- the
    //  fine-grained hand-over wins at every size again: 1500 rows 0.77 -> 0.65 ms, 2 x 1500 rows 0.80 -> 0.73 ms.)
    g->eval_seq++;
    const unsigned* my_tickets = g->grp ? g->grp->tickets : g->dtickets;
    if (zeroed_tickets && zeroed_tickets == my_tickets) {}   // (the covariance build in front of it did that)
    else if (g->grp) HIPCHK(hipMemsetAsync(g->grp->tickets, 0, (size_t)g->grp->bt.count * ticket_count(nt) * sizeof(unsigned), m));
    else HIPCHK(hipMemsetAsync(g->dtickets, 0, (size_t)ticket_count(nt) * sizeof(unsigned), m));
    launch_potf2(g->dA, ld, 0, g->d16, g->d64, g->dlogdet, m, B(g));
    const bool zf = g->zfuse && !with_inverse;              // (LL-only: z = L^-1 y inside the panel-solve and step launches)
    g->last_main = -1;
    const bool l5 = g->prof >= 5;                           // level 5: every launch of the factorisation's stream is stamped
    for (int kb = 0; kb + 1 < nt; kb++) {
        {
            TimedLaunch tl(g, m, l5, true);
            launch_trsm_inv64(g->dA, g->d64, ld, kb, nt, m, B(g), zf ? g->dz : nullptr, g->dw);
            tl.done(KIND_TRSM, 2.0 * (nt - kb - 1) * TILE * (double)TILE * TILE / 2);      // (triangular solve: half a product)
        }
        // block rows < kb+1 of L are final, and so are the columns <= kb of every row below them
        const int b = kb + 1;
        const bool hand_over = w > 0 && b - done >= w;
        if (hand_over) HIPCHK(hipEventRecord(g->bev[nblk], m));
        const StepPlan sp = plan_step(nt, P, near, kb, S);
        if (sp.wa1 > sp.wa0) {
            // panel p is factored (its last panel solve is enqueued): the far columns get the panel's K = P*128 in
            // one pass, before the next panel's first step widens the near window into them
            TimedLaunch tl(g, m, g->prof >= 2, true);
            launch_syrk_wide(g->dA, ld, nt, sp.wide_k0, sp.wide_kw, sp.wa0, sp.wa1, (kb / P) & 1, m, B(g));
            tl.done(KIND_WIDE, trailing_flop(nt, sp.wa0, sp.wa1, sp.wide_kw));
        }
        // level 2 times a rotating eighth of the step launches (every step is sampled once in 8 evaluations):
        // an event pair around every launch costs several percent of the evaluation
        TimedLaunch tl(g, m, sampled(g, kb + (int)g->eval_seq, PROF_STRIDE), true);
        // (look-ahead form: plain stores -- the panel solve that follows reads the column at once, and reading
        //  freshly non-temporally stored tiles took it 50 us instead of 16)
        launch_syrk_step(g->dA, ld, kb, nt, g->d16, g->d64, g->dlogdet, g->dtickets, m, B(g), sp.wcol, sp.ks,
                         zf ? g->dz : nullptr, g->dw);
        tl.done(KIND_STEP, trailing_flop(nt, kb + 1, kb + 1 + sp.wcol, kb + 1 - sp.ks));
        if (hand_over) {
            // The block's own 6-8 launches take the host 15-35 us.  Where a chain step is shorter than that (small
            // matrices: ~35 us per step) they are enqueued behind the WHOLE chain of the factorisation -- enqueued at
            // the hand-over they left the main stream dry at every block, and the host is far ahead of the device
            // again before the first block is due.  Long steps (many tiles, or a group of experts): right here,
            // behind the step launch, so that the inverse streams start as early as the device allows even under a
            // slow host (a profiler doubles the host's cost per launch).
            if (chain_first) forks.push_back({done, b});
            else if ((rc = fork_inverse_block(g, done, b, nblk, nt - b <= w))) return rc;    // (true: the next block is the last)
            done = b;
            nblk++;
        }
    }
    if (mark && (rc = phase_mark(g, 2))) return rc;         // end of the factorisation on the main stream
    for (size_t i = 0; i < forks.size(); i++)
        if ((rc = fork_inverse_block(g, forks[i].a, forks[i].b, (int)i, nt - forks[i].b <= w))) return rc;
    if (w > 0) {
        if ((rc = enqueue_last_block(g, done, nblk))) return rc;      // waits for everything the other streams still do
    } else if (with_inverse) {
        if ((rc = enqueue_inverse_block(g, 0, nt, true, m, nullptr, nullptr))) return rc;
    } else if (zf) {
        // the last block's share of z (its diagonal block was factored inside the last step launch); nothing else of the
        // inverse is needed for a log-likelihood
        launch_trsm_inv64(g->dA, g->d64, ld, nt - 1, nt, m, B(g), g->dz, g->dw);
    } else {
        // inverses of all diagonal factor blocks at once (off the factorisation's critical path)
        launch_trtri_diag(g->dA, ld, 0, nt, g->d64, g->dT, g->dU, m, B(g));
    }
    HIPCHK(hipGetLastError());
    return CUGP_OK;
}

int enqueue_trtri(cugp_gp* g)
{
    for (int s = 1; s < g->nt; s *= 2) {
        launch_trtri_level(g->dA, g->dT, g->dU, g->npad, g->nt, s, 1, g->stream);
        launch_trtri_level(g->dA, g->dT, g->dU, g->npad, g->nt, s, 2, g->stream);
    }
    HIPCHK(hipGetLastError());
    return CUGP_OK;
}

int phase_mark(cugp_gp* g, int i)
{
    if (g->prof >= 1) HIPCHK(hipEventRecord(g->pev[i], g->stream));
    return CUGP_OK;
}

// K build + factorisation (+ inverse quantities, traces when want_grad); results land in dout.
// hd: the kernels read the hyper-scalars from device memory (a copy node refreshes it) -- the captured form.
int record_eval(cugp_gp* g, bool want_grad, const HyperScalars* hd)
{
    int rc;
    hipStream_t s = g->stream;
    CovFn cf;
    if ((rc = cov_fn(g, s, hd, &cf))) return rc;
    if ((rc = phase_mark(g, 0))) return rc;
    unsigned* const tickets = g->grp ? g->grp->tickets : g->dtickets;
    if ((rc = reset_stamps(g))) return rc;
    {
        TimedLaunch tl(g, s, g->prof >= 5);
        launch_kbuild(g->dX, g->n, g->d, g->npad, cf, g->dA, false, s, B(g), tickets);   // also zeroes the step tickets
        // (bytes, not flop: the lower 64x64 tiles of K written once + X read)
        tl.done(KIND_BUILD, (double)trace_num_blocks(g->npad) * 64 * 64 * 8 + (double)g->n * g->d * 8);
    }
    if ((rc = phase_mark(g, 1))) return rc;
    g->vec_early = want_grad;
    g->vec_done = false;
    g->zfuse = !want_grad && g->tune[TUNE_ZFUSE] != 0;
    if (g->zfuse) {                                            // the running right-hand side of the forward substitution: w = y
        if (g->grp) launch_copy_y_to_w(g->npad, s, B(g));
        else HIPCHK(hipMemcpyAsync(g->dw, g->dy, (size_t)g->npad * sizeof(double), hipMemcpyDeviceToDevice, s));
    }
    rc = enqueue_potrf(g, want_grad, true, tickets);           // + L^-1 and K^-1, block rows at a time beside it
    g->vec_early = false;
    const bool zfused = g->zfuse;
    g->zfuse = false;
    if (rc) return rc;
    if (want_grad) {
        if ((rc = phase_mark(g, 3))) return rc;              // "trtri" phase = what is left of the inverse blocks
        if ((rc = phase_mark(g, 4))) return rc;
        if (!g->vec_done) {
            launch_trmv_lower(g->dT, g->npad, g->npad, g->dy, g->dz, s, B(g));        // z = L^-1 y
            launch_trmv_upper(g->dU, g->npad, g->npad, g->dz, g->dalpha, s, B(g));    // alpha = L^-T z
        }
        // traces and the final sums in ONE launch: the last block of k_trace finishes the evaluation (kernels.hip)
        launch_trace(g->dX, g->n, g->d, g->npad, cf, g->dKinv, g->dalpha, g->dpart, s, B(g), g->dz, g->dlogdet, g->dout,
                     host_grad_out(g), tickets + 2 * g->nt);
    } else {
        if ((rc = phase_mark(g, 3))) return rc;
        if ((rc = phase_mark(g, 4))) return rc;
        if (!zfused) {                                         // (TUNE_ZFUSE = 0: the substitution as 2 nt launches behind the factorisation)
            if (g->grp) launch_copy_y_to_w(g->npad, s, B(g));
            else HIPCHK(hipMemcpyAsync(g->dw, g->dy, (size_t)g->npad * sizeof(double), hipMemcpyDeviceToDevice, s));
            launch_trsv_lower(g->dA, g->dT, g->npad, g->nt, g->dw, g->dz, s, B(g));   // L z = y
        }
        launch_finalize(g->dz, g->npad, g->n, g->dlogdet, g->nt, nullptr, 0, cf.h, g->dout, host_out(g), s, cf.hd, B(g));
    }
    if ((rc = phase_mark(g, 5))) return rc;
    HIPCHK(hipGetLastError());
    // (k_finalize wrote the results into the pinned host buffer itself)
    return CUGP_OK;
}

// The evaluation as a captured HIP graph on g's stream (g->grp's group while that is set, with the group's graphs):
// captured once per launch-shape epoch -- gexec / gepoch [0] log-likelihood only, [1] with gradient -- then replayed.
// The kernels read the hyper-scalars from g->dhs, which the graph's first node refreshes from g->hhs.
int replay_eval(cugp_gp* g, hipGraphExec_t gexec[2], unsigned gepoch[2], bool want_grad)
{
    const int gi = want_grad ? 1 : 0;
    if (!gexec[gi] || gepoch[gi] != g->cfg_epoch) {
        if (gexec[gi]) (void)hipGraphExecDestroy(gexec[gi]);
        gexec[gi] = nullptr;
        hipGraph_t graph = nullptr;
        HIPCHK(hipStreamBeginCapture(g->stream, hipStreamCaptureModeThreadLocal));
        const int rc = record_eval(g, want_grad, g->dhs);
        hipError_t e = hipStreamEndCapture(g->stream, &graph);   // always leave capture mode
        if (rc == CUGP_OK && e == hipSuccess) e = hipGraphInstantiate(&gexec[gi], graph, nullptr, nullptr, 0);
        if (graph) (void)hipGraphDestroy(graph);
        if (rc || e != hipSuccess) {
            gexec[gi] = nullptr;
            return rc ? rc : fail(CUGP_ERR_DEVICE, "graph capture", e);
        }
        gepoch[gi] = g->cfg_epoch;
    }
    HIPCHK(hipGraphLaunch(gexec[gi], g->stream));
    return CUGP_OK;
}

int enqueue_eval(cugp_gp* g, bool want_grad)
{
    int rc;
    if (!g->have_data) return fail(CUGP_ERR_INVALID, "no training data set (cugp_set_data)");
    if ((rc = fetch_eval(g))) return rc;                      // one evaluation in flight per handle
    TuneScope ts(g);
    if ((rc = use_device(g))) return rc;
    if ((rc = ensure_factor_bufs(g))) return rc;
    if (want_grad && (rc = ensure_inverse_bufs(g))) return rc;
    if (const int pe = prepare_kernels())                     // per-device launch attributes (dynamic LDS sizes)
        return fail(CUGP_ERR_DEVICE, "hipFuncSetAttribute(MaxDynamicSharedMemorySize)", (hipError_t)pe);
    g->factor_valid = g->inverse_valid = false;

    // Replay a captured graph when the evaluation is a single-stream sequence (no hand-over to the other
    // streams) and nothing is being timed; otherwise enqueue the launches one by one.
    // (measured: 16 x 1500 rows 4.7 -> 4.1 ms, 2 x 1500 rows 1.25 -> 1.18 ms; nothing to gain above ~3000 rows)
    const bool graph = g->tune[TUNE_GRAPHS] != 0 && g->prof == 0 && g->nt <= GRAPH_MAX_TILES &&
                       pipe_block(g, want_grad) == 0;
    if (graph && !g->ard) *g->hhs = scalars(g);              // (ARD: staged where theta was set, weights included)
    if ((rc = graph ? replay_eval(g, g->gexec, g->gepoch, want_grad)
                    : record_eval(g, want_grad, nullptr))) return rc;
    g->pending = true;
    g->pending_grad = want_grad;
    g->pev_valid = g->prof >= 1;
    return CUGP_OK;
}

// Gradient quantities from a factor that is already valid (a log-likelihood-only evaluation at the same data and
// hyper-parameters came first: Covsum::compute_loglikelihood then compute_gradient_loghyperparam, or the value and
// gradient halves of the evaluation-sparing line search): L^-1, K^-1, alpha, traces -- no rebuild of K, no second
// factorisation.  One stream (the factorisation it could have run beside is over).
int enqueue_continue(cugp_gp* g)
{
    int rc;
    if ((rc = fetch_eval(g))) return rc;
    if (!g->factor_valid) return fail(CUGP_ERR_INVALID, "no valid factor to continue from");
    TuneScope ts(g);
    if ((rc = use_device(g))) return rc;
    if ((rc = ensure_inverse_bufs(g))) return rc;
    if (const int pe = prepare_kernels())
        return fail(CUGP_ERR_DEVICE, "hipFuncSetAttribute(MaxDynamicSharedMemorySize)", (hipError_t)pe);
    hipStream_t s = g->stream;
    g->inverse_valid = false;
    HIPCHK(hipMemsetAsync(g->dtickets + g->nt, 0, (size_t)(g->nt + 1) * sizeof(unsigned), s));     // k_trtri_block's stage counters, k_trace's arrival counter
    if ((rc = reset_stamps(g))) return rc;
    if ((rc = enqueue_inverse_block(g, 0, g->nt, true, s, nullptr, nullptr))) return rc;
    launch_trmv_lower(g->dT, g->npad, g->npad, g->dy, g->dz, s);
    launch_trmv_upper(g->dU, g->npad, g->npad, g->dz, g->dalpha, s);
    CovFn cf;
    if ((rc = cov_fn(g, s, nullptr, &cf))) return rc;
    launch_trace(g->dX, g->n, g->d, g->npad, cf, g->dKinv, g->dalpha, g->dpart, s, {}, g->dz, g->dlogdet, g->dout, g->hout,
                 g->dtickets + 2 * g->nt);
    HIPCHK(hipGetLastError());
    g->pending = true;
    g->pending_grad = true;
    g->pev_valid = false;
    return CUGP_OK;
}

// After a synchronise that follows ANY launch sequence with k_trtri_block in it: did one of its bounded stage waits
// run out?  (pinned status word, entry 6 of a result row.)  Reads and clears it.
bool barrier_expired(double* row)
{
    if (row[6] == 0.0) return false;
    row[6] = 0.0;
    return true;
}

// nothing of the evaluation is kept: NaN results, and the next call starts from the covariance build
void discard_eval(cugp_gp* g)
{
    g->factor_valid = g->inverse_valid = false;
    g->last_ll = g->last_quad = g->last_logdet = NAN;
    for (double& v : g->last_g) v = NAN;
}

// The results of g's evaluation from its 8-double host row (host_out) -- or, when a bounded wait inside a kernel ran out
// (k_trtri_block's stage barrier), none: nothing of that evaluation is to be trusted, and it is discarded (false).
bool read_result_row(cugp_gp* g, double* row, bool grad)
{
    if (barrier_expired(row)) {
        discard_eval(g);
        return false;
    }
    g->last_ll = row[0];
    g->last_quad = row[4];
    g->last_logdet = row[5];
    g->factor_valid = true;
    if (grad) {
        const double* gr = row + (g->ard ? ARD_ROW_GRAD : 1);
        for (int i = 0; i < g->nh; i++) g->last_g[i] = gr[i];
        g->inverse_valid = true;
        g->tg_valid = false;                                 // (a new inverse: the multi-target results are stale)
    }
    return true;
}

int fetch_eval(cugp_gp* g)
{
    if (!g->pending) return CUGP_OK;
    int rc;
    if ((rc = use_device(g))) return rc;
    HIPCHK(hipStreamSynchronize(g->stream));
    g->pending = false;
    const bool ok = read_result_row(g, g->hout, g->pending_grad);
    if (g->prof >= 2) drain_kernel_events(g);
    if (!ok) return fail(CUGP_ERR_DEVICE, "a stage barrier of k_trtri_block ran out of polls (the evaluation was abandoned; results NaN)");
    return CUGP_OK;
}

}  // namespace

extern "C" {

int cugp_version(void) { return 100; }

#ifndef CUGP_BUILD_ID
#define CUGP_BUILD_ID "unknown"
#endif
const char* cugp_build_id(void) { return CUGP_BUILD_ID; }

const char* cugp_last_error(void) { return g_err.c_str(); }

int cugp_device_count(int* count)
{
    if (!count) return CUGP_ERR_INVALID;
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) { *count = 0; return fail(CUGP_ERR_NODEVICE, "hipGetDeviceCount", e); }
    *count = c;
    return CUGP_OK;
}

int cugp_create(int n, int d, int device, cugp_gp** out) { return cugp_create_padded(n, d, device, 0, out); }

static int create_handle(int n, int d, int device, int npad_min, bool ard, cugp_gp** out, int kernel = KERNEL_SE);

int cugp_create_padded(int n, int d, int device, int npad_min, cugp_gp** out)
{
    return create_handle(n, d, device, npad_min, false, out);
}

int cugp_create_kernel(int n, int d, int device, int npad_min, int kernel, cugp_gp** out)
{
    if (kernel < 0 || kernel >= KERNEL_COUNT)
        return fail(CUGP_ERR_INVALID, "cugp_create_kernel: unknown kernel kind (0 SE, 1 Matern 3/2, 2 Matern 5/2)");
    return create_handle(n, d, device, npad_min, false, out, kernel);
}

int cugp_kernel_kind(const cugp_gp* g, int* kernel)
{
    if (!g || !kernel) return fail(CUGP_ERR_INVALID, "cugp_kernel_kind: null argument");
    *kernel = g->kernel;
    return CUGP_OK;
}

int cugp_create_ard(int n, int d, int device, cugp_gp** out) { return create_handle(n, d, device, 0, true, out); }
int cugp_create_ard_padded(int n, int d, int device, int npad_min, cugp_gp** out)
{
    return create_handle(n, d, device, npad_min, true, out);
}

// one length scale per input dimension with any covariance family (kind 0: cugp_create_ard_padded, the same launches)
int cugp_create_ard_kernel(int n, int d, int device, int npad_min, int kernel, cugp_gp** out)
{
    if (kernel < 0 || kernel >= KERNEL_COUNT)
        return fail(CUGP_ERR_INVALID, "cugp_create_ard_kernel: unknown kernel kind (0 SE, 1 Matern 3/2, 2 Matern 5/2)");
    return create_handle(n, d, device, npad_min, true, out, kernel);
}

static int create_handle(int n, int d, int device, int npad_min, bool ard, cugp_gp** out, int kernel)
{
    if (!out || n <= 0 || d <= 0) return fail(CUGP_ERR_INVALID, "cugp_create: n, d must be positive");
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess || cnt <= 0)
        return fail(CUGP_ERR_NODEVICE, "no HIP device visible (libcugp has no CPU fallback)");
    if (device < 0 || device >= cnt) return fail(CUGP_ERR_INVALID, "cugp_create: device index out of range");
    cugp_gp* g = new (std::nothrow) cugp_gp;
    if (!g) return fail(CUGP_ERR_NOMEM, "host allocation");
    g->n = n; g->d = d; g->device = device;
    g->ard = ard;
    g->kernel = kernel;
    if (ard) { g->nh = d + 2; g->theta.assign(g->nh, 0.0); g->last_g.assign(g->nh, NAN); }
    const size_t nrow = ard ? (size_t)ARD_ROW_GRAD + g->nh : 8, ncol = g->nh;
    g->nt = ((n > npad_min ? n : npad_min) + TILE - 1) / TILE;
    g->npad = g->nt * TILE;
    g->nblocks_trace = trace_num_blocks(g->npad);
    *out = nullptr;
    {   // the process defaults as they stand now
        std::lock_guard<std::mutex> lk(g_tune_mu);
        tune_defaults_locked();
        for (int k = 0; k < TUNE_COUNT; k++) g->tune[k] = g_tune_default[k];
    }
    g_live[device < 64 ? device : 63].fetch_add(1, std::memory_order_relaxed);
    g->counted = true;
    hipError_t e = hipSetDevice(device);
    // the four streams, at the priorities the handle's size and tuning ask for (want_chain_first; a handle that joins a
    // group or a BCM later gets them re-created there)
    if (e == hipSuccess && apply_stream_prio(g) != CUGP_OK) e = hipErrorUnknown;
    for (std::vector<hipEvent_t>* v : {&g->bev, &g->oev, &g->lev}) {
        v->assign((size_t)g->nt + 2, nullptr);
        for (size_t i = 0; i < v->size() && e == hipSuccess; i++) e = hipEventCreateWithFlags(&(*v)[i], hipEventDisableTiming);
    }
    if (e == hipSuccess) e = hipMalloc((void**)&g->dX, (size_t)n * d * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&g->dy, (size_t)g->npad * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&g->dz, (size_t)g->npad * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&g->dalpha, (size_t)g->npad * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&g->dw, (size_t)g->npad * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&g->d16, (size_t)g->nt * 8 * 256 * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&g->d64, (size_t)g->nt * 8192 * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&g->dlogdet, (size_t)g->nt * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&g->dpart, (size_t)g->nblocks_trace * ncol * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&g->dout, nrow * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&g->dtickets, (size_t)ticket_count(g->nt) * sizeof(unsigned));
    if (e == hipSuccess) e = hipHostMalloc((void**)&g->hout, nrow * sizeof(double), hipHostMallocDefault);
    if (e == hipSuccess) memset(g->hout, 0, nrow * sizeof(double));   // (entry 6 is the status word fetch_eval reads)
    if (e == hipSuccess) e = hipHostMalloc((void**)&g->hhs, hs_bytes(g), hipHostMallocDefault);
    if (e == hipSuccess) e = hipMalloc((void**)&g->dhs, hs_bytes(g));
    if (e == hipSuccess && ard) stage_ard(g);
    for (int i = 0; i <= NPHASE && e == hipSuccess; i++) e = hipEventCreate(&g->pev[i]);
    if (e != hipSuccess) {
        int code = fail(e == hipErrorOutOfMemory ? CUGP_ERR_NOMEM : CUGP_ERR_DEVICE, "cugp_create", e);
        cugp_destroy(g);
        return code;
    }
    *out = g;
    return CUGP_OK;
}

int cugp_destroy(cugp_gp* g)
{
    if (!g) return CUGP_OK;
    (void)hipSetDevice(g->device);
    if (g->stream) (void)hipStreamSynchronize(g->stream);
    if (g->aux) (void)hipStreamSynchronize(g->aux);
    if (g->aux2) (void)hipStreamSynchronize(g->aux2);
    if (g->lq) (void)hipStreamSynchronize(g->lq);
    barrier_release(g);                                   // (no barrier grid of this handle runs any more)
    if (g->counted) g_live[g->device >= 0 && g->device < 64 ? g->device : 63].fetch_sub(1, std::memory_order_relaxed);
    if (g->cov_f) (void)cugp_destroy(g->cov_f);           // (synchronises its own stream first)
    if (g->cov_ev) (void)hipEventDestroy(g->cov_ev);
    g->cov_scr.release();
    g->samp.release();
    g->tg_pred.release();
    g->app.release();
    if (g->tg_hout) (void)hipHostFree(g->tg_hout);
    if (g->loo_hout) (void)hipHostFree(g->loo_hout);
    for (double* p : {g->loo_pt, g->loo_out, g->loo_B, g->loo_P})
        if (p) (void)hipFree(p);
    double* bufs[] = {g->dX, g->dy, g->dA, g->dT, g->dU, g->dKinv, g->dz, g->dalpha, g->dw, g->d16, g->dlogdet,
                      g->dpart, g->dout, g->d64, g->tg_y, g->tg_z, g->tg_a, g->tg_part, g->tg_out};
    for (double* p : bufs)
        if (p) (void)hipFree(p);
    if (g->dtickets) (void)hipFree(g->dtickets);
    if (g->dstamps) (void)hipFree(g->dstamps);
    g->pred.release();
    if (g->hout) (void)hipHostFree(g->hout);
    if (g->hhs) (void)hipHostFree(g->hhs);
    if (g->dhs) (void)hipFree(g->dhs);
    for (hipGraphExec_t x : g->gexec)
        if (x) (void)hipGraphExecDestroy(x);
    for (int i = 0; i <= NPHASE; i++)
        if (g->pev[i]) (void)hipEventDestroy(g->pev[i]);
    for (hipEvent_t e : g->kev) (void)hipEventDestroy(e);
    for (std::vector<hipEvent_t>* v : {&g->bev, &g->oev, &g->lev})
        for (hipEvent_t e : *v)
            if (e) (void)hipEventDestroy(e);
    if (g->aux) (void)hipStreamDestroy(g->aux);
    if (g->aux2) (void)hipStreamDestroy(g->aux2);
    if (g->lq) (void)hipStreamDestroy(g->lq);
    if (g->stream) (void)hipStreamDestroy(g->stream);
    delete g;
    return CUGP_OK;
}

int cugp_set_overlap(cugp_gp* g, int enable)
{
    if (!g) return CUGP_ERR_INVALID;
    int rc;
    if ((rc = use_device(g)) || (rc = fetch_eval(g))) return rc;
    g->overlap = enable != 0;                                // (a captured graph is only used without hand-over)
    return apply_stream_prio(g);                             // (without the hand-over nothing runs beside the chain)
}

int cugp_dims(const cugp_gp* g, int* n, int* d, int* npad)
{
    if (!g) return CUGP_ERR_INVALID;
    if (n) *n = g->n;
    if (d) *d = g->d;
    if (npad) *npad = g->npad;
    return CUGP_OK;
}

static int set_data_common(cugp_gp* g, const double* X, const double* y, hipMemcpyKind kind)
{
    if (!g || !X || !y) return fail(CUGP_ERR_INVALID, "cugp_set_data: null argument");
    int rc;
    if ((rc = use_device(g))) return rc;
    if ((rc = fetch_eval(g))) return rc;
    sync_tuning(g);                                        // (the process defaults may have moved since the handle was created)
    if ((rc = apply_stream_prio(g))) return rc;
    HIPCHK(hipMemcpyAsync(g->dX, X, (size_t)g->n * g->d * sizeof(double), kind, g->stream));
    HIPCHK(hipMemsetAsync(g->dy, 0, (size_t)g->npad * sizeof(double), g->stream));
    HIPCHK(hipMemcpyAsync(g->dy, y, (size_t)g->n * sizeof(double), kind, g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));
    g->have_data = true;
    g->factor_valid = g->inverse_valid = false;
    return CUGP_OK;
}

int cugp_set_data(cugp_gp* g, const double* X, const double* y) { return set_data_common(g, X, y, hipMemcpyHostToDevice); }

int cugp_set_data_device(cugp_gp* g, const double* dX, const double* dy)
{
    return set_data_common(g, dX, dy, hipMemcpyDeviceToDevice);
}

// ---- hyper-parameters and results: the 3-entry calls and their _ard twins are argument checks (refuse_ard / want_ard)
// in front of one body over the handle's nh entries ----
// A set that changes nothing (and holds no NaN) keeps the factor.  ARD: the staging area may still be read by a copy
// enqueued for a prediction, so the stream runs dry before it is written again.
static int set_theta(cugp_gp* g, const double* th)
{
    int rc;
    if ((rc = fetch_eval(g))) return rc;
    bool changed = false;
    for (int i = 0; i < g->nh; i++) changed = changed || th[i] != g->theta[i] || std::isnan(th[i]);
    if (!changed) return CUGP_OK;
    if (g->ard) {
        if ((rc = use_device(g))) return rc;
        HIPCHK(hipStreamSynchronize(g->stream));
    }
    g->factor_valid = g->inverse_valid = false;
    g->theta.assign(th, th + g->nh);
    if (g->ard) stage_ard(g);
    return CUGP_OK;
}

static void get_theta(const cugp_gp* g, double* th) { std::copy(g->theta.begin(), g->theta.end(), th); }

// the last evaluation's results (either pointer may be null)
static void copy_grad(const cugp_gp* g, double* ll, double* gr)
{
    if (ll) *ll = g->last_ll;
    if (gr) std::copy(g->last_g.begin(), g->last_g.end(), gr);
}

int cugp_set_loghyper(cugp_gp* g, const double hp[3])
{
    if (!g || !hp) return CUGP_ERR_INVALID;
    if (const int rc = refuse_ard(g, "cugp_set_loghyper", "cugp_set_loghyper_ard")) return rc;
    return set_theta(g, hp);
}

int cugp_get_loghyper(const cugp_gp* g, double hp[3])
{
    if (!g || !hp) return CUGP_ERR_INVALID;
    if (const int rc = refuse_ard(g, "cugp_get_loghyper", "cugp_get_loghyper_ard")) return rc;
    get_theta(g, hp);
    return CUGP_OK;
}

// the _ard calls' common argument check, before any device call: no null argument and a possible nh (the handle is not
// looked at before that), then an ARD handle and nh == d + 2
static int want_ard(const cugp_gp* g, int nh, const char* call, bool pointers_ok = true)
{
    char buf[256];
    if (!g || !pointers_ok || nh < 3) {
        snprintf(buf, sizeof buf, "%s: null argument or nh < 3", call);
        return fail(CUGP_ERR_INVALID, buf);
    }
    if (!g->ard) {
        snprintf(buf, sizeof buf, "%s: the handle is isotropic (3 hyper-parameters); create it with cugp_create_ard", call);
        return fail(CUGP_ERR_INVALID, buf);
    }
    if (nh != g->d + 2) {
        snprintf(buf, sizeof buf, "%s: nh = %d, the handle has d + 2 = %d hyper-parameters", call, nh, g->d + 2);
        return fail(CUGP_ERR_INVALID, buf);
    }
    return CUGP_OK;
}

int cugp_num_hyper(const cugp_gp* g, int* nh)
{
    if (!g || !nh) return fail(CUGP_ERR_INVALID, "cugp_num_hyper: null argument");
    *nh = g->nh;
    return CUGP_OK;
}

int cugp_set_loghyper_ard(cugp_gp* g, const double* hp, int nh)
{
    if (const int rc = want_ard(g, nh, "cugp_set_loghyper_ard", hp != nullptr)) return rc;
    return set_theta(g, hp);
}

int cugp_get_loghyper_ard(const cugp_gp* g, double* hp, int nh)
{
    if (const int rc = want_ard(g, nh, "cugp_get_loghyper_ard", hp != nullptr)) return rc;
    get_theta(g, hp);
    return CUGP_OK;
}

int cugp_loglik_grad_enqueue(cugp_gp* g, int want_grad)
{
    if (!g) return CUGP_ERR_INVALID;
    int rc;
    if ((rc = fetch_eval(g))) return rc;
    return enqueue_eval(g, want_grad != 0);
}

int cugp_loglik_grad_fetch(cugp_gp* g, double* ll, double gr[3])
{
    if (!g) return CUGP_ERR_INVALID;
    int rc;
    if (gr && (rc = refuse_ard(g, "cugp_loglik_grad_fetch", "cugp_loglik_grad_fetch_ard"))) return rc;
    if ((rc = fetch_eval(g))) return rc;
    copy_grad(g, ll, gr);
    return CUGP_OK;
}

int cugp_loglik(cugp_gp* g, double* ll)
{
    if (!g || !ll) return CUGP_ERR_INVALID;
    int rc;
    if ((rc = fetch_eval(g))) return rc;
    if (!g->factor_valid) {
        if ((rc = enqueue_eval(g, false))) return rc;
        if ((rc = fetch_eval(g))) return rc;
    }
    *ll = g->last_ll;
    return CUGP_OK;
}

int cugp_loglik_grad(cugp_gp* g, double* ll, double gr[3])
{
    if (!g) return CUGP_ERR_INVALID;
    int rc;
    if (gr && (rc = refuse_ard(g, "cugp_loglik_grad", "cugp_loglik_grad_ard"))) return rc;
    if ((rc = fetch_eval(g))) return rc;
    if (!g->inverse_valid) {
        // a valid factor (cugp_loglik came first at the same point) is continued, not recomputed
        if ((rc = (g->factor_valid && g->prof == 0) ? enqueue_continue(g) : enqueue_eval(g, true))) return rc;
        if ((rc = fetch_eval(g))) return rc;
    }
    copy_grad(g, ll, gr);
    return CUGP_OK;
}

int cugp_grad(cugp_gp* g, double gr[3])
{
    if (!g) return CUGP_ERR_INVALID;
    if (const int rc = refuse_ard(g, "cugp_grad", "cugp_loglik_grad_ard")) return rc;
    return cugp_loglik_grad(g, nullptr, gr);
}

int cugp_loglik_grad_fetch_ard(cugp_gp* g, double* ll, double* gr, int nh)
{
    int rc;
    if ((rc = want_ard(g, nh, "cugp_loglik_grad_fetch_ard"))) return rc;
    if ((rc = fetch_eval(g))) return rc;
    copy_grad(g, ll, gr);
    return CUGP_OK;
}

int cugp_loglik_grad_ard(cugp_gp* g, double* ll, double* gr, int nh)
{
    int rc;
    if ((rc = want_ard(g, nh, "cugp_loglik_grad_ard", ll && gr))) return rc;
    if ((rc = cugp_loglik_grad(g, nullptr, nullptr))) return rc;     // (the evaluation itself is shared)
    copy_grad(g, ll, gr);
    return CUGP_OK;
}

int cugp_last_quad_logdet(const cugp_gp* g, double* quad, double* logdet)
{
    if (!g || !g->factor_valid) return fail(CUGP_ERR_INVALID, "no evaluation available");
    if (quad) *quad = g->last_quad;
    if (logdet) *logdet = g->last_logdet;
    return CUGP_OK;
}

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

// where predict_passes left the test inputs, W = Ks L^-T and the means / variances on the device
struct PredBufs { double *xt, *w, *mean, *var; };

// The prediction at nt test points on g's stream: of g alone (bt = {}), or of every expert of g's group by ONE sequence
// of batched launches (bt: the group's table; blockIdx.y = expert).  Xt goes into the scratch `scr` (test inputs, then
// Ks and W of one pass, [expert][cpad][npad] each), then per pass of `chunk` test points k_cross, k_predict_gemm and
// k_predict_finish.  rows null: means and variances into the scratch behind W (one pass, chunk >= nt; *pb).  Else
// product-of-experts rows: expert i's 1/v at rows[i * rstride + t], m/v at rows[i * rstride + nt + t].
// latent: the same launches with noise_var = 0 in the scalars k_predict_finish takes by value -- the variance of the
// latent function, sf2 - |W_t|^2, computed directly; nothing else reads them.
static int predict_passes(cugp_gp* g, Batch bt, const double* Xt, int nt, int chunk, Scratch& scr, double* rows,
                          size_t rstride, PredBufs* pb = nullptr, bool latent = false)
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
static int predict_grad_passes(cugp_gp* g, Batch bt, int tiles, const double* Xt, int nt, bool with_noise, bool want_var,
                               Scratch& scr, double* rows, size_t row_stride, double** rows_out = nullptr)
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
            const bool timed = (g->prof == 3 || g->prof == 4) && g->kev_used + 2 <= (int)g->kev.size() &&
                               hipEventRecord(g->kev[g->kev_used], s) == hipSuccess;
            launch_targets_alpha(dW, g->dU, dV, g->npad, cpad, s);
            if (timed && hipEventRecord(g->kev[g->kev_used + 1], s) == hipSuccess) {
                g->kev_prev[g->kev_used / 2] = -1;
                g->kev_kind[g->kev_used / 2] = KIND_PREDICT;
                g->kev_flopv[g->kev_used / 2] = gemm_flop;
                g->kev_used += 2;
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
    if (e == hipSuccess) e = hipStreamSynchronize(s);                // the one host wait
    if (e != hipSuccess) { (void)hipStreamSynchronize(s); return fail(CUGP_ERR_DEVICE, "cugp_predict_grad", e); }
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
static int pred_chunk_rows(const cugp_gp* g, int count, int nt)
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
// g's factor handle (cov_f), created on first use for `tiles` tile rows or more: the joint predictive covariance and the
// Schur complement of cugp_append are written into its A and factored there
static int cov_factor_handle(cugp_gp* g, int tiles)
{
    int rc;
    if (!g->cov_f || g->cov_tiles < tiles) {
        HIPCHK(hipStreamSynchronize(g->stream));
        if (g->cov_f) (void)cugp_destroy(g->cov_f);
        g->cov_f = nullptr;
        g->cov_tiles = 0;
        cugp_gp* f = nullptr;
        if ((rc = cugp_create(tiles * TILE, 1, g->device, &f))) return rc;
        // it never builds an inverse, so it launches no barrier grid: it takes no part in the device's budget of them
        g_live[f->device < 64 ? f->device : 63].fetch_sub(1, std::memory_order_relaxed);
        f->counted = false;
        f->overlap = false;
        f->is_factor = true;
        // (created before the two flags were set: a factor handle of TUNE_PRIO_MIN_NT tile rows got a prioritised stream)
        if ((rc = apply_stream_prio(f)) || (rc = ensure_factor_bufs(f))) { cugp_destroy(f); return rc; }
        g->cov_f = f;
        g->cov_tiles = tiles;
        if ((rc = use_device(g))) return rc;
    }
    return CUGP_OK;
}

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
    if (!g->cov_ev) HIPCHK(hipEventCreateWithFlags(&g->cov_ev, hipEventDisableTiming));
    cugp_gp* f = g->cov_f;
    f->n = nt;                                                       // (a smaller problem in the handle's buffers)
    f->nt = tiles;
    f->npad = ntpad;
    const CovShape cs = predict_cov_shape(ntpad, g->n);
    if ((rc = g->cov_scr.grow((size_t)(cs.split - 1) * ntpad * ntpad, g->stream))) return rc;
    {
        TimedLaunch tl(g, g->stream, g->prof >= 3);
        launch_predict_cov(pb.w, g->npad, ntpad, cs, f->dA, g->cov_scr.p, g->stream);
        tl.done(KIND_COV, 2.0 * cs.tiles * (32.0 * cs.wm) * (32.0 * cs.wm) * cs.kend);
    }
    CovFn cf;
    if ((rc = cov_fn(g, g->stream, nullptr, &cf))) return rc;
    launch_predict_cov_finish(pb.xt, nt, g->d, ntpad, cf, with_noise, jitter, f->dA, g->cov_scr.p, cs.split - 1,
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
    if (e == hipSuccess) e = hipStreamSynchronize(g->stream);
    if (e != hipSuccess) { (void)hipStreamSynchronize(g->stream); return fail(CUGP_ERR_DEVICE, "cugp_predict_cov copy", e); }
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
static int sample_tail(cugp_gp* g, cugp_gp* f, const double* dm, int nt, int nsamples, const double* normals, double* samples,
                       const char* call)
{
    int rc;
    const int ntpad = f->npad, nspad = (nsamples + TILE - 1) / TILE * TILE;
    const size_t nz = (size_t)nspad * ntpad;
    if ((rc = g->samp.grow(2 * nz + (size_t)nsamples * nt, g->stream))) return rc;
    double* dZ = g->samp.p;
    double* dF = dZ + nz;
    double* dS = dF + nz;
    // the factor handle's stream goes on behind Sigma (an event, no host wait): C = chol(Sigma), F = Z C^T, + mean
    HIPCHK(hipEventRecord(g->cov_ev, g->stream));
    hipStream_t fs = f->stream;
    HIPCHK(hipStreamWaitEvent(fs, g->cov_ev, 0));
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
    if ((rc = g->cov_scr.grow((size_t)(cs.split - 1) * TILE * TILE, s))) return rc;
    launch_predict_cov(dW, npad, TILE, cs, f->dA, g->cov_scr.p, s);                 // P P^T
    launch_predict_cov_finish(Xb, kk, d, TILE, cf, true, 0.0, f->dA, g->cov_scr.p, cs.split - 1, nullptr, s);   // S
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
    if (g->tg_m > 0) return fail(CUGP_ERR_INVALID, "cugp_append: the handle has targets set (cugp_set_targets): targets have no new rows");
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
    g->tg_valid = false;
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
    cugp_gp* f = g->cov_f;
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
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) { (void)hipStreamSynchronize(s); return fail(CUGP_ERR_DEVICE, "cugp_append", e); }
    g->pev_valid = false;
    (void)read_result_row(g, g->hout, true);
    // a Schur complement that is not positive definite: NaN results, the data stays extended, and the next ordinary
    // evaluation factors all rows afresh
    if (!std::isfinite(g->last_ll)) discard_eval(g);
    return CUGP_OK;
}

// (bcm.cpp: the experts' common padded size carries n, so an expert takes no appended rows for the rest of its life)
int cugp_mark_bcm_expert(cugp_gp* g)
{
    if (!g) return CUGP_ERR_INVALID;
    g->bcm_expert = true;
    int rc;
    if ((rc = use_device(g)) || (rc = fetch_eval(g))) return rc;
    return apply_stream_prio(g);                             // (an expert's streams carry no priority)
}

// ---------------------------------------------------------------- intermediates
int cugp_compute_K_train(cugp_gp* g, double* K)
{
    if (!g || !K) return CUGP_ERR_INVALID;
    if (!g->have_data) return fail(CUGP_ERR_INVALID, "no training data set");
    int rc;
    if ((rc = use_device(g))) return rc;
    if ((rc = fetch_eval(g))) return rc;
    if ((rc = ensure(&g->dA, (size_t)g->npad * g->npad))) return rc;
    g->factor_valid = g->inverse_valid = false;
    TuneScope ts(g);
    CovFn cf;
    if ((rc = cov_fn(g, g->stream, nullptr, &cf))) return rc;
    launch_kbuild(g->dX, g->n, g->d, g->npad, cf, g->dA, true, g->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy2DAsync(K, (size_t)g->n * sizeof(double), g->dA, (size_t)g->npad * sizeof(double),
                            (size_t)g->n * sizeof(double), g->n, hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));
    return CUGP_OK;
}

int cugp_compute_squared_dist(cugp_gp* g, double c, double* S)
{
    if (!g || !S) return CUGP_ERR_INVALID;
    if (!g->have_data) return fail(CUGP_ERR_INVALID, "no training data set");
    int rc;
    if ((rc = refuse_ard(g, "cugp_compute_squared_dist", "cugp_compute_K_train (an ARD handle has no single length scale to divide by)")))
        return rc;
    if ((rc = use_device(g))) return rc;
    if ((rc = fetch_eval(g))) return rc;
    if ((rc = ensure(&g->dA, (size_t)g->npad * g->npad))) return rc;
    g->factor_valid = g->inverse_valid = false;
    launch_sqdist(g->dX, g->n, g->d, g->npad, c, g->dA, g->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy2DAsync(S, (size_t)g->n * sizeof(double), g->dA, (size_t)g->npad * sizeof(double),
                            (size_t)g->n * sizeof(double), g->n, hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));
    return CUGP_OK;
}

int cugp_compute_k_test(cugp_gp* g, const double* Xt, int nt, double* Ks)
{
    if (!g || !Xt || !Ks || nt <= 0) return CUGP_ERR_INVALID;
    if (!g->have_data) return fail(CUGP_ERR_INVALID, "no training data set");
    int rc;
    if ((rc = use_device(g))) return rc;
    const int ntpad = ((nt + TILE - 1) / TILE) * TILE;
    double *dXt = nullptr, *dKs = nullptr;
    HIPCHK(hipMalloc((void**)&dXt, (size_t)nt * g->d * sizeof(double)));
    hipError_t e = hipMalloc((void**)&dKs, (size_t)ntpad * g->npad * sizeof(double));
    if (e == hipSuccess) e = hipMemcpyAsync(dXt, Xt, (size_t)nt * g->d * sizeof(double), hipMemcpyHostToDevice, g->stream);
    if (e == hipSuccess) {
        TuneScope ts(g);
        CovFn cf;
        // (e: HIP errors of this function, reported below; rc: an error cov_fn has already reported -- both pass the frees)
        if ((rc = cov_fn(g, g->stream, nullptr, &cf)) == CUGP_OK) {
            launch_kcross(g->dX, g->n, g->d, g->npad, dXt, nt, ntpad, cf, dKs, g->stream);
            e = hipMemcpy2DAsync(Ks, (size_t)g->n * sizeof(double), dKs, (size_t)g->npad * sizeof(double),
                                 (size_t)g->n * sizeof(double), nt, hipMemcpyDeviceToHost, g->stream);
        }
    }
    if (e == hipSuccess) e = hipStreamSynchronize(g->stream);
    (void)hipFree(dXt);
    if (dKs) (void)hipFree(dKs);
    if (rc) return rc;
    if (e != hipSuccess) return fail(CUGP_ERR_DEVICE, "cugp_compute_k_test", e);
    return CUGP_OK;
}

static int copy_square(cugp_gp* g, const double* dsrc, double* dst)
{
    HIPCHK(hipMemcpy2DAsync(dst, (size_t)g->n * sizeof(double), dsrc, (size_t)g->npad * sizeof(double),
                            (size_t)g->n * sizeof(double), g->n, hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));
    return CUGP_OK;
}

int cugp_get_cholesky(cugp_gp* g, double* L)
{
    if (!g || !L) return CUGP_ERR_INVALID;
    int rc;
    if ((rc = fetch_eval(g))) return rc;
    if (!g->factor_valid) return fail(CUGP_ERR_INVALID, "cugp_get_cholesky: evaluate the likelihood first");
    if ((rc = use_device(g))) return rc;
    if ((rc = copy_square(g, g->dA, L))) return rc;
    for (int i = 0; i < g->n; i++)                       // matrixops.cpp:100-107: strict upper zeroed
        for (int j = i + 1; j < g->n; j++) L[(size_t)i * g->n + j] = 0.0;
    return CUGP_OK;
}

int cugp_get_K_inverse(cugp_gp* g, double* Kinv)
{
    if (!g || !Kinv) return CUGP_ERR_INVALID;
    int rc;
    if ((rc = fetch_eval(g))) return rc;
    if (!g->inverse_valid) return fail(CUGP_ERR_INVALID, "cugp_get_K_inverse: evaluate the gradient first");
    if ((rc = use_device(g))) return rc;
    if ((rc = copy_square(g, g->dKinv, Kinv))) return rc;
    for (int i = 0; i < g->n; i++)
        for (int j = i + 1; j < g->n; j++) Kinv[(size_t)i * g->n + j] = Kinv[(size_t)j * g->n + i];
    return CUGP_OK;
}

int cugp_get_alpha(cugp_gp* g, double* alpha)
{
    if (!g || !alpha) return CUGP_ERR_INVALID;
    int rc;
    if ((rc = fetch_eval(g))) return rc;
    if (!g->inverse_valid) return fail(CUGP_ERR_INVALID, "cugp_get_alpha: evaluate the gradient first");
    if ((rc = use_device(g))) return rc;
    HIPCHK(hipMemcpyAsync(alpha, g->dalpha, (size_t)g->n * sizeof(double), hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));
    return CUGP_OK;
}

// ---------------------------------------------------------------- multi-target regression
// m target vectors over the handle's inputs and hyper-parameters: everything that depends on the targets is N^2 work
// behind ONE factorisation and inverse (the handle's own evaluation, untouched).  Argument errors come first, then "no
// device" (a process without a GPU never looks into the handle), then what only the handle can tell.
namespace {
int tg_invalid(const char* call, const char* what)
{
    char buf[256];
    snprintf(buf, sizeof buf, "%s: %s", call, what);
    return fail(CUGP_ERR_INVALID, buf);
}

int tg_device(const char* call)
{
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) == hipSuccess && cnt > 0) return CUGP_OK;
    char buf[256];
    snprintf(buf, sizeof buf, "%s: no HIP device visible (libcugp has no CPU fallback)", call);
    return fail(CUGP_ERR_NODEVICE, buf);
}

// the checks every evaluating call shares, behind its own argument checks
int tg_ready(const cugp_gp* g, const char* call)
{
    if (const int rc = tg_device(call)) return rc;
    if (g->tg_m <= 0) return tg_invalid(call, "no targets set (cugp_set_targets)");
    return CUGP_OK;
}

// Z, A, the gradient of the summed objective and the final sums for the current (data, hp, targets): the handle's own
// evaluation first (whichever route cugp_loglik_grad takes; nothing of it is touched), then four launches on its stream
// and ONE host wait.
int eval_targets(cugp_gp* g)
{
    int rc;
    if ((rc = cugp_loglik_grad(g, nullptr, nullptr))) return rc;
    if (g->tg_valid && g->inverse_valid) return CUGP_OK;
    if ((rc = use_device(g))) return rc;
    TuneScope ts(g);
    hipStream_t s = g->stream;
    launch_predict_gemm(g->tg_y, g->dT, g->tg_z, g->npad, g->tg_mpad / TILE, g->nt, s);       // Z = Y L^-T
    launch_targets_alpha(g->tg_z, g->dU, g->tg_a, g->npad, g->tg_m, s);                        // A = Z L^-1
    CovFn cf;
    if ((rc = cov_fn(g, s, nullptr, &cf))) return rc;
    launch_trace_targets(g->dX, g->n, g->d, g->npad, cf, g->dKinv, g->tg_a, g->tg_m, g->tg_part, s);
    launch_finalize_targets(g->tg_z, g->npad, g->n, g->d, g->tg_m, g->last_logdet, g->tg_part, cf, g->tg_out, g->tg_hout, s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    g->tg_row.assign(g->tg_hout, g->tg_hout + 1 + g->nh + g->tg_m);
    g->tg_valid = true;
    return CUGP_OK;
}

// f = -sum_t LL_t and its gradient at th (NaN where the evaluation fails)
void targets_objective(void* ctx, const double* th, int nh, double* f, double* gr)
{
    cugp_gp* g = (cugp_gp*)ctx;
    if (set_theta(g, th) == CUGP_OK && eval_targets(g) == CUGP_OK) {
        *f = -1.0 * g->tg_row[0];
        std::copy(g->tg_row.begin() + 1, g->tg_row.begin() + 1 + nh, gr);
    } else {
        *f = NAN;
        std::fill(gr, gr + nh, NAN);
    }
}
}  // namespace

int cugp_set_targets(cugp_gp* g, const double* Y, int m)
{
    const char* call = "cugp_set_targets";
    if (!g || !Y) return tg_invalid(call, "null argument");
    if (m <= 0) return tg_invalid(call, "m must be positive");
    int rc;
    if ((rc = tg_device(call))) return rc;
    if (!g->have_data) return tg_invalid(call, "no training data set (cugp_set_data comes first: it supplies X)");
    if ((rc = use_device(g))) return rc;
    if ((rc = fetch_eval(g))) return rc;
    HIPCHK(hipStreamSynchronize(g->stream));
    g->tg_valid = false;
    const int mpad = (m + TILE - 1) / TILE * TILE;
    const size_t cnt = (size_t)mpad * g->npad, row = (size_t)1 + g->nh + mpad;
    if (mpad != g->tg_mpad) {
        for (double** p : {&g->tg_y, &g->tg_z, &g->tg_a, &g->tg_out}) {
            if (*p) (void)hipFree(*p);
            *p = nullptr;
        }
        if (g->tg_hout) (void)hipHostFree(g->tg_hout);
        g->tg_hout = nullptr;
        g->tg_m = g->tg_mpad = 0;
        if ((rc = ensure(&g->tg_y, cnt)) || (rc = ensure(&g->tg_z, cnt)) || (rc = ensure(&g->tg_a, cnt)) ||
            (rc = ensure(&g->tg_out, row)))
            return rc;
        HIPCHK(hipHostMalloc((void**)&g->tg_hout, row * sizeof(double), hipHostMallocDefault));
        g->tg_mpad = mpad;
    }
    if ((rc = ensure(&g->tg_part, (size_t)g->nblocks_trace * g->nh))) return rc;
    hipStream_t s = g->stream;
    HIPCHK(hipMemsetAsync(g->tg_y, 0, cnt * sizeof(double), s));
    HIPCHK(hipMemsetAsync(g->tg_z, 0, cnt * sizeof(double), s));
    HIPCHK(hipMemsetAsync(g->tg_a, 0, cnt * sizeof(double), s));
    HIPCHK(hipMemcpy2DAsync(g->tg_y, (size_t)g->npad * sizeof(double), Y, (size_t)g->n * sizeof(double),
                            (size_t)g->n * sizeof(double), m, hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    g->tg_m = m;
    return CUGP_OK;
}

int cugp_num_targets(const cugp_gp* g, int* m)
{
    if (!g || !m) return tg_invalid("cugp_num_targets", "null argument");
    *m = g->tg_m;
    return CUGP_OK;
}

int cugp_loglik_grad_targets(cugp_gp* g, double* ll, double* gr, int nh, double* ll_each)
{
    const char* call = "cugp_loglik_grad_targets";
    if (!g) return tg_invalid(call, "null handle");
    if (nh < 3) return tg_invalid(call, "nh is not the handle's (cugp_num_hyper)");
    int rc;
    if ((rc = tg_ready(g, call))) return rc;
    if (nh != g->nh) return tg_invalid(call, "nh is not the handle's (cugp_num_hyper)");
    if ((rc = eval_targets(g))) return rc;
    const double* r = g->tg_row.data();
    if (ll) *ll = r[0];
    if (gr) std::copy(r + 1, r + 1 + nh, gr);
    if (ll_each) std::copy(r + 1 + nh, r + 1 + nh + g->tg_m, ll_each);
    return CUGP_OK;
}

int cugp_get_alpha_targets(cugp_gp* g, double* alpha)
{
    const char* call = "cugp_get_alpha_targets";
    if (!g || !alpha) return tg_invalid(call, "null argument");
    int rc;
    if ((rc = tg_ready(g, call))) return rc;
    if ((rc = eval_targets(g))) return rc;
    HIPCHK(hipMemcpy2DAsync(alpha, (size_t)g->n * sizeof(double), g->tg_a, (size_t)g->npad * sizeof(double),
                            (size_t)g->n * sizeof(double), g->tg_m, hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));
    return CUGP_OK;
}

// Means of every target and (var given) the variance, which no target enters: cugp_predict's own k_cross, k_predict_gemm
// and k_predict_finish launches, unchanged, give it; the means are A Ks^T (launch_targets_mean).  One pass over the nt test
// points, as cugp_predict.
int cugp_predict_targets(cugp_gp* g, const double* Xt, int nt, double* mean, double* var)
{
    const char* call = "cugp_predict_targets";
    if (!g || !Xt || !mean) return tg_invalid(call, "null argument");
    if (nt <= 0) return tg_invalid(call, "nt must be positive");
    int rc;
    if ((rc = tg_ready(g, call))) return rc;
    if ((rc = eval_targets(g))) return rc;                          // (a stale handle is re-evaluated first)
    TuneScope ts(g);
    const int m = g->tg_m, ntpad = (nt + TILE - 1) / TILE * TILE, split = targets_mean_split(g->npad);
    const size_t nxt = (((size_t)nt * g->d + 15) / 16) * 16, nks = (size_t)ntpad * g->npad;
    const size_t np = (size_t)split * ((m + 63) / 64 * 64) * ntpad, nm = (size_t)m * nt;
    hipStream_t s = g->stream;
    if ((rc = g->tg_pred.grow(nxt + 2 * nks + 2 * (size_t)ntpad + np + nm, s))) return rc;
    double* dXt = g->tg_pred.p;
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
    launch_targets_mean(g->tg_a, dKs, dP, g->npad, m, nt, ntpad, dM, s);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(mean, dM, nm * sizeof(double), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && var) e = hipMemcpyAsync(var, dv, (size_t)nt * sizeof(double), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) { (void)hipStreamSynchronize(s); return fail(CUGP_ERR_DEVICE, "cugp_predict_targets", e); }
    return CUGP_OK;
}

// conjugate gradients on the multi-target objective from the current hyper-parameters (cugp_cg_minimize_n over the handle's
// nh entries; trace rows of 1 + nh); the end point stays set, as cugp_cg_solve leaves it
int cugp_cg_solve_targets(cugp_gp* g, int budget, double* trace, int trace_cap, int* nevals)
{
    const char* call = "cugp_cg_solve_targets";
    if (!g) return tg_invalid(call, "null handle");
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
    return (size_t)(LOO_PT_ROWS + 1 + g->npad / 64) * g->npad + (size_t)g->nh * g->nblocks_trace;
}

// the evaluation that leaves K^-1 and alpha (a stale handle: re-evaluated, as predict_device does), then the LOO launches
// and ONE host wait.  The results row is in g->loo_hout ([0] L_LOO, [1 ..] the gradient when wanted); NaN where the
// covariance is not positive definite (the header's convention).
int loo_eval(cugp_gp* g, bool want_grad, const char* call)
{
    int rc;
    if (!g->have_data) return tg_invalid(call, "no training data set (cugp_set_data)");
    if ((rc = cugp_loglik_grad(g, nullptr, nullptr))) return rc;
    if ((rc = use_device(g))) return rc;
    const size_t nn = (size_t)g->npad * g->npad, row = (size_t)1 + g->nh;
    if ((rc = ensure(&g->loo_pt, loo_small_count(g))) || (rc = ensure(&g->loo_out, row))) return rc;
    if (!g->loo_hout) HIPCHK(hipHostMalloc((void**)&g->loo_hout, row * sizeof(double), hipHostMallocDefault));
    if (want_grad && !g->loo_P) {                                    // both or neither: a failure leaves the handle as it was
        if ((rc = ensure(&g->loo_B, nn))) return rc;
        if ((rc = ensure(&g->loo_P, nn))) { (void)hipFree(g->loo_B); g->loo_B = nullptr; return rc; }
    }
    for (size_t i = 0; i < row; i++) g->loo_hout[i] = NAN;
    if (!g->inverse_valid) return CUGP_OK;                           // (NaN evaluation: nothing to read K^-1 from)
    TuneScope ts(g);
    hipStream_t s = g->stream;
    double* pt = g->loo_pt;
    double* b = pt + (size_t)LOO_PT_ROWS * g->npad;
    double* bpart = b + g->npad;
    double* part = bpart + (size_t)(g->npad / 64) * g->npad;
    launch_loo_point(g->dKinv, g->dalpha, g->dy, g->n, g->npad, pt, g->loo_out, g->loo_hout, s);
    if (want_grad) {
        if (const int pe = prepare_kernels())
            return fail(CUGP_ERR_DEVICE, "hipFuncSetAttribute(MaxDynamicSharedMemorySize)", (hipError_t)pe);
        launch_loo_mirror_scale(g->dKinv, pt, g->n, g->npad, g->loo_B, bpart, b, s);
        {
            TimedLaunch tl(g, s, g->prof >= 2 && g->prof <= 4);      // (no stamp slot in k_loo_product: level 5 does not time it)
            launch_loo_product(g->loo_B, g->loo_P, g->npad, s);
            tl.done(KIND_LOO, (double)tri_tiles(g->nt) * 2.0 * TILE * TILE * g->npad);
        }
        CovFn cf;
        if ((rc = cov_fn(g, s, nullptr, &cf))) return rc;
        launch_trace_loo(g->dX, g->n, g->d, g->npad, cf, g->loo_P, g->dalpha, b, part, g->loo_out, g->loo_hout, s);
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) { (void)hipStreamSynchronize(s); return fail(CUGP_ERR_DEVICE, call, e); }
    if (g->prof >= 2) drain_kernel_events(g);
    return CUGP_OK;
}

// f = -L_LOO and its gradient at th (NaN where the evaluation fails)
void loo_objective(void* ctx, const double* th, int nh, double* f, double* gr)
{
    cugp_gp* g = (cugp_gp*)ctx;
    if (set_theta(g, th) == CUGP_OK && loo_eval(g, true, "cugp_cg_solve_loo") == CUGP_OK) {
        *f = -1.0 * g->loo_hout[0];
        std::copy(g->loo_hout + 1, g->loo_hout + 1 + nh, gr);
    } else {
        *f = NAN;
        std::fill(gr, gr + nh, NAN);
    }
}
}  // namespace

int cugp_loo(cugp_gp* g, double* lpl, double* gr, int nh)
{
    const char* call = "cugp_loo";
    if (!g) return tg_invalid(call, "null handle");
    if (!lpl) return tg_invalid(call, "lpl is NULL");
    if (nh < 3) return tg_invalid(call, "nh is not the handle's (cugp_num_hyper)");
    int rc;
    if ((rc = tg_device(call))) return rc;
    if (nh != g->nh) return tg_invalid(call, "nh is not the handle's (cugp_num_hyper)");
    if ((rc = loo_eval(g, gr != nullptr, call))) return rc;
    *lpl = g->loo_hout[0];
    if (gr) std::copy(g->loo_hout + 1, g->loo_hout + 1 + nh, gr);
    return CUGP_OK;
}

int cugp_loo_predict(cugp_gp* g, double* mean, double* var, double* logp)
{
    const char* call = "cugp_loo_predict";
    if (!g) return tg_invalid(call, "null handle");
    if (!mean || !var) return tg_invalid(call, "mean or var is NULL");
    int rc;
    if ((rc = tg_device(call))) return rc;
    if ((rc = loo_eval(g, false, call))) return rc;
    const size_t bytes = (size_t)g->n * sizeof(double);
    if (!g->inverse_valid) {
        std::fill(mean, mean + g->n, NAN);
        std::fill(var, var + g->n, NAN);
        if (logp) std::fill(logp, logp + g->n, NAN);
        return CUGP_OK;
    }
    hipStream_t s = g->stream;
    hipError_t e = hipMemcpyAsync(mean, g->loo_pt, bytes, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(var, g->loo_pt + g->npad, bytes, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && logp) e = hipMemcpyAsync(logp, g->loo_pt + 2 * (size_t)g->npad, bytes, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) { (void)hipStreamSynchronize(s); return fail(CUGP_ERR_DEVICE, call, e); }
    return CUGP_OK;
}

// (minimize.cpp; internal) cugp_cg_minimize_n's loop with the iterates as its record
int cugp_cg_minimize_n_iterates(cugp_objective_n_fn fn, void* ctx, double* theta, int nh, int budget, double* rows,
                                int rows_cap, int* nevals, int* nrows);

// conjugate gradients on -L_LOO from the current hyper-parameters: the loop of cugp_cg_minimize_n over the handle's nh
// entries; the end point stays set, as cugp_cg_solve leaves it.  The trace holds the ITERATES, rows of nh + 1: the start
// and the point each line search ended at -- the objective never rises along it; the row behind the last one written
// (when there is room) carries NaN in every entry, so a caller can count them.  *nevals: evaluations made.
int cugp_cg_solve_loo(cugp_gp* g, int budget, double* trace, int trace_cap, int* nevals)
{
    const char* call = "cugp_cg_solve_loo";
    if (!g) return tg_invalid(call, "null handle");
    if (budget <= 0) return tg_invalid(call, "budget must be positive");
    int rc;
    if ((rc = tg_device(call))) return rc;
    if (!g->have_data) return tg_invalid(call, "no training data set (cugp_set_data)");
    std::vector<double> th(g->theta);
    int nrows = 0;
    if ((rc = cugp_cg_minimize_n_iterates(loo_objective, g, th.data(), g->nh, budget, trace, trace_cap, nevals, &nrows)))
        return rc;
    if (trace && nrows < trace_cap) std::fill(trace + (size_t)nrows * (g->nh + 1), trace + (size_t)(nrows + 1) * (g->nh + 1), NAN);
    return set_theta(g, th.data());
}

// ---------------------------------------------------------------- stand-alone LA
namespace {

// a handle whose A holds a caller matrix (identity padded) instead of a kernel build
int la_handle(int n, const double* K, const double* y, int device, cugp_gp** out)
{
    int rc = cugp_create(n, 1, device, out);
    if (rc) return rc;
    cugp_gp* g = *out;
    if ((rc = ensure_factor_bufs(g)) || (rc = ensure_inverse_bufs(g))) { cugp_destroy(g); return rc; }
    std::vector<double> pad((size_t)g->npad * g->npad, 0.0);
    for (int i = 0; i < g->npad; i++) {
        if (i < n) memcpy(&pad[(size_t)i * g->npad], K + (size_t)i * n, (size_t)n * sizeof(double));
        else pad[(size_t)i * g->npad + i] = 1.0;
    }
    hipError_t e = hipMemcpy(g->dA, pad.data(), pad.size() * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(g->dy, 0, (size_t)g->npad * sizeof(double));
    if (e == hipSuccess && y) e = hipMemcpy(g->dy, y, (size_t)n * sizeof(double), hipMemcpyHostToDevice);
    if (e != hipSuccess) { cugp_destroy(g); return fail(CUGP_ERR_DEVICE, "la upload", e); }
    return CUGP_OK;
}

int la_factor_inverse(cugp_gp* g, bool inverse)
{
    int rc;
    TuneScope ts(g);
    if ((rc = enqueue_potrf(g, inverse))) return rc;
    HIPCHK(hipStreamSynchronize(g->stream));
    if (barrier_expired(g->hout)) return fail(CUGP_ERR_DEVICE, "a stage barrier of k_trtri_block ran out of polls");
    g->factor_valid = true;
    g->inverse_valid = inverse;
    return CUGP_OK;
}

}  // namespace

int cugp_potrf(int n, const double* K, double* L, int device)
{
    if (n <= 0 || !K || !L) return CUGP_ERR_INVALID;
    cugp_gp* g = nullptr;
    int rc = la_handle(n, K, nullptr, device, &g);
    if (rc) return rc;
    if (!(rc = la_factor_inverse(g, false))) rc = cugp_get_cholesky(g, L);
    cugp_destroy(g);
    return rc;
}

int cugp_potri(int n, const double* K, double* Kinv, int device)
{
    if (n <= 0 || !K || !Kinv) return CUGP_ERR_INVALID;
    cugp_gp* g = nullptr;
    int rc = la_handle(n, K, nullptr, device, &g);
    if (rc) return rc;
    if (!(rc = la_factor_inverse(g, true))) rc = cugp_get_K_inverse(g, Kinv);
    cugp_destroy(g);
    return rc;
}

static int la_solve(int n, const double* K, const double* y, double* x, double* quad, double* logdet, int device)
{
    cugp_gp* g = nullptr;
    int rc = la_handle(n, K, y, device, &g);
    if (rc) return rc;
    TuneScope ts(g);
    if (!(rc = enqueue_potrf(g, false)) && !(rc = enqueue_trtri(g))) {
        launch_trmv_lower(g->dT, g->npad, g->npad, g->dy, g->dz, g->stream);
        launch_trmv_upper(g->dU, g->npad, g->npad, g->dz, g->dalpha, g->stream);
        launch_finalize(g->dz, g->npad, g->n, g->dlogdet, g->nt, nullptr, 0, scalars(g), g->dout, g->hout, g->stream);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess && x)
            e = hipMemcpyAsync(x, g->dalpha, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, g->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(g->stream);
        if (e != hipSuccess) rc = fail(CUGP_ERR_DEVICE, "la_solve", e);
        else if (barrier_expired(g->hout)) rc = fail(CUGP_ERR_DEVICE, "a stage barrier of k_trtri_block ran out of polls");
        else {
            if (quad) *quad = g->hout[4];
            if (logdet) *logdet = g->hout[5];
        }
    }
    cugp_destroy(g);
    return rc;
}

int cugp_chol_and_det(int n, const double* K, const double* y, double* quad, double* logdet, int device)
{
    if (n <= 0 || !K || !y || !quad || !logdet) return CUGP_ERR_INVALID;
    return la_solve(n, K, y, nullptr, quad, logdet, device);
}

int cugp_potrs_vec(int n, const double* K, const double* y, double* x, int device)
{
    if (n <= 0 || !K || !y || !x) return CUGP_ERR_INVALID;
    return la_solve(n, K, y, x, nullptr, nullptr, device);
}

// ---------------------------------------------------------------- sparse variational GP regression on inducing points
// include/cugp.h and DESIGN.md section 25.  The M x M side is two ordinary handles: `u` over Z with the noise slot holding
// the jitter (its own evaluation: Lu, Lu^-1, Lu^-T) and `b`, a factor handle whose A receives B = I + P / s2 and goes the
// way cugp_potri's does (LB, LB^-1, LB^-T, B^-1).  The N side streams the data in chunks through u's cross-covariance and
// triangular-product launches on u's stream; the new passes are kernels.h's launch_sparse_* / launch_trace_cross.
// One side of the model: a set of p label vectors over the handle's rows -- the handle's own y (p = 1 from creation on), or
// the targets (cugp_sparse_set_targets) -- with everything that depends on them and the results of
// that side's last evaluation.  Both sides share P and the factor handle b, so evaluating one clears the other's `valid`.
struct SparseSide {
    // The route of three steps: the three small solves (true: launch_trmv_lower / _upper on one vector; false: products on
    // the tile over the rows of a matrix), the rank-p term of the weights (true: yv, bv in k_trace_cross's registers;
    // false: k_sparse_weights_targets into G first) and the mean of a prediction (true: k_sparse_predict_finish's; false:
    // launch_targets_mean).  Everything else is one kernel family that the own y runs with p = 1.  The routes stay apart
    // because each is another summation order -- other bits -- for no shared benefit; the flag is the side's, not p == 1's:
    // one target keeps the matrix route and its bits.
    bool vector = false;
    int p = 0, rows = 0;                            // label vectors (0: none set); rows of each of the five vectors: 1, or p rounded up to 128
    size_t ystride = 0;                             // the row stride of y: n rounded up to 128
    double *y = nullptr, *yy = nullptr;             // [p][ystride], zero padded to the chunks' 128-row tiles, and y_t'y_t
    double *vec = nullptr;                          // q, c', gamma', beta', beta' / s2^2: [rows][mpad] each
    double *part = nullptr;                         // the slabs' shares of q: [p][chunk pad / 128][mpad]
    bool valid = false, pd = false;                 // b, c' hold for (data, Z, theta, labels); ... and both matrices were positive definite
    bool row_grad = false, row_z = false;           // the row holds the gradient; gz holds the gradient in Z
    std::vector<double> row, gz;                    // [F, g (nh), F_t (p)] and gZ [m][d]
    double *dout = nullptr, *hout = nullptr;        // results row, device and pinned
    Scratch pred;
    double* v(int k, int mpad) const { return vec + (size_t)k * rows * mpad; }     // vector k of the five
};

struct cugp_sparse {
    int n = 0, m = 0, d = 0, mpad = 0, device = 0, kernel = KERNEL_SE, nh = 3, chunk_rows = 0;
    bool ard = false;
    double jitter = 1e-6;
    cugp_gp *u = nullptr, *b = nullptr;
    double *dX = nullptr;                           // [n][d]
    bool have_data = false, have_z = false;
    std::vector<double> theta;
    SparseSide own, tg;                             // the handle's own y; the targets (cugp_sparse_set_targets)
    // scratch, created on first use
    double *dS = nullptr, *dW = nullptr, *dG = nullptr;      // one chunk: k(X_c, Z), W_c, G_c^T ([chunk pad][mpad])
    double *dP = nullptr, *dscr = nullptr;                   // P and the Gram launch's partial tiles
    double *dM[4] = {nullptr, nullptr, nullptr, nullptr};    // H, H2, a product, R (mpad^2 each): the gradient's
    double *dpart = nullptr;                                 // trace partials: the rectangle's, then the square's
    // the gradient with respect to Z (cugp_sparse_bound_grad_z): created on its first use
    std::vector<double> z;                                   // Z as set, [m][d] (the host copy cugp_sparse_get_inducing returns)
    double *dzpart = nullptr, *dzacc = nullptr, *dzout = nullptr, *hz = nullptr;   // partial blocks, running sums, result, its pinned copy
};

namespace {
int sp_chunk_max(const cugp_sparse* s)
{
    const int rows = s->chunk_rows > 0 ? s->chunk_rows : SPARSE_CHUNK_DEFAULT;
    return ((s->n < rows ? s->n : rows) + TILE - 1) / TILE * TILE;
}

size_t sp_blocks_uf(const cugp_sparse* s)
{
    size_t nb = 0;
    const int chunks = sparse_shape(s->n, s->mpad, s->chunk_rows, 0).chunks;
    for (int c = 0; c < chunks; c++) nb += (size_t)(sparse_shape(s->n, s->mpad, s->chunk_rows, c).cpad / 64) * (s->mpad / 64);
    return nb;
}

int sp_ensure(cugp_sparse* s, bool want_grad)
{
    int rc;
    const size_t cm = (size_t)sp_chunk_max(s) * s->mpad, mm = (size_t)s->mpad * s->mpad;
    int split = 1;
    const int chunks = sparse_shape(s->n, s->mpad, s->chunk_rows, 0).chunks;
    for (int c = 0; c < chunks; c++) split = std::max(split, sparse_shape(s->n, s->mpad, s->chunk_rows, c).split);
    if ((rc = ensure(&s->dS, cm)) || (rc = ensure(&s->dW, cm)) || (rc = ensure(&s->dP, mm)) ||
        (rc = ensure(&s->dscr, (size_t)split * mm)))
        return rc;
    if (want_grad) {
        if ((rc = ensure(&s->dG, cm))) return rc;
        for (double*& p : s->dM)
            if ((rc = ensure(&p, mm))) return rc;
        const size_t nb = sp_blocks_uf(s) + (size_t)(s->mpad / 64) * (s->mpad / 64);
        if ((rc = ensure(&s->dpart, (size_t)(s->nh - 1) * nb))) return rc;
    }
    return CUGP_OK;
}

// the buffers of the Z gradient, all or none: a failed allocation leaves the handle as it was
int sp_ensure_z(cugp_sparse* s)
{
    if (s->hz) return CUGP_OK;
    const size_t md = (size_t)s->m * s->d;
    int slots = sparse_z_shape(s->mpad, s->mpad, s->d).ranges;                    // the square's pass
    const int chunks = sparse_shape(s->n, s->mpad, s->chunk_rows, 0).chunks;
    for (int c = 0; c < chunks; c++)
        slots = std::max(slots, sparse_z_shape(sparse_shape(s->n, s->mpad, s->chunk_rows, c).cpad, s->mpad, s->d).ranges);
    double *part = nullptr, *acc = nullptr, *out = nullptr, *h = nullptr;
    hipError_t e = hipMalloc((void**)&part, (size_t)slots * md * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&acc, md * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&out, md * sizeof(double));
    if (e == hipSuccess) e = hipHostMalloc((void**)&h, md * sizeof(double), hipHostMallocDefault);
    if (e != hipSuccess) {
        for (double* p : {part, acc, out})
            if (p) (void)hipFree(p);
        return fail(e == hipErrorOutOfMemory ? CUGP_ERR_NOMEM : CUGP_ERR_DEVICE, "the inducing-input gradient's partial blocks", e);
    }
    s->dzpart = part; s->dzacc = acc; s->dzout = out; s->hz = h;
    return CUGP_OK;
}

// S_c = k(X_c, Z) and W_c = S_c Lu^-T of one chunk on u's stream: the launches of a prediction with the chunk as test rows
void sp_chunk_w(cugp_sparse* s, const CovFn& cf, const SparseShape& c)
{
    cugp_gp* u = s->u;
    launch_kcross(u->dX, s->m, s->d, s->mpad, s->dX + (size_t)c.r0 * s->d, c.count, c.cpad, cf, s->dS, u->stream);
    launch_predict_gemm(s->dS, u->dT, s->dW, s->mpad, c.cpad / TILE, u->nt, u->stream);
}

void sp_side_free(SparseSide& r)
{
    for (double** q : {&r.y, &r.yy, &r.vec, &r.part, &r.dout}) {
        if (*q) (void)hipFree(*q);
        *q = nullptr;
    }
    if (r.hout) (void)hipHostFree(r.hout);
    r.hout = nullptr;
    r.p = r.rows = 0;
    r.valid = false;
}

// a side's buffers for p label vectors, all or none: a failed allocation leaves the side without labels
int sp_side_alloc(cugp_sparse* s, SparseSide& r, int p)
{
    sp_side_free(r);
    const int rows = r.vector ? 1 : (p + TILE - 1) / TILE * TILE;
    const size_t ypad = ((size_t)s->n + TILE - 1) / TILE * TILE, nrow = (size_t)1 + s->nh + p;
    int rc = ensure(&r.y, (size_t)p * ypad);
    if (!rc) rc = ensure(&r.yy, (size_t)p);
    if (!rc) rc = ensure(&r.vec, (size_t)5 * rows * s->mpad);
    if (!rc) rc = ensure(&r.part, (size_t)p * (sp_chunk_max(s) / TILE) * s->mpad);
    if (!rc) rc = ensure(&r.dout, nrow);
    if (!rc && hipHostMalloc((void**)&r.hout, nrow * sizeof(double), hipHostMallocDefault) != hipSuccess)
        rc = fail(CUGP_ERR_NOMEM, "cugp_sparse: the pinned results row");
    if (rc) { sp_side_free(r); return rc; }
    r.p = p;
    r.rows = rows;
    r.ystride = ypad;
    return CUGP_OK;
}

// the checks every evaluating call shares, behind its own argument checks and in front of any device work
int sp_ready(const cugp_sparse* s, const SparseSide& r, const char* call)
{
    if (!s->have_data) return tg_invalid(call, "no data set (cugp_sparse_set_data)");
    if (r.p <= 0) return tg_invalid(call, "no targets set (cugp_sparse_set_targets)");
    if (!s->have_z) return tg_invalid(call, "no inducing inputs set (cugp_sparse_set_inducing)");
    return CUGP_OK;
}

// The bound (and its gradient) of one side at the current hyper-parameters: F = sum_t F_t over the side's p label vectors,
// with the F_t behind the gradient's slots.  The results land in that side's row and gz: NaN where Kuu or B is not
// positive definite (the header's convention).  Two host waits beyond the inner evaluation's: in front of B's
// factorisation, which runs on the factor handle's own stream, and at the end.
// One sequence and one kernel family for both sides; a side's `vector` picks the route of the small solves and of the
// weights' rank-p term (SparseSide).
// want_z (with want_grad): the same sequence with the Z pass behind every k_trace_cross, on the weights that launch read
// -- no launch of the sequence changes, so F and the hyper-parameter components keep their bits -- and no further host wait.
int sp_eval(cugp_sparse* s, SparseSide& r, bool want_grad, const char* call, bool want_z = false)
{
    int rc;
    if ((rc = sp_ready(s, r, call))) return rc;
    SparseSide& other = &r == &s->own ? s->tg : s->own;
    if (r.valid && (r.row_grad || !want_grad) && (r.row_z || !want_z)) return CUGP_OK;
    cugp_gp *u = s->u, *b = s->b;
    if (want_z) {
        if ((rc = use_device(u))) return rc;
        if ((rc = sp_ensure_z(s))) return rc;
    }
    const int p = r.p, nrow = 1 + s->nh + p;
    r.valid = r.pd = false;
    other.valid = false;                                               // (b and P are about to be rewritten)
    r.row.assign((size_t)nrow, NAN);
    r.row_grad = want_grad;
    r.row_z = want_z;
    if (want_z) r.gz.assign((size_t)s->m * s->d, NAN);
    std::vector<double> th(s->theta);
    th[s->nh - 1] = 0.5 * std::log(s->jitter);                        // the noise slot of the inner handle: Kuu = k(Z, Z) + eps I
    if ((rc = set_theta(u, th.data()))) return rc;
    if ((rc = cugp_loglik_grad(u, nullptr, nullptr))) return rc;       // Lu, Lu^-1, Lu^-T
    if ((rc = use_device(u))) return rc;
    if ((rc = sp_ensure(s, want_grad))) return rc;
    if (!std::isfinite(u->last_ll)) { r.valid = true; return CUGP_OK; }       // Kuu is not positive definite: NaN results
    if (const int pe = prepare_kernels())
        return fail(CUGP_ERR_DEVICE, "hipFuncSetAttribute(MaxDynamicSharedMemorySize)", (hipError_t)pe);
    hipStream_t st = u->stream;
    const int mp = s->mpad, nl = s->nh - 2;
    const double sf2 = std::exp(s->theta[s->nh - 2] * 2), s2 = std::exp(s->theta[s->nh - 1] * 2);
    double *q = r.v(0, mp), *cp = r.v(1, mp), *gp = r.v(2, mp), *bp = r.v(3, mp), *bsc = r.v(4, mp);
    const int chunks = sparse_shape(s->n, mp, s->chunk_rows, 0).chunks;
    CovFn cf;
    {
        TuneScope ts(u);
        if ((rc = cov_fn(u, st, nullptr, &cf))) return rc;
        for (int c = 0; c < chunks; c++) {
            const SparseShape sh = sparse_shape(s->n, mp, s->chunk_rows, c);
            sp_chunk_w(s, cf, sh);
            launch_sparse_gram(s->dW, mp, sh, s->dP, s->dscr, c == 0, st);
            launch_sparse_wty_targets(s->dW, mp, sh.cpad, r.y + sh.r0, r.ystride, p, r.part, q, c == 0, st);
        }
        launch_sparse_form_b(s->dP, mp, s2, b->dA, st);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(st));
    }
    if ((rc = la_factor_inverse(b, true))) return rc;                  // LB, LB^-1, LB^-T, B^-1 (cugp_potri's route)
    if ((rc = use_device(u))) return rc;
    TuneScope ts(u);
    if (r.vector) launch_trmv_lower(b->dT, mp, mp, q, cp, st);         // c' = LB^-1 q
    else launch_predict_gemm(q, b->dT, cp, mp, r.rows / TILE, b->nt, st);      // C' = Q LB^-T: row t = LB^-1 q_t
    const size_t nb_uf = sp_blocks_uf(s), nb_uu = (size_t)(mp / 64) * (mp / 64);
    double *part_uf = s->dpart, *part_uu = want_grad ? s->dpart + (size_t)(nl + 1) * nb_uf : nullptr;
    if (want_grad) {
        double *H = s->dM[0], *H2 = s->dM[1], *X1 = s->dM[2], *R = s->dM[3];
        if (r.vector) {
            launch_trmv_upper(b->dU, mp, mp, cp, gp, st);              // gamma' = LB^-T c'
            launch_trmv_upper(u->dU, mp, mp, gp, bp, st);              // beta' = Lu^-T gamma'
        } else {
            launch_targets_alpha(cp, b->dU, gp, mp, p, st);            // Gamma' = C' LB^-1: row t = LB^-T c'_t
            launch_targets_alpha(gp, u->dU, bp, mp, p, st);            // Beta' = Gamma' Lu^-1: row t = Lu^-T gamma'_t
        }
        launch_sparse_h_targets(b->dKinv, s->dP, gp, bp, p, s->m, mp, s2, H, H2, bsc, st);
        launch_targets_alpha(H, u->dU, X1, mp, mp, st);                // H Lu^-1
        launch_sparse_transpose(X1, R, mp, 1.0 / s2, st);              // R = Lu^-T H / s2
        launch_targets_alpha(H2, u->dU, X1, mp, mp, st);               // H2 Lu^-1
        launch_sparse_transpose(X1, H, mp, 1.0, st);                   // Lu^-T H2
        launch_targets_alpha(H, u->dU, H2, mp, mp, st);                // 2 G_uu = Lu^-T H2 Lu^-1
        size_t pofs = 0;
        for (int c = 0; c < chunks; c++) {
            const SparseShape sh = sparse_shape(s->n, mp, s->chunk_rows, c);
            if (chunks > 1) sp_chunk_w(s, cf, sh);                     // (one chunk: W is still there)
            launch_sparse_weights(s->dW, R, s->dG, sh.cpad, mp, st);
            if (!r.vector)                                             // (the rank-p part goes into G: the traces get no yv, bv)
                launch_sparse_weights_targets(s->dG, sh.cpad, mp, r.y + sh.r0, r.ystride, bsc, p, sh.count, s->m, st);
            const double *yv = r.vector ? r.y + sh.r0 : nullptr, *bv = r.vector ? bsc : nullptr;
            launch_trace_cross(s->dX + (size_t)sh.r0 * s->d, sh.count, sh.cpad, u->dX, s->m, s->d, mp, cf, s->dG, yv, bv,
                               part_uf, nb_uf, pofs, st);
            if (want_z)
                launch_trace_cross_z(s->dX + (size_t)sh.r0 * s->d, sh.count, sh.cpad, u->dX, s->m, s->d, mp, cf, s->dG, yv, bv,
                                     s->dzpart, s->dzacc, c == 0, false, s->dzout, s->hz, st);
            pofs += (size_t)(sh.cpad / 64) * (mp / 64);
        }
        launch_trace_cross(u->dX, s->m, mp, u->dX, s->m, s->d, mp, cf, H2, nullptr, nullptr, part_uu, nb_uu, 0, st);
        if (want_z) {
            for (size_t i = 0; i < (size_t)s->m * s->d; i++) s->hz[i] = NAN;
            launch_trace_cross_z(u->dX, s->m, mp, u->dX, s->m, s->d, mp, cf, H2, nullptr, nullptr, s->dzpart, s->dzacc, false,
                                 true, s->dzout, s->hz, st);
        }
    }
    for (int i = 0; i < nrow; i++) r.hout[i] = NAN;
    const double* puf = want_grad ? part_uf : nullptr;
    const double ls2 = s->theta[s->nh - 1] * 2;
    const SparseFinalTargets fin{s->dP, b->dKinv, cp, gp, b->dlogdet, r.yy, s->m, mp, b->nt, p, (double)s->n, sf2, s2, ls2};
    launch_sparse_finalize_targets(fin, puf, nb_uf, part_uu, nb_uu, nl, r.dout, r.hout, st);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { (void)hipStreamSynchronize(st); return fail(CUGP_ERR_DEVICE, call, e); }
    r.pd = std::isfinite(r.hout[0]);
    if (r.pd) {                                                        // (B is not positive definite: NaN results)
        r.row[0] = r.hout[0];
        if (want_grad) std::copy(r.hout + 1, r.hout + 1 + s->nh, r.row.begin() + 1);
        std::copy(r.hout + 1 + s->nh, r.hout + nrow, r.row.begin() + 1 + s->nh);      // the F_t
        if (want_z) std::copy(s->hz, s->hz + (size_t)s->m * s->d, r.gz.begin());
    }
    r.valid = true;
    return CUGP_OK;
}

int sp_set_theta(cugp_sparse* s, const double* th)
{
    bool changed = false;
    for (int i = 0; i < s->nh; i++) changed = changed || th[i] != s->theta[i] || std::isnan(th[i]);
    if (!changed) return CUGP_OK;
    s->theta.assign(th, th + s->nh);
    s->own.valid = s->tg.valid = false;
    return CUGP_OK;
}

// [F, g, F_t] of a side's last evaluation to wherever the caller wants them
void sp_copy_row(const SparseSide& r, int nh, double* F, double* g, double* F_each)
{
    *F = r.row[0];
    if (g) std::copy(r.row.begin() + 1, r.row.begin() + 1 + nh, g);
    if (F_each) std::copy(r.row.begin() + 1 + nh, r.row.end(), F_each);
}

bool sp_z_moved(const cugp_sparse* s, const double* zv)                // (a NaN counts as moved)
{
    for (size_t i = 0; i < s->z.size(); i++)
        if (zv[i] != s->z[i]) return true;
    return false;
}

struct SpObjective {                                                    // what the two callbacks below are handed
    cugp_sparse* s;
    SparseSide* side;
    const char* call;
};

// f = -F of the side and its gradient at th (NaN where the evaluation fails)
void sp_objective(void* ctx, const double* th, int nh, double* f, double* gr)
{
    const SpObjective* o = (const SpObjective*)ctx;
    SparseSide& r = *o->side;
    if (sp_set_theta(o->s, th) == CUGP_OK && sp_eval(o->s, r, true, o->call) == CUGP_OK) {
        *f = -1.0 * r.row[0];
        std::copy(r.row.begin() + 1, r.row.begin() + 1 + nh, gr);
    } else {
        *f = NAN;
        std::fill(gr, gr + nh, NAN);
    }
}

// the same at v = [theta, vec Z]; a Z that differs goes to the handle
void sp_objective_z(void* ctx, const double* v, int nv, double* f, double* gr)
{
    const SpObjective* o = (const SpObjective*)ctx;
    cugp_sparse* s = o->s;
    SparseSide& r = *o->side;
    if ((!sp_z_moved(s, v + s->nh) || cugp_sparse_set_inducing(s, v + s->nh) == CUGP_OK) && sp_set_theta(s, v) == CUGP_OK &&
        sp_eval(s, r, true, o->call, true) == CUGP_OK) {
        *f = -1.0 * r.row[0];
        std::copy(r.row.begin() + 1, r.row.begin() + 1 + s->nh, gr);
        std::copy(r.gz.begin(), r.gz.end(), gr + s->nh);
    } else {
        *f = NAN;
        std::fill(gr, gr + nv, NAN);
    }
}

// Conjugate gradients on -F of a side from the current hyper-parameters: cugp_cg_minimize_n's loop over the handle's nh
// entries with the iterates as its record, as cugp_cg_solve_loo keeps it; the end point stays set
int sp_cg_theta(cugp_sparse* s, SpObjective* o, int budget, double* trace, int trace_cap, int* nevals)
{
    int rc, nrows = 0;
    std::vector<double> th(s->theta);
    if ((rc = cugp_cg_minimize_n_iterates(sp_objective, o, th.data(), s->nh, budget, trace, trace_cap, nevals, &nrows))) return rc;
    if (trace && nrows < trace_cap) std::fill(trace + (size_t)nrows * (s->nh + 1), trace + (size_t)(nrows + 1) * (s->nh + 1), NAN);
    return sp_set_theta(s, th.data());
}

// the same loop over the nh + m d variables [theta, vec Z]; the record keeps [theta, f] of the iterates
int sp_cg_theta_z(cugp_sparse* s, SpObjective* o, int budget, double* trace, int trace_cap, int* nevals)
{
    int rc, nrows = 0;
    if ((rc = use_device(s->u)) || (rc = sp_ensure_z(s))) return rc;
    const int nv = s->nh + s->m * s->d, cap = trace ? std::max(trace_cap, 0) : 0;
    std::vector<double> v(s->theta), rows((size_t)cap * (nv + 1), NAN);
    v.insert(v.end(), s->z.begin(), s->z.end());
    if ((rc = cugp_cg_minimize_n_iterates(sp_objective_z, o, v.data(), nv, budget, cap ? rows.data() : nullptr, cap, nevals, &nrows)))
        return rc;
    for (int r = 0; r < nrows; r++) {
        std::copy(rows.begin() + (size_t)r * (nv + 1), rows.begin() + (size_t)r * (nv + 1) + s->nh, trace + (size_t)r * (s->nh + 1));
        trace[(size_t)r * (s->nh + 1) + s->nh] = rows[(size_t)r * (nv + 1) + nv];
    }
    if (trace && nrows < trace_cap) std::fill(trace + (size_t)nrows * (s->nh + 1), trace + (size_t)(nrows + 1) * (s->nh + 1), NAN);
    if (sp_z_moved(s, v.data() + s->nh) && (rc = cugp_sparse_set_inducing(s, v.data() + s->nh))) return rc;
    return sp_set_theta(s, v.data());
}

// the three cg calls: the argument checks, then the driver of the side
int sp_cg(cugp_sparse* s, SparseSide cugp_sparse::*side, bool inducing, const char* call, int budget, double* trace, int trace_cap,
          int* nevals)
{
    if (!s) return tg_invalid(call, "null handle");
    if (budget <= 0) return tg_invalid(call, "budget must be positive");
    if (const int rc = sp_ready(s, s->*side, call)) return rc;
    SpObjective o{s, &(s->*side), call};
    return inducing ? sp_cg_theta_z(s, &o, budget, trace, trace_cap, nevals) : sp_cg_theta(s, &o, budget, trace, trace_cap, nevals);
}
}  // namespace

int cugp_sparse_plan(int n, int m, int chunk_rows, int pass, int out[5])
{
    const char* call = "cugp_sparse_plan";
    if (!out) return tg_invalid(call, "out is NULL");
    if (n < 1 || m < 1 || m > CUGP_SPARSE_MAX_M) return tg_invalid(call, "n < 1, m < 1 or m beyond CUGP_SPARSE_MAX_M");
    if (chunk_rows < 0 || chunk_rows % TILE) return tg_invalid(call, "chunk_rows must be 0 or a multiple of 128");
    const SparseShape c = sparse_shape(n, (m + TILE - 1) / TILE * TILE, chunk_rows, pass < 0 ? 0 : pass);
    if (pass < 0 || pass >= c.chunks) return tg_invalid(call, "pass beyond the last one");
    out[0] = c.r0; out[1] = c.count; out[2] = c.cpad; out[3] = c.split; out[4] = c.kstep;
    return c.chunks;
}

// test rows per prediction pass: whole 128-row tiles whose Ks, Wt and Vt ([rows][mpad] each) stay within 1 GiB, at most 2^20
static int sparse_predict_rows(int mpad)
{
    const int rows = (int)std::min<size_t>(((size_t)1 << 30) / ((size_t)3 * mpad * sizeof(double)) / TILE * TILE, (size_t)1 << 20);
    return rows < TILE ? TILE : rows;
}

int cugp_sparse_predict_plan(int m, int nt, int pass, int out[2])
{
    const char* call = "cugp_sparse_predict_plan";
    if (!out) return tg_invalid(call, "out is NULL");
    if (m < 1 || m > CUGP_SPARSE_MAX_M) return tg_invalid(call, "m < 1 or m beyond CUGP_SPARSE_MAX_M");
    if (nt <= 0) return tg_invalid(call, "nt must be positive");
    const int rows = sparse_predict_rows((m + TILE - 1) / TILE * TILE);
    const int passes = (int)(((long long)nt + rows - 1) / rows);
    if (pass < 0 || pass >= passes) return tg_invalid(call, "pass beyond the last one");
    out[0] = pass * rows;                                               // (< nt: no overflow)
    out[1] = nt - out[0] < rows ? nt - out[0] : rows;
    return passes;
}

int cugp_sparse_create(int n, int m, int d, int device, int kernel, int ard, double jitter, int chunk_rows, cugp_sparse** out)
{
    const char* call = "cugp_sparse_create";
    if (!out) return tg_invalid(call, "out is NULL");
    if (n < 1 || d < 1) return tg_invalid(call, "n and d must be positive");
    if (m < 1) return tg_invalid(call, "m < 1: at least one inducing input");
    if (m > CUGP_SPARSE_MAX_M) return tg_invalid(call, "m beyond CUGP_SPARSE_MAX_M");
    if (kernel < 0 || kernel >= KERNEL_COUNT) return tg_invalid(call, "unknown kernel kind");
    if (chunk_rows < 0 || chunk_rows % TILE) return tg_invalid(call, "chunk_rows must be 0 or a multiple of 128");
    if (!(jitter > 0.0) || !std::isfinite(jitter)) return tg_invalid(call, "jitter must be positive and finite");
    int rc;
    if ((rc = tg_device(call))) return rc;
    cugp_sparse* s = new (std::nothrow) cugp_sparse;
    if (!s) return fail(CUGP_ERR_NOMEM, "host allocation");
    *out = nullptr;
    s->n = n; s->m = m; s->d = d; s->device = device; s->kernel = kernel; s->ard = ard != 0;
    s->nh = s->ard ? d + 2 : 3;
    s->jitter = jitter; s->chunk_rows = chunk_rows;
    s->mpad = (m + TILE - 1) / TILE * TILE;
    s->theta.assign(s->nh, 0.0);
    s->own.vector = true;
    s->own.row.assign((size_t)2 + s->nh, NAN);
    if ((rc = create_handle(m, d, device, 0, s->ard, &s->u, kernel)) || (rc = cugp_create(m, 1, device, &s->b)) ||
        (rc = ensure_factor_bufs(s->b)) || (rc = ensure_inverse_bufs(s->b))) { cugp_sparse_destroy(s); return rc; }
    if ((rc = sp_side_alloc(s, s->own, 1))) { cugp_sparse_destroy(s); return rc; }
    hipError_t e = hipMalloc((void**)&s->dX, (size_t)n * d * sizeof(double));
    if (e == hipSuccess) e = hipMemset(s->b->dy, 0, (size_t)s->b->npad * sizeof(double));
    if (e != hipSuccess) {
        rc = fail(e == hipErrorOutOfMemory ? CUGP_ERR_NOMEM : CUGP_ERR_DEVICE, call, e);
        cugp_sparse_destroy(s);
        return rc;
    }
    *out = s;
    return CUGP_OK;
}

int cugp_sparse_destroy(cugp_sparse* s)
{
    if (!s) return CUGP_OK;
    (void)hipSetDevice(s->device);
    if (s->u && s->u->stream) (void)hipStreamSynchronize(s->u->stream);
    if (s->u) (void)cugp_destroy(s->u);
    if (s->b) (void)cugp_destroy(s->b);
    for (double* p : {s->dX, s->dS, s->dW, s->dG, s->dP, s->dscr, s->dM[0], s->dM[1], s->dM[2], s->dM[3], s->dpart, s->dzpart,
                      s->dzacc, s->dzout})
        if (p) (void)hipFree(p);
    for (SparseSide* r : {&s->own, &s->tg}) {
        sp_side_free(*r);
        r->pred.release();
    }
    if (s->hz) (void)hipHostFree(s->hz);
    delete s;
    return CUGP_OK;
}

int cugp_sparse_dims(const cugp_sparse* s, int* n, int* m, int* d, int* mpad, int* chunk_rows)
{
    if (!s) return tg_invalid("cugp_sparse_dims", "null handle");
    if (n) *n = s->n;
    if (m) *m = s->m;
    if (d) *d = s->d;
    if (mpad) *mpad = s->mpad;
    if (chunk_rows) *chunk_rows = s->chunk_rows > 0 ? s->chunk_rows : SPARSE_CHUNK_DEFAULT;
    return CUGP_OK;
}

int cugp_sparse_num_hyper(const cugp_sparse* s, int* nh)
{
    if (!s || !nh) return tg_invalid("cugp_sparse_num_hyper", "null argument");
    *nh = s->nh;
    return CUGP_OK;
}

int cugp_sparse_set_data(cugp_sparse* s, const double* X, const double* y)
{
    const char* call = "cugp_sparse_set_data";
    if (!s || !X || !y) return tg_invalid(call, "null argument");
    int rc;
    if ((rc = use_device(s->u))) return rc;
    hipStream_t st = s->u->stream;
    SparseSide& r = s->own;
    HIPCHK(hipMemcpyAsync(s->dX, X, (size_t)s->n * s->d * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(r.y, 0, r.ystride * sizeof(double), st));
    HIPCHK(hipMemcpyAsync(r.y, y, (size_t)s->n * sizeof(double), hipMemcpyHostToDevice, st));
    launch_sparse_yy_targets(r.y, r.ystride, s->n, 1, r.yy, st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    s->have_data = true;
    s->own.valid = s->tg.valid = false;
    return CUGP_OK;
}

int cugp_sparse_set_inducing(cugp_sparse* s, const double* Z)
{
    if (!s || !Z) return tg_invalid("cugp_sparse_set_inducing", "null argument");
    const std::vector<double> zero((size_t)s->m, 0.0);                 // (the inner handle's labels are never read by this model)
    if (const int rc = cugp_set_data(s->u, Z, zero.data())) return rc;
    s->z.assign(Z, Z + (size_t)s->m * s->d);
    s->have_z = true;
    s->own.valid = s->tg.valid = false;
    return CUGP_OK;
}

int cugp_sparse_set_loghyper(cugp_sparse* s, const double* hp, int nh)
{
    const char* call = "cugp_sparse_set_loghyper";
    if (!s || !hp) return tg_invalid(call, "null argument");
    if (nh != s->nh) return tg_invalid(call, "nh is not the handle's (cugp_sparse_num_hyper)");
    return sp_set_theta(s, hp);
}

int cugp_sparse_get_loghyper(const cugp_sparse* s, double* hp, int nh)
{
    const char* call = "cugp_sparse_get_loghyper";
    if (!s || !hp) return tg_invalid(call, "null argument");
    if (nh != s->nh) return tg_invalid(call, "nh is not the handle's (cugp_sparse_num_hyper)");
    std::copy(s->theta.begin(), s->theta.end(), hp);
    return CUGP_OK;
}

int cugp_sparse_bound(cugp_sparse* s, double* F)
{
    const char* call = "cugp_sparse_bound";
    if (!s || !F) return tg_invalid(call, "null argument");
    if (const int rc = sp_eval(s, s->own, false, call)) return rc;
    sp_copy_row(s->own, s->nh, F, nullptr, nullptr);
    return CUGP_OK;
}

int cugp_sparse_bound_grad(cugp_sparse* s, double* F, double* g, int nh)
{
    const char* call = "cugp_sparse_bound_grad";
    if (!s || !F || !g) return tg_invalid(call, "null argument");
    if (nh != s->nh) return tg_invalid(call, "nh is not the handle's (cugp_sparse_num_hyper)");
    if (const int rc = sp_eval(s, s->own, true, call)) return rc;
    sp_copy_row(s->own, s->nh, F, g, nullptr);
    return CUGP_OK;
}

namespace {
// The prediction of one side, behind the call's own argument checks.  Per pass of cugp_sparse_predict_plan Ks, Wt and Vt;
// the variance, which no y enters, by k_sparse_predict_finish.  A vector side's mean comes from that launch too; a matrix
// side's means are (C' / s2) Vt^T (launch_targets_mean), each pass's rows copied to their place in the target-major
// result, and its `var` may be NULL (then the launch is left out).
int sp_predict(cugp_sparse* s, SparseSide& r, const char* call, const double* Xt, int nt, int with_noise, double* mean, double* var)
{
    int rc;
    if ((rc = sp_eval(s, r, false, call))) return rc;                  // (answers from the last evaluation's state when it holds)
    const int p = r.p;
    const bool matrix = !r.vector;
    if (!r.pd) {
        std::fill(mean, mean + (size_t)p * nt, NAN);
        if (var) std::fill(var, var + nt, NAN);
        return CUGP_OK;
    }
    cugp_gp *u = s->u, *b = s->b;
    if ((rc = use_device(u))) return rc;
    TuneScope ts(u);
    hipStream_t st = u->stream;
    const int mp = s->mpad, p64 = (p + 63) / 64 * 64;
    int pr[2];                                                         // the passes of cugp_sparse_predict_plan: the first is the largest
    const int passes = cugp_sparse_predict_plan(s->m, nt, 0, pr);
    if (passes < 1) return passes;
    const int cmax = (pr[1] + TILE - 1) / TILE * TILE;
    const size_t nxt = (((size_t)nt * s->d + 15) / 16) * 16, nks = (size_t)cmax * mp;
    // the matrix route's own: C' / s2, launch_targets_mean's partial sums, a pass's means [p][rows]; its dm is one pass's, unread
    const size_t ncs = matrix ? (size_t)p64 * mp : 0, npp = matrix ? (size_t)targets_mean_split(mp) * p64 * cmax : 0;
    const size_t nm = matrix ? (size_t)p * pr[1] : 0, ndm = matrix ? (size_t)cmax : (size_t)nt;
    if ((rc = r.pred.grow(nxt + 3 * nks + ncs + npp + nm + ndm + nt, st))) return rc;
    double *dXt = r.pred.p, *dKs = dXt + nxt, *dWt = dKs + nks, *dVt = dWt + nks, *dCs = dVt + nks, *dPp = dCs + ncs;
    double *dM = dPp + npp, *dm = dM + nm, *dv = dm + ndm;
    HIPCHK(hipMemcpyAsync(dXt, Xt, (size_t)nt * s->d * sizeof(double), hipMemcpyHostToDevice, st));
    CovFn cf;
    if ((rc = cov_fn(u, st, nullptr, &cf))) return rc;
    const double sf2 = std::exp(s->theta[s->nh - 2] * 2), s2 = std::exp(s->theta[s->nh - 1] * 2);
    const double* cp = r.v(1, mp);                                     // c', or C'
    if (matrix) launch_sparse_scale_targets(cp, p, p64, s->m, mp, s2, dCs, st);
    hipError_t e = hipGetLastError();
    for (int ps = 0; ps < passes && e == hipSuccess; ps++) {
        (void)cugp_sparse_predict_plan(s->m, nt, ps, pr);
        const int t0 = pr[0], c = pr[1], cpad = (c + TILE - 1) / TILE * TILE;
        launch_kcross(u->dX, s->m, s->d, mp, dXt + (size_t)t0 * s->d, c, cpad, cf, dKs, st);
        launch_predict_gemm(dKs, u->dT, dWt, mp, cpad / TILE, u->nt, st);      // Wt = Ks Lu^-T
        launch_predict_gemm(dWt, b->dT, dVt, mp, cpad / TILE, b->nt, st);      // Vt = Wt LB^-T
        if (var) launch_sparse_predict_finish(dWt, dVt, cp, mp, c, sf2, s2, with_noise ? s2 : 0.0, matrix ? dm : dm + t0, dv + t0, st);
        if (matrix) launch_targets_mean(dCs, dVt, dPp, mp, p, c, cpad, dM, st);       // [p][c], packed
        e = hipGetLastError();
        if (e == hipSuccess && matrix)                                         // row t of the pass to mean[t * nt + t0 ..]
            e = hipMemcpy2DAsync(mean + t0, (size_t)nt * sizeof(double), dM, (size_t)c * sizeof(double),
                                 (size_t)c * sizeof(double), p, hipMemcpyDeviceToHost, st);
    }
    if (e == hipSuccess && !matrix) e = hipMemcpyAsync(mean, dm, (size_t)nt * sizeof(double), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && var) e = hipMemcpyAsync(var, dv, (size_t)nt * sizeof(double), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { (void)hipStreamSynchronize(st); return fail(CUGP_ERR_DEVICE, call, e); }
    return CUGP_OK;
}
}  // namespace

int cugp_sparse_predict(cugp_sparse* s, const double* Xt, int nt, int with_noise, double* mean, double* var)
{
    const char* call = "cugp_sparse_predict";
    if (!s || !Xt || !mean || !var) return tg_invalid(call, "null argument");
    if (nt <= 0) return tg_invalid(call, "nt must be positive");
    return sp_predict(s, s->own, call, Xt, nt, with_noise, mean, var);
}

// ---- joint covariance, draws and input gradients of the prediction (include/cugp.h)
// The product launch of cugp_sparse_predict_cov at the process's current tuning, and where it refuses: pure arithmetic
int cugp_sparse_predict_cov_plan(int m, int nt, int out[4])
{
    const char* call = "cugp_sparse_predict_cov_plan";
    if (!out) return tg_invalid(call, "out is NULL");
    if (m < 1 || m > CUGP_SPARSE_MAX_M) return tg_invalid(call, "m < 1 or m beyond CUGP_SPARSE_MAX_M");
    if (nt <= 0) return tg_invalid(call, "nt must be positive");
    if (nt > CUGP_SPARSE_MAX_M) return tg_invalid(call, "nt beyond CUGP_SPARSE_MAX_M: the padded nt^2 must fit an int in the factor handle's kernels");
    const int mpad = (m + TILE - 1) / TILE * TILE, ntpad = (nt + TILE - 1) / TILE * TILE;
    if (nt > sparse_predict_rows(mpad))
        return tg_invalid(call, "nt beyond the first pass of cugp_sparse_predict_plan: Wt and Vt must be whole");
    int tn[TUNE_COUNT];                                                // the process defaults: what a handle without keys of its own takes over
    {
        std::lock_guard<std::mutex> lk(g_tune_mu);
        tune_defaults_locked();
        std::copy(g_tune_default, g_tune_default + TUNE_COUNT, tn);
    }
    const int* prev = t_tune;
    t_tune = tn;
    const CovShape cs = predict_cov_shape(ntpad, mpad);
    t_tune = prev;
    out[0] = ntpad; out[1] = 32 * cs.wm; out[2] = cs.split; out[3] = cs.kstep;
    return CUGP_OK;
}

namespace {
// The shared half of cugp_sparse_predict_cov and cugp_sparse_predict_sample, behind their argument checks: the own side's
// state (evaluated first when stale), Ks, Wt and Vt of all nt points in ONE pass, the marginal prediction by
// cugp_sparse_predict's launch (the mean's bits), then into the lower tiles of the factor handle of the inner handle u
//   Sigma = k(Xt,Xt) (+ s2 I) + jitter I - (Wt Wt^T - Vt Vt^T)
// by k_sparse_predict_cov (both products on one set of accumulators, split over k as k_predict_cov's) and
// k_predict_cov_finish as it stands.  The inner handle keeps eps in its noise slot -- an ARD handle's scalars are read from
// the device, where that slot cannot be replaced for one launch --, so the finish is told there is no noise and s2 rides in
// its jitter argument: the same single addition to the diagonal, and nothing of eps reaches Sigma.
// *pd false: Kuu or B is not positive definite (nothing was enqueued; the caller writes NaN).
int sp_predict_cov_device(cugp_sparse* s, const char* call, const double* Xt, int nt, bool with_noise, double jitter,
                          double** dmean, cugp_gp** fout, bool* pd)
{
    int rc;
    if ((rc = sp_eval(s, s->own, false, call))) return rc;
    *pd = s->own.pd;
    if (!*pd) return CUGP_OK;
    cugp_gp *u = s->u, *b = s->b;
    if ((rc = use_device(u))) return rc;
    TuneScope ts(u);
    hipStream_t st = u->stream;
    const int mp = s->mpad, tiles = (nt + TILE - 1) / TILE, ntpad = tiles * TILE;
    if ((rc = cov_factor_handle(u, tiles))) return rc;
    if (!u->cov_ev) HIPCHK(hipEventCreateWithFlags(&u->cov_ev, hipEventDisableTiming));
    cugp_gp* f = u->cov_f;
    f->n = nt;                                                         // (a smaller problem in the handle's buffers)
    f->nt = tiles;
    f->npad = ntpad;
    const size_t nxt = (((size_t)nt * s->d + 15) / 16) * 16, nks = (size_t)ntpad * mp;
    if ((rc = s->own.pred.grow(nxt + 3 * nks + 2 * (size_t)ntpad, st))) return rc;
    double *dXt = s->own.pred.p, *dKs = dXt + nxt, *dWt = dKs + nks, *dVt = dWt + nks, *dm = dVt + nks, *dv = dm + ntpad;
    HIPCHK(hipMemcpyAsync(dXt, Xt, (size_t)nt * s->d * sizeof(double), hipMemcpyHostToDevice, st));
    CovFn cf;
    if ((rc = cov_fn(u, st, nullptr, &cf))) return rc;
    const double sf2 = std::exp(s->theta[s->nh - 2] * 2), s2 = std::exp(s->theta[s->nh - 1] * 2);
    launch_kcross(u->dX, s->m, s->d, mp, dXt, nt, ntpad, cf, dKs, st);
    launch_predict_gemm(dKs, u->dT, dWt, mp, tiles, u->nt, st);        // Wt = Ks Lu^-T
    launch_predict_gemm(dWt, b->dT, dVt, mp, tiles, b->nt, st);        // Vt = Wt LB^-T
    launch_sparse_predict_finish(dWt, dVt, s->own.v(1, mp), mp, nt, sf2, s2, with_noise ? s2 : 0.0, dm, dv, st);
    const CovShape cs = predict_cov_shape(ntpad, mp);
    if ((rc = u->cov_scr.grow((size_t)(cs.split - 1) * ntpad * ntpad, st))) return rc;
    launch_sparse_predict_cov(dWt, dVt, mp, ntpad, cs, f->dA, u->cov_scr.p, st);
    cf.h.noise_var = s2;                                               // (by value; unread: with_noise is off, see above)
    launch_predict_cov_finish(dXt, nt, s->d, ntpad, cf, false, with_noise ? s2 + jitter : jitter, f->dA, u->cov_scr.p,
                              cs.split - 1, f->dtickets, st);
    HIPCHK(hipGetLastError());
    *dmean = dm;
    *fout = f;
    return CUGP_OK;
}

// the refusals the covariance and the draws share, in front of any device work: cugp_sparse_predict_cov_plan's
int sp_cov_refuse(const cugp_sparse* s, const char* call, int nt)
{
    if (nt <= 0) return tg_invalid(call, "nt must be positive");
    if (nt > CUGP_SPARSE_MAX_M) return tg_invalid(call, "nt beyond CUGP_SPARSE_MAX_M (cugp_sparse_predict_cov_plan)");
    if (nt > sparse_predict_rows(s->mpad))
        return tg_invalid(call, "nt beyond the first pass of cugp_sparse_predict_plan (cugp_sparse_predict_cov_plan)");
    return sp_ready(s, s->own, call);
}
}  // namespace

int cugp_sparse_predict_cov(cugp_sparse* s, const double* Xt, int nt, int with_noise, double* mean, double* cov)
{
    const char* call = "cugp_sparse_predict_cov";
    if (!s || !Xt || !cov) return tg_invalid(call, "null argument");
    int rc;
    if ((rc = sp_cov_refuse(s, call, nt))) return rc;
    double* dm = nullptr;
    cugp_gp* f = nullptr;
    bool pd = false;
    hipStream_t st = s->u->stream;
    if ((rc = sp_predict_cov_device(s, call, Xt, nt, with_noise != 0, 0.0, &dm, &f, &pd))) { (void)hipStreamSynchronize(st); return rc; }
    if (!pd) {
        if (mean) std::fill(mean, mean + nt, NAN);
        std::fill(cov, cov + (size_t)nt * nt, NAN);
        return CUGP_OK;
    }
    hipError_t e = hipSuccess;
    if (mean) e = hipMemcpyAsync(mean, dm, (size_t)nt * sizeof(double), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess)
        e = hipMemcpy2DAsync(cov, (size_t)nt * sizeof(double), f->dA, (size_t)f->npad * sizeof(double),
                             (size_t)nt * sizeof(double), nt, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { (void)hipStreamSynchronize(st); return fail(CUGP_ERR_DEVICE, call, e); }
    // lower triangle, mirrored (cugp_predict_cov's result), in 32 x 32 blocks read along their rows: a column walk over the
    // whole matrix lands on a few cache sets where nt is a multiple of 512 (measured: 530 ms of 535 at nt = 4096)
    constexpr int MB = 32;
    for (int i0 = 0; i0 < nt; i0 += MB)
        for (int j0 = i0; j0 < nt; j0 += MB)
            for (int j = j0; j < j0 + MB && j < nt; j++) {
                const double* lo = cov + (size_t)j * nt;
                for (int i = i0; i < i0 + MB && i < j; i++) cov[(size_t)i * nt + j] = lo[i];
            }
    return CUGP_OK;
}

int cugp_sparse_predict_sample(cugp_sparse* s, const double* Xt, int nt, int with_noise, double jitter, int nsamples,
                               const double* normals, double* samples)
{
    const char* call = "cugp_sparse_predict_sample";
    if (!s || !Xt || !normals || !samples) return tg_invalid(call, "null argument");
    if (nsamples <= 0) return tg_invalid(call, "nsamples must be positive");
    if (!std::isfinite(jitter) || !(jitter >= 0.0)) return tg_invalid(call, "jitter must be finite and not negative");
    int rc;
    if ((rc = sp_cov_refuse(s, call, nt))) return rc;
    double* dm = nullptr;
    cugp_gp* f = nullptr;
    bool pd = false;
    if ((rc = sp_predict_cov_device(s, call, Xt, nt, with_noise != 0, jitter, &dm, &f, &pd))) {
        (void)hipStreamSynchronize(s->u->stream);
        return rc;
    }
    if (!pd) {
        std::fill(samples, samples + (size_t)nsamples * nt, NAN);
        return CUGP_OK;
    }
    return sample_tail(s->u, f, dm, nt, nsamples, normals, samples, call);
}

// Mean, variance and their gradients with respect to the test inputs, in cugp_sparse_predict's passes.  Per pass Ks, Wt, Vt
// and the marginal prediction by cugp_sparse_predict's launches, then -- dvar asked for -- T = Vt LB^-1, D = Wt - T
// (k_sparse_predict_diff, into Vt's place: the prediction has read it) and U = D Lu^-1, both products
// launch_targets_alpha's; then k_predict_grad and its finish, the exact model's instantiations, with (X, n, npad) :=
// (Z, m, mpad), a = beta' / s2 for alpha and U for V.  gamma' and beta' are formed here, by the evaluation's own two
// launches, into this call's scratch whether or not the last evaluation was a gradient one: the same kernels on the same
// inputs give the bits bound_grad's hold, and bound_grad's are not written.
int cugp_sparse_predict_grad(cugp_sparse* s, const double* Xt, int nt, int with_noise, double* mean, double* var, double* dmean,
                             double* dvar)
{
    const char* call = "cugp_sparse_predict_grad";
    if (!s || !Xt) return tg_invalid(call, "null argument");
    if (!dmean && !dvar) return tg_invalid(call, "dmean and dvar are both NULL");
    if (nt <= 0) return tg_invalid(call, "nt must be positive");
    int rc;
    if ((rc = sp_eval(s, s->own, false, call))) return rc;
    const size_t nout = (size_t)nt * s->d;
    if (!s->own.pd) {
        if (mean) std::fill(mean, mean + nt, NAN);
        if (var) std::fill(var, var + nt, NAN);
        if (dmean) std::fill(dmean, dmean + nout, NAN);
        if (dvar) std::fill(dvar, dvar + nout, NAN);
        return CUGP_OK;
    }
    cugp_gp *u = s->u, *b = s->b;
    if ((rc = use_device(u))) return rc;
    TuneScope ts(u);
    hipStream_t st = u->stream;
    const int mp = s->mpad, d = s->d;
    const bool want_var = dvar != nullptr;
    int pr[2];
    const int passes = cugp_sparse_predict_plan(s->m, nt, 0, pr);
    if (passes < 1) return passes;
    const int cmax = (pr[1] + TILE - 1) / TILE * TILE;
    const size_t nxt = (((size_t)nt * d + 15) / 16) * 16, nks = (size_t)cmax * mp, pstride = (size_t)pr[1] * d;
    const size_t npart = (size_t)predict_grad_tiles(s->m) * 2 * pstride;
    if ((rc = s->own.pred.grow(nxt + (want_var ? 4 : 3) * nks + npart + 3 * (size_t)mp + 2 * (size_t)nt + 2 * nout, st))) return rc;
    double *dXt = s->own.pred.p, *dKs = dXt + nxt, *dWt = dKs + nks, *dVt = dWt + nks, *dT = dVt + nks;
    double *dP = dT + (want_var ? nks : 0), *dgam = dP + npart, *dbet = dgam + mp, *da = dbet + mp;
    double *dm = da + mp, *dv = dm + nt, *dgm = dv + nt, *dgv = dgm + nout;
    HIPCHK(hipMemcpyAsync(dXt, Xt, (size_t)nt * d * sizeof(double), hipMemcpyHostToDevice, st));
    CovFn cf;
    if ((rc = cov_fn(u, st, nullptr, &cf))) return rc;
    const double sf2 = std::exp(s->theta[s->nh - 2] * 2), s2 = std::exp(s->theta[s->nh - 1] * 2);
    const double* cp = s->own.v(1, mp);                                   // c'
    launch_trmv_upper(b->dU, mp, mp, cp, dgam, st);                    // gamma' = LB^-T c'
    launch_trmv_upper(u->dU, mp, mp, dgam, dbet, st);                  // beta' = Lu^-T gamma'
    hipError_t e = hipGetLastError();
    for (int ps = 0; ps < passes && e == hipSuccess; ps++) {
        (void)cugp_sparse_predict_plan(s->m, nt, ps, pr);
        const int t0 = pr[0], c = pr[1], cpad = (c + TILE - 1) / TILE * TILE;
        const double* xt = dXt + (size_t)t0 * d;
        launch_kcross(u->dX, s->m, d, mp, xt, c, cpad, cf, dKs, st);
        launch_predict_gemm(dKs, u->dT, dWt, mp, cpad / TILE, u->nt, st);      // Wt = Ks Lu^-T
        launch_predict_gemm(dWt, b->dT, dVt, mp, cpad / TILE, b->nt, st);      // Vt = Wt LB^-T
        launch_sparse_predict_finish(dWt, dVt, cp, mp, c, sf2, s2, with_noise ? s2 : 0.0, dm + t0, dv + t0, st);
        if (want_var) launch_targets_alpha(dVt, b->dU, dT, mp, cpad, st);      // T = Vt LB^-1
        if (want_var || ps == 0)                                               // D = Wt - T over Vt; a = beta' / s2 once
            launch_sparse_predict_diff(dWt, dT, want_var ? dVt : nullptr, mp, cpad, dbet, s2, s->m, ps == 0 ? da : nullptr, st);
        if (want_var) launch_targets_alpha(dVt, u->dU, dT, mp, cpad, st);      // U = D Lu^-1
        launch_predict_grad(u->dX, s->m, d, mp, xt, c, cf, dKs, want_var ? dT : nullptr, da, dP, pstride, st);
        launch_predict_grad_finish(dP, pstride, s->m, c, d, cf, dgm + (size_t)t0 * d, want_var ? dgv + (size_t)t0 * d : nullptr, st);
        e = hipGetLastError();
    }
    if (e == hipSuccess && mean) e = hipMemcpyAsync(mean, dm, (size_t)nt * sizeof(double), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && var) e = hipMemcpyAsync(var, dv, (size_t)nt * sizeof(double), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && dmean) e = hipMemcpyAsync(dmean, dgm, nout * sizeof(double), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && dvar) e = hipMemcpyAsync(dvar, dgv, nout * sizeof(double), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { (void)hipStreamSynchronize(st); return fail(CUGP_ERR_DEVICE, call, e); }
    return CUGP_OK;
}

int cugp_sparse_cg_solve(cugp_sparse* s, int budget, double* trace, int trace_cap, int* nevals)
{
    return sp_cg(s, &cugp_sparse::own, false, "cugp_sparse_cg_solve", budget, trace, trace_cap, nevals);
}

// ---- the inducing inputs as variables
int cugp_sparse_get_inducing(const cugp_sparse* s, double* Z)
{
    const char* call = "cugp_sparse_get_inducing";
    if (!s || !Z) return tg_invalid(call, "null argument");
    if (!s->have_z) return tg_invalid(call, "no inducing inputs set (cugp_sparse_set_inducing)");
    std::copy(s->z.begin(), s->z.end(), Z);
    return CUGP_OK;
}

int cugp_sparse_bound_grad_z(cugp_sparse* s, double* F, double* g, int nh, double* gZ)
{
    const char* call = "cugp_sparse_bound_grad_z";
    if (!s || !F || !g || !gZ) return tg_invalid(call, "null argument");
    if (nh != s->nh) return tg_invalid(call, "nh is not the handle's (cugp_sparse_num_hyper)");
    if (const int rc = sp_eval(s, s->own, true, call, true)) return rc;
    sp_copy_row(s->own, s->nh, F, g, nullptr);
    std::copy(s->own.gz.begin(), s->own.gz.end(), gZ);
    return CUGP_OK;
}

int cugp_sparse_cg_solve_z(cugp_sparse* s, int budget, double* trace, int trace_cap, int* nevals)
{
    return sp_cg(s, &cugp_sparse::own, true, "cugp_sparse_cg_solve_z", budget, trace, trace_cap, nevals);
}

// ---- p targets over one set of inducing points (include/cugp.h)
// The calls below are the single-target ones with sp_eval, sp_predict and sp_cg asked for the targets' side; what is
// theirs alone is the targets' data.  Either side's evaluation writes the shared factor handle b and P, so it takes the
// other side's validity.
int cugp_sparse_set_targets(cugp_sparse* s, const double* Y, int p)
{
    const char* call = "cugp_sparse_set_targets";
    if (!s || !Y) return tg_invalid(call, "null argument");
    if (p < 1) return tg_invalid(call, "p must be positive");
    if (!s->have_data) return tg_invalid(call, "no data set (cugp_sparse_set_data comes first: it supplies X)");
    int rc;
    if ((rc = use_device(s->u))) return rc;
    hipStream_t st = s->u->stream;
    HIPCHK(hipStreamSynchronize(st));
    SparseSide& r = s->tg;
    r.valid = false;
    if (p != r.p && (rc = sp_side_alloc(s, r, p))) return rc;          // (all or none: the handle is left without targets)
    HIPCHK(hipMemsetAsync(r.y, 0, (size_t)p * r.ystride * sizeof(double), st));
    HIPCHK(hipMemsetAsync(r.vec, 0, (size_t)5 * r.rows * s->mpad * sizeof(double), st));
    HIPCHK(hipMemcpy2DAsync(r.y, r.ystride * sizeof(double), Y, (size_t)s->n * sizeof(double), (size_t)s->n * sizeof(double), p,
                            hipMemcpyHostToDevice, st));
    launch_sparse_yy_targets(r.y, r.ystride, s->n, p, r.yy, st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    return CUGP_OK;
}

int cugp_sparse_num_targets(const cugp_sparse* s, int* p)
{
    if (!s || !p) return tg_invalid("cugp_sparse_num_targets", "null argument");
    *p = s->tg.p;
    return CUGP_OK;
}

int cugp_sparse_bound_targets(cugp_sparse* s, double* F, double* F_each)
{
    const char* call = "cugp_sparse_bound_targets";
    if (!s || !F) return tg_invalid(call, "null argument");
    if (const int rc = sp_eval(s, s->tg, false, call)) return rc;
    sp_copy_row(s->tg, s->nh, F, nullptr, F_each);
    return CUGP_OK;
}

int cugp_sparse_bound_grad_targets(cugp_sparse* s, double* F, double* g, int nh, double* F_each)
{
    const char* call = "cugp_sparse_bound_grad_targets";
    if (!s || !F || !g) return tg_invalid(call, "null argument");
    if (nh != s->nh) return tg_invalid(call, "nh is not the handle's (cugp_sparse_num_hyper)");
    if (const int rc = sp_eval(s, s->tg, true, call)) return rc;
    sp_copy_row(s->tg, s->nh, F, g, F_each);
    return CUGP_OK;
}

int cugp_sparse_bound_grad_z_targets(cugp_sparse* s, double* F, double* g, int nh, double* gZ, double* F_each)
{
    const char* call = "cugp_sparse_bound_grad_z_targets";
    if (!s || !F || !g || !gZ) return tg_invalid(call, "null argument");
    if (nh != s->nh) return tg_invalid(call, "nh is not the handle's (cugp_sparse_num_hyper)");
    if (const int rc = sp_eval(s, s->tg, true, call, true)) return rc;
    sp_copy_row(s->tg, s->nh, F, g, F_each);
    std::copy(s->tg.gz.begin(), s->tg.gz.end(), gZ);
    return CUGP_OK;
}

// means of every target [p][nt] and (var given) the variance, which no target enters
int cugp_sparse_predict_targets(cugp_sparse* s, const double* Xt, int nt, int with_noise, double* mean, double* var)
{
    const char* call = "cugp_sparse_predict_targets";
    if (!s || !Xt || !mean) return tg_invalid(call, "null argument");
    if (nt <= 0) return tg_invalid(call, "nt must be positive");
    return sp_predict(s, s->tg, call, Xt, nt, with_noise, mean, var);
}

// cugp_sparse_cg_solve (inducing 0) or cugp_sparse_cg_solve_z (otherwise) on -sum_t F_t: the same loop, record and end point
int cugp_sparse_cg_solve_targets(cugp_sparse* s, int budget, int inducing, double* trace, int trace_cap, int* nevals)
{
    return sp_cg(s, &cugp_sparse::tg, inducing != 0, "cugp_sparse_cg_solve_targets", budget, trace, trace_cap, nevals);
}

// ---------------------------------------------------------------- timing
int cugp_set_profiling(cugp_gp* g, int level)
{
    if (!g) return CUGP_ERR_INVALID;
    int rc;
    if ((rc = use_device(g))) return rc;
    if ((rc = fetch_eval(g))) return rc;
    g->prof = level;
    if (level >= 2 && g->kev.empty()) {
        g->kev.resize(MAX_KEV);
        g->kev_kind.assign(MAX_KEV / 2, 0);
        g->kev_prev.assign(MAX_KEV / 2, -1);
        g->kev_flopv.assign(MAX_KEV / 2, 0.0);
        for (auto& e : g->kev) HIPCHK(hipEventCreate(&e));
    }
    if (level >= 5 && !g->dstamps) {
        HIPCHK(hipMalloc((void**)&g->dstamps, (size_t)2 * STAMP_STRIDE * sizeof(unsigned long long)));
        g->hstamps.assign((size_t)2 * STAMP_STRIDE, 0ull);
    }
    return CUGP_OK;
}

int cugp_get_phase_ms(cugp_gp* g, double ms[6])
{
    if (!g || !ms) return CUGP_ERR_INVALID;
    int rc;
    if ((rc = fetch_eval(g))) return rc;
    if (!g->pev_valid) return fail(CUGP_ERR_INVALID, "profiling was off for the last evaluation");
    if ((rc = use_device(g))) return rc;
    for (int i = 0; i < 5; i++) {
        float t = 0;
        HIPCHK(hipEventElapsedTime(&t, g->pev[i], g->pev[i + 1]));
        ms[i] = t;
    }
    float t = 0;
    HIPCHK(hipEventElapsedTime(&t, g->pev[0], g->pev[5]));
    ms[5] = t;
    return CUGP_OK;
}

int cugp_get_kernel_stats_kind(cugp_gp* g, int kind, double* sum_ms, long long* launches, double* flop, int reset)
{
    if (!g || kind < 0 || kind >= KIND_COUNT) return CUGP_ERR_INVALID;
    int rc;
    if ((rc = fetch_eval(g))) return rc;
    if (sum_ms) *sum_ms = g->kst_ms[kind];
    if (launches) *launches = g->kst_launches[kind];
    if (flop) *flop = g->kst_flop[kind];
    if (reset) { g->kst_ms[kind] = 0; g->kst_launches[kind] = 0; g->kst_flop[kind] = 0; g->kst_disp_ms[kind] = 0; }
    return CUGP_OK;
}

// level 5 only: the same launches' durations counted from the END of the launch directly in front of each on its
// stream (the chain of the factorisation's stream: panel solve -> [far update] -> step launch -> ...), which is where
// rocprofv3 --kernel-trace puts the begin of an in-order dispatch behind another; launches without such a
// predecessor count from their first workgroup's start.  Read it BEFORE a resetting cugp_get_kernel_stats_kind.
int cugp_get_kernel_stats_dispatch_ms(cugp_gp* g, int kind, double* sum_ms)
{
    if (!g || !sum_ms || kind < 0 || kind >= KIND_COUNT) return CUGP_ERR_INVALID;
    int rc;
    if ((rc = fetch_eval(g))) return rc;
    *sum_ms = g->kst_disp_ms[kind];
    return CUGP_OK;
}

int cugp_get_kernel_stats(cugp_gp* g, double* sum_ms, long long* launches, double* flop, int reset)
{
    return cugp_get_kernel_stats_kind(g, 0, sum_ms, launches, flop, reset);
}

void* cugp_get_stream(cugp_gp* g) { return g ? (void*)g->stream : nullptr; }

// ---------------------------------------------------------------- optimiser glue
namespace {
// f = -LL and its gradient at th, over the handle's nh entries (NaN where the evaluation fails)
void gp_objective(void* ctx, const double* th, int nh, double* f, double* gr)
{
    cugp_gp* g = (cugp_gp*)ctx;
    double ll = NAN;
    if (set_theta(g, th) == CUGP_OK && cugp_loglik_grad(g, nullptr, nullptr) == CUGP_OK) copy_grad(g, &ll, gr);
    else std::fill(gr, gr + nh, NAN);
    *f = -1.0 * ll;
}
void gp_objective3(void* ctx, const double th[3], double* f, double gr[3]) { gp_objective(ctx, th, 3, f, gr); }

// conjugate gradients from the current hyper-parameters; the end point stays set (covkernel.cpp:646)
int cg_solve(cugp_gp* g, int budget, double* trace, int trace_cap, int* nevals)
{
    std::vector<double> th(g->theta);
    if (const int rc = cugp_cg_minimize_n(gp_objective, g, th.data(), g->nh, budget, trace, trace_cap, nevals)) return rc;
    return set_theta(g, th.data());
}
}  // namespace

int cugp_cg_solve(cugp_gp* g, int budget, double* trace, int trace_cap, int* nevals)
{
    if (!g) return CUGP_ERR_INVALID;
    if (const int rc = refuse_ard(g, "cugp_cg_solve", "cugp_cg_solve_ard")) return rc;
    return cg_solve(g, budget, trace, trace_cap, nevals);
}

namespace {
void gp_value(void* ctx, const double th[3], double* f)
{
    cugp_gp* g = (cugp_gp*)ctx;
    double ll = NAN;
    cugp_set_loghyper(g, th);
    if (cugp_loglik(g, &ll) != CUGP_OK) ll = NAN;
    *f = -1.0 * ll;
}
void gp_gradient(void* ctx, const double th[3], double gr[3])
{
    cugp_gp* g = (cugp_gp*)ctx;
    cugp_set_loghyper(g, th);                   // unchanged point: the factor of the value call stays valid
    if (cugp_grad(g, gr) != CUGP_OK) gr[0] = gr[1] = gr[2] = NAN;
}
}  // namespace

int cugp_cg_solve_ard(cugp_gp* g, int budget, double* trace, int trace_cap, int* nevals)
{
    if (!g) return fail(CUGP_ERR_INVALID, "cugp_cg_solve_ard: null handle");
    if (const int rc = want_ard(g, g->d + 2, "cugp_cg_solve_ard")) return rc;
    return cg_solve(g, budget, trace, trace_cap, nevals);
}

int cugp_cg_solve_sparing(cugp_gp* g, int budget, double* trace, int trace_cap, int* nevals, int* ngrads)
{
    if (!g) return CUGP_ERR_INVALID;
    if (const int rc = refuse_ard(g, "cugp_cg_solve_sparing", "cugp_cg_solve_ard")) return rc;
    double th[3] = {g->theta[0], g->theta[1], g->theta[2]};
    int rc = cugp_cg_minimize_sparing(gp_value, gp_gradient, g, th, budget, trace, trace_cap, nevals, ngrads);
    if (rc) return rc;
    return cugp_set_loghyper(g, th);
}

int cugp_rprop_solve(cugp_gp* g, int iters, double* trace, int trace_cap, int* nevals)
{
    if (!g) return CUGP_ERR_INVALID;
    if (const int rc = refuse_ard(g, "cugp_rprop_solve", "cugp_cg_solve_ard")) return rc;
    double th[3] = {g->theta[0], g->theta[1], g->theta[2]};
    int rc = cugp_rprop_minimize(gp_objective3, g, th, iters, trace, trace_cap, nevals);
    if (rc) return rc;
    return cugp_set_loghyper(g, th);
}

// ---------------------------------------------------------------- test hooks
// Process default of one tuning key.  Thread-safe (a lock); a handle takes the defaults over when it next starts to
// enqueue -- an evaluation already enqueued keeps the shapes it was enqueued with -- except for the keys set for that
// handle alone with cugp_set_handle_tuning.
int cugp_set_tuning(int key, int value)
{
    if (key < 0 || key >= TUNE_COUNT) return CUGP_ERR_INVALID;
    std::lock_guard<std::mutex> lk(g_tune_mu);
    tune_defaults_locked();
    g_tune_default[key] = value;
    return CUGP_OK;
}

// One key for ONE handle (no other handle, and no later cugp_set_tuning, changes it); own = 0 hands the key back to the
// process default.  The handle's owner thread calls it, like every other call on the handle.
int cugp_set_handle_tuning(cugp_gp* g, int key, int value, int own)
{
    if (!g || key < 0 || key >= TUNE_COUNT) return CUGP_ERR_INVALID;
    int rc;
    if ((rc = fetch_eval(g))) return rc;
    g->tune_own[key] = own != 0;
    if (own && g->tune[key] != value) {
        g->tune[key] = value;
        if (key != TUNE_GRAPHS) g->cfg_epoch++;
    }
    if (key != TUNE_STREAM_PRIO && key != TUNE_PRIO_MIN_NT && key != TUNE_PIPE_BLOCK) return CUGP_OK;
    if (!own) sync_tuning(g);
    if ((rc = use_device(g))) return rc;
    return apply_stream_prio(g);
}

// 1: the handle's factorisation stream is at the device's highest priority (kernels.h TUNE_STREAM_PRIO: the rule, or the
// key's explicit bit 0), so its next evaluation runs chain-first; 0: default priority
int cugp_chain_first(const cugp_gp* g, int* on)
{
    if (!g || !on) return fail(CUGP_ERR_INVALID, "cugp_chain_first: null argument");
    *on = g->chain_first ? 1 : 0;
    return CUGP_OK;
}

// Tile rows per hand-over of the inverse to the other streams for a matrix of nt tile rows evaluated alone (what
// TUNE_PIPE_BLOCK < 0 means; pure arithmetic, no device).  From interleaved A/B runs of uniform blocks of 2 ... 8 tiles
// at 32, 47, 64, 79 and 128 tile rows, with and without the factorisation's stream prioritised
// (profiles/r07_sweep_handover_prio.txt; against "about nt / 16", in % of the evaluation, without / with priority):
//   32 tiles: 2 and 4 equal, 5 and more +3 %;  47 tiles: 3, 4 and 6 within the spread, 2 +3 %   -> nt / 16 stays
//   64 tiles: 5 -0.8 / -1.2 %, 8 -0.2 / -1.6 %, 6 +1.5 / -0.2 %  -> 5: the one size that gains either way
//   79 tiles: 8 -2.1 / -2.2 %, 4 to 6 within +-0.5 %;  128 tiles: 8 (= nt / 16), 4 to 6 +0.4 ... +2.3 %  -> at least 8
// So: single tiles up to 8 tile rows (600 and 1000 rows: -9 % and -3 % against 2), about a sixteenth of the matrix with
// at least 2 below 60 tile rows, 5 from 60 to 71, at least 8 from 72 on; never more than 16.  Non-decreasing in nt.
// The band's edges are guesses: nothing between 47 and 64 or between 64 and 79 tile rows was swept, 5 rests on the one
// measured size 64 (its neighbours there: 4 +-0, 6 +1.5 %), 72 is half-way to 79 and 60 is simply close to 64.
int cugp_pipe_block_for(int nt)
{
    if (nt <= 8) return 1;
    int w = (nt + 8) / 16;
    if (w < 2) w = 2;
    if (nt >= 60 && w < 5) w = 5;
    if (nt >= 72 && w < 8) w = 8;
    return w > 16 ? 16 : w;
}

int cugp_get_handle_tuning(cugp_gp* g, int key, int* value)
{
    if (!g || !value || key < 0 || key >= TUNE_COUNT) return CUGP_ERR_INVALID;
    sync_tuning(g);
    *value = g->tune[key];
    return CUGP_OK;
}

int cugp_potrf_plan(int nt, int P, int near, int kb, int out[5])
{
    int v[6];
    const int rc = cugp_potrf_plan_sub(nt, P, near, 1, kb, v);
    if (rc || !out) return rc ? rc : CUGP_ERR_INVALID;
    for (int i = 0; i < 5; i++) out[i] = v[i];
    return CUGP_OK;
}

int cugp_potrf_plan_sub(int nt, int P, int near, int S, int kb, int out[6])
{
    if (!out || nt <= 1 || kb < 0 || kb + 1 >= nt || P < 1 || S < 1) return CUGP_ERR_INVALID;
    const StepPlan sp = plan_step(nt, P, near, kb, S);
    const int v[6] = {sp.wide_k0, sp.wide_kw, sp.wa0, sp.wa1, sp.wcol, sp.ks};
    for (int i = 0; i < 6; i++) out[i] = v[i];
    return CUGP_OK;
}

int cugp_test_gemm_nt(int m, int n, int k, const double* A, const double* B, double* C, int device)
{
    if (m <= 0 || n <= 0 || k <= 0 || m % TILE || n % TILE || k % 16 || !A || !B || !C)
        return fail(CUGP_ERR_INVALID, "cugp_test_gemm_nt: m,n multiples of 128 and k of 16");
    HIPCHK(hipSetDevice(device));
    double *dA = nullptr, *dB = nullptr, *dC = nullptr;
    HIPCHK(hipMalloc((void**)&dA, (size_t)m * k * sizeof(double)));
    HIPCHK(hipMalloc((void**)&dB, (size_t)n * k * sizeof(double)));
    HIPCHK(hipMalloc((void**)&dC, (size_t)m * n * sizeof(double)));
    HIPCHK(hipMemcpy(dA, A, (size_t)m * k * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dB, B, (size_t)n * k * sizeof(double), hipMemcpyHostToDevice));
    launch_test_gemm_nt(dA, dB, dC, m, n, k, nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(C, dC, (size_t)m * n * sizeof(double), hipMemcpyDeviceToHost));
    (void)hipFree(dA); (void)hipFree(dB); (void)hipFree(dC);
    return CUGP_OK;
}

// stand-alone dense-LA timings on a synthetic SPD matrix built on the device (no host traffic in the timed
// region): the like-for-like counterparts of the reference's library probes cuda_src/cholesky_cu_solver.cpp
// (cusolverDnDpotrf), tmi_cu_solver.cpp (cublasDtrsm vs identity = triangular inverse) and
// cublas_matrix_multiply.cpp (cublasDgemm).  op: 0 Cholesky, 1 triangular inverse of the factor,
// 2 K^-1 = L^-T L^-1 from the triangular inverse, 3 the three together.  ms = best of `reps`.
int cugp_bench_la(int op, int n, int device, int reps, double* ms)
{
    return cugp_bench_la_check(op, n, device, reps, ms, nullptr);
}

// the same, and (ops 0 and 3) the log-determinant of the matrix from the factor it timed, so a test can tell
// that the timed launches produced the right factor
int cugp_bench_la_check(int op, int n, int device, int reps, double* ms, double* logdet)
{
    if (!ms || n <= 0 || op < 0 || op > 5 || reps <= 0) return CUGP_ERR_INVALID;
    cugp_gp* g = nullptr;
    const int d = 4;
    int rc = cugp_create(n, d, device, &g);
    if (rc) return rc;
    std::vector<double> X((size_t)n * d), y(n, 0.0);
    unsigned long long st = 88172645463325252ull;                 // xorshift: reproducible inputs
    for (double& v : X) { st ^= st << 13; st ^= st >> 7; st ^= st << 17; v = (double)(st >> 11) / 9007199254740992.0 * 6.0 - 3.0; }
    const double hp[3] = {0.0, 0.0, -1.0};
    if ((rc = cugp_set_data(g, X.data(), y.data())) || (rc = cugp_set_loghyper(g, hp)) ||
        (rc = ensure_factor_bufs(g)) || (rc = ensure_inverse_bufs(g))) { cugp_destroy(g); return rc; }
    hipEvent_t e0, e1;
    hipError_t e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    double best = 1e300;
    TuneScope ts(g);
    // op 5: the sparse model's Gram product on one chunk of SPARSE_CHUNK_DEFAULT rows against n inducing points: W is that
    // many rows of the (full) matrix K, its rows taken round and round; the partial tiles and their fixed-order sum are timed
    const SparseShape gs = sparse_shape(SPARSE_CHUNK_DEFAULT, g->npad, 0, 0);
    double *gw = nullptr, *gscr = nullptr;
    if (op == 5 && e == hipSuccess) e = hipMalloc((void**)&gw, (size_t)gs.cpad * g->npad * sizeof(double));
    if (op == 5 && e == hipSuccess) e = hipMalloc((void**)&gscr, (size_t)gs.split * g->npad * g->npad * sizeof(double));
    for (int r = 0; r < reps + 1 && e == hipSuccess && rc == CUGP_OK; r++) {
        launch_kbuild(g->dX, g->n, g->d, g->npad, CovFn{KERNEL_SE, false, scalars(g), nullptr}, g->dA, op >= 4, g->stream);
        for (int r0 = 0; op == 5 && r == 0 && r0 < gs.cpad && e == hipSuccess; r0 += g->npad)
            e = hipMemcpyAsync(gw + (size_t)r0 * g->npad, g->dA, (size_t)std::min(g->npad, gs.cpad - r0) * g->npad * sizeof(double),
                               hipMemcpyDeviceToDevice, g->stream);
        if (op == 1 || op == 2) rc = enqueue_potrf(g, false);
        if (op == 2 && !rc) rc = enqueue_trtri(g);
        if (rc) break;
        e = hipEventRecord(e0, g->stream);
        if (op == 4) launch_test_gemm_nt(g->dA, g->dA, g->dKinv, g->npad, g->npad, g->npad, g->stream);   // uniform tiles
        if (op == 5) launch_sparse_gram(gw, g->npad, gs, g->dKinv, gscr, true, g->stream);
        if (op == 0) rc = enqueue_potrf(g, false);
        if (op == 1) rc = enqueue_trtri(g);
        if (op == 2) launch_lauum(g->dU, g->dKinv, g->npad, 0, g->nt, g->stream);
        if (op == 3) rc = enqueue_potrf(g, true);                              // as an evaluation runs them
        if (e == hipSuccess) e = hipEventRecord(e1, g->stream);
        if (e == hipSuccess) e = hipEventSynchronize(e1);
        float t = 0;
        if (e == hipSuccess) e = hipEventElapsedTime(&t, e0, e1);
        if (r > 0 && t < best) best = t;                          // first round warms up
        if (e == hipSuccess && barrier_expired(g->hout)) rc = fail(CUGP_ERR_DEVICE, "a stage barrier of k_trtri_block ran out of polls");
    }
    if (logdet && rc == CUGP_OK && e == hipSuccess) {
        *logdet = NAN;
        if (op == 0 || op == 3) {                                     // 2 * sum of the diagonal blocks' shares
            std::vector<double> part(g->nt);
            e = hipMemcpy(part.data(), g->dlogdet, (size_t)g->nt * sizeof(double), hipMemcpyDeviceToHost);
            double acc = 0.0;
            for (double v : part) acc += v;
            *logdet = 2.0 * acc;
        }
    }
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    if (gw) (void)hipFree(gw);
    if (gscr) (void)hipFree(gscr);
    cugp_destroy(g);
    if (rc) return rc;
    if (e != hipSuccess) return fail(CUGP_ERR_DEVICE, "cugp_bench_la", e);
    *ms = best;
    return CUGP_OK;
}

int cugp_mfma_peak_tflops(int device, double* tflops)
{
    if (!tflops) return CUGP_ERR_INVALID;
    HIPCHK(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    const int blocks = prop.multiProcessorCount * 2;      // 8 waves per CU = 2 per SIMD
    const int iters = 20000;
    double* sink = nullptr;
    HIPCHK(hipMalloc((void**)&sink, (size_t)blocks * 256 * sizeof(double)));
    hipEvent_t a, b;
    HIPCHK(hipEventCreate(&a));
    HIPCHK(hipEventCreate(&b));
    launch_mfma_peak(sink, blocks, 2000, nullptr);
    HIPCHK(hipEventRecord(a, nullptr));
    launch_mfma_peak(sink, blocks, iters, nullptr);
    HIPCHK(hipEventRecord(b, nullptr));
    HIPCHK(hipEventSynchronize(b));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, a, b));
    const double flop = (double)blocks * 4 /*waves*/ * iters * 8.0 * 2048.0;
    *tflops = flop / (ms * 1e-3) / 1e12;
    (void)hipEventDestroy(a); (void)hipEventDestroy(b); (void)hipFree(sink);
    return CUGP_OK;
}

// ---------------------------------------------------------------- grouped evaluation (internal, group.h)
struct cugp_group {
    std::vector<cugp_gp*> experts;
    GroupCtx ctx;
    ExpertPtrs* dtab = nullptr;
    bool tab_valid = false;
    hipGraphExec_t gexec[2] = {nullptr, nullptr};
    unsigned gepoch[2] = {0, 0};
    bool pending = false, pending_grad = false;   // an evaluation is enqueued and not yet fetched
    Scratch pred;                   // grouped prediction scratch (predict_passes: test inputs, [expert][ntpad][npad] Ks and W)
};

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

// the experts' device buffers into the group's table (after a buffer was allocated)
static int write_group_table(cugp_group* gr)
{
    cugp_gp* lead = gr->experts[0];
    const int k = (int)gr->experts.size(), nt = lead->nt;
    std::vector<ExpertPtrs> tab(k);
    for (int i = 0; i < k; i++) {
        cugp_gp* e = gr->experts[i];
        tab[i] = ExpertPtrs{e->dA, e->dT, e->dU, e->dKinv, e->d16, e->d64, e->dlogdet, e->dy, e->dz, e->dalpha,
                            e->dw, e->dpart, gr->ctx.dout + (size_t)i * gr->ctx.row, e->dX,
                            gr->ctx.tickets + (size_t)i * ticket_count(nt), e->n};
    }
    HIPCHK(hipStreamSynchronize(lead->stream));           // a captured graph may still be reading the old table
    HIPCHK(hipMemcpy(gr->dtab, tab.data(), tab.size() * sizeof(ExpertPtrs), hipMemcpyHostToDevice));
    gr->tab_valid = true;
    return CUGP_OK;
}

// the experts share launches only at one set of hyper-parameters (a NaN matches none)
static bool same_loghyper(const cugp_group* gr)
{
    const cugp_gp* lead = gr->experts[0];
    for (const cugp_gp* e : gr->experts)
        if (e->theta != lead->theta) return false;
    return true;
}

// Enqueue one evaluation of all experts of the group on the lead expert's stream(s); results stay on the device
// (ctx.dout, [k][8], an ARD group's [k][8 + nh]) and travel to the pinned ctx.hout (ctx.hrows) behind it.
// cugp_group_fetch waits and reads them.  An ARD group reads the lead expert's scalars AND weights (hs_bytes(lead)): the
// copy in front of the launches -- the node at the head of a captured graph -- takes them from the lead's staging area.
int cugp_group_enqueue(cugp_group* gr, int want_grad)
{
    if (!gr) return CUGP_ERR_INVALID;
    cugp_gp* lead = gr->experts[0];
    const int nt = lead->nt;
    int rc;
    if (gr->pending) return fail(CUGP_ERR_BUSY, "cugp_group_enqueue: an evaluation is already in flight");
    TuneScope ts(lead);                                       // the group runs on the lead expert's tuning
    if (nt > lead->tune[TUNE_GROUP_MAX_TILES]) return CUGP_ERR_INVALID;
    // the batched step kernel puts its workgroups on gridDim.y (65535 at most): larger experts go one by one
    if ((long long)nt * (nt + 1) / 2 + 16 > 65535) return CUGP_ERR_INVALID;
    if (!same_loghyper(gr)) return CUGP_ERR_INVALID;
    for (cugp_gp* e : gr->experts)
        if (!e->have_data || e->prof != 0 || pipe_block(e, want_grad != 0) != 0) return CUGP_ERR_INVALID;   // (experts of a BCM have their own overlap off)
    if ((rc = use_device(lead))) return rc;
    for (cugp_gp* e : gr->experts) {
        if ((rc = fetch_eval(e))) return rc;
        const bool had = e->dA && e->dT && e->dU && (!want_grad || e->dKinv);
        if ((rc = ensure_factor_bufs(e))) return rc;
        if (want_grad && (rc = ensure_inverse_bufs(e))) return rc;
        if (!had) gr->tab_valid = false;
    }
    if (const int pe = prepare_kernels())
        return fail(CUGP_ERR_DEVICE, "hipFuncSetAttribute(MaxDynamicSharedMemorySize)", (hipError_t)pe);
    if (!gr->tab_valid && (rc = write_group_table(gr))) return rc;
    for (cugp_gp* e : gr->experts) e->factor_valid = e->inverse_valid = false;
    if (!lead->ard) *lead->hhs = scalars(lead);             // (ARD: staged where theta was set, weights included)
    gr->ctx.overlap = lead->tune[TUNE_GROUP_OVERLAP] != 0;
    {   // one batched k_trtri_block launch holds count x G workgroups: G = the experts' smallest reserved share
        int cap = TRTRI_BLOCK_MAXWG;
        for (cugp_gp* e : gr->experts) { const int sh = barrier_share(e); if (sh < cap) cap = sh; }
        gr->ctx.gcap = gr->ctx.overlap && cap >= 16 ? cap / 2 : cap;
    }
    lead->grp = &gr->ctx;
    // (with the hand-over the sequence spans several streams: enqueued launch by launch, not replayed)
    const bool graph = lead->tune[TUNE_GRAPHS] != 0 && nt <= GRAPH_MAX_TILES && pipe_block(lead, want_grad != 0) == 0 &&
                       panel_width(lead) == 1;
    rc = graph ? replay_eval(lead, gr->gexec, gr->gepoch, want_grad != 0) : record_eval(lead, want_grad != 0, lead->dhs);
    lead->grp = nullptr;
    if (rc) return rc;
    gr->pending = true;
    gr->pending_grad = want_grad != 0;
    return CUGP_OK;
}

int cugp_group_fetch(cugp_group* gr, double* ll, double* g)
{
    if (!gr || !ll) return CUGP_ERR_INVALID;
    if (!gr->pending) return fail(CUGP_ERR_INVALID, "cugp_group_fetch: nothing enqueued");
    cugp_gp* lead = gr->experts[0];
    const int k = (int)gr->experts.size();
    int rc;
    if ((rc = use_device(lead))) return rc;
    HIPCHK(hipStreamSynchronize(lead->stream));
    gr->pending = false;
    bool ok = true;                                           // (every expert's row is read: every status word cleared)
    for (int i = 0; i < k; i++) {
        double* row = gr->ctx.hout + (size_t)i * 8;
        if (gr->ctx.hrows && gr->pending_grad) {              // ARD: the gradient row, with the status word of the 8-row
            double* wide = gr->ctx.hrows + (size_t)i * gr->ctx.row;
            wide[6] = row[6];
            row[6] = 0.0;
            row = wide;
        }
        ok = read_result_row(gr->experts[i], row, gr->pending_grad) && ok;
    }
    if (!ok) {                                                // (see fetch_eval)
        for (cugp_gp* e : gr->experts) discard_eval(e);
        return fail(CUGP_ERR_DEVICE, "a stage barrier of k_trtri_block ran out of polls (the group's evaluation was abandoned)");
    }
    for (int i = 0; i < k; i++) {
        const cugp_gp* e = gr->experts[i];
        ll[i] = e->last_ll;
        if (gr->pending_grad && g)
            for (int j = 0; j < e->nh; j++) g[(size_t)e->nh * i + j] = e->last_g[j];
    }
    return CUGP_OK;
}

int cugp_internal_fail(int code, const char* what) { return fail(code, what); }

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

int cugp_group_eval(cugp_group* gr, int want_grad, double* ll, double* g)
{
    if (!gr || !ll) return CUGP_ERR_INVALID;
    const int rc = cugp_group_enqueue(gr, want_grad);
    return rc ? rc : cugp_group_fetch(gr, ll, g);
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

}  // extern "C"
