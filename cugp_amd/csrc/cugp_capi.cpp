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
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>

#include "handle.h"

using namespace cugp;

static thread_local std::string g_err;

int cugp::fail(int code, const char* what, hipError_t e)
{
    char buf[512];
    if (e != hipSuccess) snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
    else snprintf(buf, sizeof buf, "%s", what);
    g_err = buf;
    return code;
}

// Argument errors come first in every call, then "no device" (a process without a GPU never looks into a handle)
int cugp::invalid_arg(const char* call, const char* what)
{
    char buf[256];
    snprintf(buf, sizeof buf, "%s: %s", call, what);
    return fail(CUGP_ERR_INVALID, buf);
}

int cugp::need_device(const char* call)
{
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) == hipSuccess && cnt > 0) return CUGP_OK;
    char buf[256];
    snprintf(buf, sizeof buf, "%s: no HIP device visible (libcugp has no CPU fallback)", call);
    return fail(CUGP_ERR_NODEVICE, buf);
}

int cugp::sync_or_fail(hipStream_t s, const char* call, hipError_t e)
{
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) { (void)hipStreamSynchronize(s); return fail(CUGP_ERR_DEVICE, call, e); }
    return CUGP_OK;
}

namespace {

constexpr int MAX_KEV = 4096;   // per-launch event pairs kept between resets
static_assert(MAX_KEV / 2 == cugp::STAMP_STRIDE, "one stamp slot per timed launch");
constexpr int GRAPH_MAX_TILES = 24;   // evaluations up to 3072 rows are replayed as captured graphs
constexpr int PROF_STRIDE = 16; // profiling level 2 times every 16th step launch, rotating (an event pair costs ~5 us of device time);
                                // level 3 times EVERY launch of the MFMA kernels (bench.py's profiled pass: averages comparable with rocprofv3's)

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

namespace cugp {

HyperScalars scalars(const cugp_gp* g)
{
    // covkernel.cpp:65-67 -- exp(2*theta) on the host; ARD: no single length scale (ell_sq = 1, not read by its kernels)
    const double* sf = &g->theta[g->nh - 2];
    return HyperScalars{g->ard ? 1.0 : std::exp(g->theta[0] * 2), std::exp(sf[0] * 2), std::exp(sf[1] * 2)};
}

// (behind the d weights: the family's shape parameters as the kernels read them -- RQ: alpha and 0.5 / alpha)
static size_t hs_bytes(const cugp_gp* g)
{
    return sizeof(HyperScalars) + (g->ard ? (size_t)(g->d + 2 * shape_count(g->kernel)) * sizeof(double) : 0);
}

// ARD: the pinned staging area always holds the current theta's scalars and weights (written where theta is set, with
// the handle's stream idle), so every user of the ARD kernels only has to enqueue the copy in front of its launches
static void stage_ard(cugp_gp* g)
{
    *g->hhs = scalars(g);
    double* w = (double*)(g->hhs + 1);
    for (int c = 0; c < g->d; c++) w[c] = std::exp(-g->theta[g->tied ? 0 : c]);
    if (g->kernel == KERNEL_RQ) {
        const double alpha = std::exp(g->theta[g->nh - 3]);
        w[g->d] = alpha;
        w[g->d + 1] = 0.5 / alpha;
    }
}

static int upload_hs(cugp_gp* g, hipStream_t s)
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
    *cf = CovFn{g->kernel, g->ard, scalars(g), hd, g->tied};
    return hd ? upload_hs(g, s) : CUGP_OK;
}

static int refuse_ard(const cugp_gp* g, const char* call, const char* use)
{
    if (!g->ard) return CUGP_OK;
    char buf[256];
    if (g->kernel == KERNEL_RQ) snprintf(buf, sizeof buf, "%s: the handle is rational quadratic (%d hyper-parameters); use %s", call, g->nh, use);
    else snprintf(buf, sizeof buf, "%s: the handle is ARD (d + 2 hyper-parameters); use %s", call, use);
    return fail(CUGP_ERR_INVALID, buf);
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
    const bool stamps = g->prof >= 5 && g->pf.dstamps && g->pf.kev_used > 0;
    if (stamps && hipMemcpy(g->pf.hstamps.data(), g->pf.dstamps, (size_t)2 * STAMP_STRIDE * sizeof(unsigned long long),
                            hipMemcpyDeviceToHost) != hipSuccess) { g->pf.kev_used = 0; return; }
    for (int i = 0; i + 1 < g->pf.kev_used; i += 2) {
        float ms = 0;
        if (stamps) {
            const unsigned long long t0 = g->pf.hstamps[i / 2], t1 = g->pf.hstamps[STAMP_STRIDE + i / 2];
            if (t1 <= t0) continue;                              // (the launch never ran)
            const int kd = g->pf.kev_kind[i / 2];
            g->pf.kst_ms[kd] += (double)(t1 - t0) * 1e-5;           // 100 MHz ticks -> ms
            g->pf.kst_launches[kd] += 1;
            g->pf.kst_flop[kd] += g->pf.kev_flopv[i / 2];
            // dispatch begin .. end as rocprofv3 sees an in-order launch behind another: from the end of the launch in
            // front of it (its workgroups may then still wait for slots held by the other streams' tiles)
            const int pv = g->pf.kev_prev[i / 2];
            const unsigned long long pe = pv >= 0 ? g->pf.hstamps[STAMP_STRIDE + pv] : 0ull;
            g->pf.kst_disp_ms[kd] += (double)(t1 - ((pe > 0 && pe < t1 && pe <= t0) ? pe : t0)) * 1e-5;
            continue;
        }
        if (hipEventElapsedTime(&ms, g->pf.kev[i], g->pf.kev[i + 1]) == hipSuccess) {
            const int kd = g->pf.kev_kind[i / 2];
            g->pf.kst_ms[kd] += ms;
            g->pf.kst_launches[kd] += 1;
            g->pf.kst_flop[kd] += g->pf.kev_flopv[i / 2];
        }
    }
    g->pf.kev_used = 0;
}

static Batch B(const cugp_gp* g) { return g->grp ? g->grp->bt : Batch{}; }

// pinned host buffer the evaluation's results land in: the group's ([expert][8]) or the handle's.  Entries 0..5: LL, the
// three gradients, y'K^-1y, log|K| (k_finalize); entry 6: set by a kernel whose bounded wait ran out (k_trtri_block)
static double* host_out(const cugp_gp* g) { return g->grp ? g->grp->hout : g->hout; }
// ... and the one a gradient evaluation's final sums land in: an ARD group's rows are wider than its status rows
static double* host_grad_out(const cugp_gp* g) { return g->grp && g->grp->hrows ? g->grp->hrows : host_out(g); }

// ---- tuning: process defaults (cugp_set_tuning) under a lock, one copy per handle ----
static std::mutex g_tune_mu;
static int g_tune_default[TUNE_COUNT];
static bool g_tune_default_init = false;

static void tune_defaults_locked()
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

void tune_defaults(int out[TUNE_COUNT])
{
    std::lock_guard<std::mutex> lk(g_tune_mu);
    tune_defaults_locked();
    std::copy(g_tune_default, g_tune_default + TUNE_COUNT, out);
}

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
static std::atomic<int> g_live[64];
static std::atomic<int> g_bar_used[64];
static int barrier_share(cugp_gp* g)
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
static void barrier_release(cugp_gp* g)
{
    if (g->bar_quota > 0) g_bar_used[g->device >= 0 && g->device < 64 ? g->device : 63].fetch_sub(g->bar_quota, std::memory_order_relaxed);
    g->bar_quota = -1;
}
// workgroups ONE barrier launch of this handle may hold; 0: none (launch by launch)
static int barrier_cap(cugp_gp* g)
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
static int pipe_block(const cugp_gp* g, bool with_inverse)
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
static bool want_chain_first(const cugp_gp* g)
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

// is this launch one of the timed ones?  level 2: one in `every`, rotating with `phase`; levels 3 and 4: all
static bool sampled(const cugp_gp* g, int phase, int every) { return g->prof >= 3 || (g->prof == 2 && phase % every == 0); }

// algorithmic flop of the inverse's tile products (multiply + add; a k tile that is triangular counts half).
// border step 1, one chunk: Wt(tj < c1, ti in [ra, ra+rw)) (+)= sum_{k in [max(tj,c0), c1)} U[tj][k] L[ti][k]
static double border1_flop(int rw, int c0, int c1)
{
    double kt = 0;
    for (int tj = 0; tj < c1; tj++) kt += (c1 - (tj > c0 ? tj : c0)) - (tj >= c0 ? 0.5 : 0.0);   // U[tj][tj] is triangular
    return kt * rw * 2.0 * TILE * TILE * TILE;
}
// border step 2: T(ti in [a, a+w), tj < a) = -sum_{k in [a, ti]} T[ti][k] Wt[tj][k]   (T[ti][ti] triangular)
static double border2_flop(int a, int w)
{
    double kt = 0;
    for (int i = 0; i < w; i++) kt += i + 0.5;
    return kt * a * 2.0 * TILE * TILE * TILE;
}
// K^-1 share of inverse rows [a, a+w): Kinv(ti,tj) (+)= sum_{k in [max(ti,a), a+w)} U[ti][k] U[tj][k]^T, tj <= ti < a+w
static double lauum_flop(int a, int w)
{
    double kt = 0;
    for (int ti = 0; ti < a + w; ti++) {
        const double k = (a + w) - (ti > a ? ti : a);
        kt += (ti + 1) * k - (ti >= a ? 0.5 * (ti + 1) : 0.0) - (ti >= a ? 0.5 * k : 0.0);   // triangular k tile; diagonal output tile
    }
    return kt * 2.0 * TILE * TILE * TILE;
}
// one level of recursive doubling over nt tiles, blocks of s: both steps move |A| x |B| tiles with k ranges up to s
static double level_flop(int nt, int s, int step)
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
static int enqueue_block_own_inverse(cugp_gp* g, int a, int wb, hipStream_t o)
{
    const int ld = g->npad;
    const int gcap = barrier_cap(g);                         // this handle's share of the device's barrier workgroups; 0: none
    if (wb <= TRTRI_BLOCK_MAX_TILES && gcap > 0) {
        unsigned* base = g->grp ? g->grp->tickets : g->dtickets;
        TimedLaunch tl(g, o, sampled(g, (a / (wb > 0 ? wb : 1)) + (int)g->pf.eval_seq, 4));
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
            TimedLaunch tl(g, o, sampled(g, a + s + step + (int)g->pf.eval_seq, 16));  // small launches: one in sixteen
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
static int enqueue_inverse_block(cugp_gp* g, int a, int b, bool kinv, hipStream_t x, hipStream_t xs, hipEvent_t own_done,
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
    const bool timed2 = sampled(g, (a / (wb > 0 ? wb : 1)) + (int)g->pf.eval_seq, 4);   // large launches: every fourth block
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
static int enqueue_last_block(cugp_gp* g, int a, int idx)
{
    const int nt = g->nt, ld = g->npad, wb = nt - a;
    hipStream_t m = g->stream;
    int rc0;
    if ((rc0 = enqueue_block_own_inverse(g, a, wb, m))) return rc0;
    const bool timed2 = sampled(g, (a / (wb > 0 ? wb : 1)) + (int)g->pf.eval_seq, 4);
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

static int phase_mark(cugp_gp* g, int i);

// level 5: the slots the timed launches enqueued from here on stamp (the sums of the ones before were drained by the
// fetch that synchronised them): starts to ~0, ends to 0, on the handle's stream in front of those launches
int reset_stamps(cugp_gp* g)
{
    if (g->prof < 5 || !g->pf.dstamps) return CUGP_OK;
    HIPCHK(hipMemsetAsync(g->pf.dstamps, 0xff, (size_t)STAMP_STRIDE * sizeof(unsigned long long), g->stream));
    HIPCHK(hipMemsetAsync(g->pf.dstamps + STAMP_STRIDE, 0, (size_t)STAMP_STRIDE * sizeof(unsigned long long), g->stream));
    return CUGP_OK;
}


// The shares of K^-1 on a stream of their own (beside the next block's bordering) or behind their block's bordering:
// for a group of experts two large launches in flight fill each other's partly empty last rounds (-3...-6 % per
// evaluation at 16x1500, 8x3000, 4x6000); for a single matrix the extra hand-over costs what it gains or more
// (1500: +1.9 %, 6000: +3.3 %, 8192 / 10000: +-0.3 %, 16384: +0.7 %).  TUNE_LAUUM_STREAM: 0 never, 1 groups, 2 always.
static bool kinv_stream(const cugp_gp* g)
{
    const int v = g->tune[TUNE_LAUUM_STREAM];
    return v >= 2 || (v == 1 && g->grp != nullptr);
}

// (the fork event bev[idx] was recorded by the caller, on the factorisation's stream behind the panel solve that made
//  the rows final)
static int fork_inverse_block(cugp_gp* g, int a, int b, int idx, bool before_last)
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

// far boundary of panel p: first tile column NOT in the near window
static int far_boundary(int nt, int P, int near, int p)
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
static StepPlan plan_step(int nt, int P, int near, int kb, int S = 1)
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
static int panel_width(const cugp_gp* g)
{
    int P = g->tune[TUNE_PANEL];
    if (P < 2 || g->nt < g->tune[TUNE_PANEL_MIN_NT] || g->nt < 3 * P) return 1;
    return P > 32 ? 32 : P;
}

// algorithmic flop of a trailing update over the tile columns [ca, cb) of an nt-tile matrix with kw k tiles:
// entries on or below the diagonal only (a diagonal tile counts half), multiply + add
static double trailing_flop(int nt, int ca, int cb, int kw)
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
static int enqueue_continue(cugp_gp* g);

// zeroed_tickets: the arrival counters a launch already in front of this on the stream has zeroed (record_eval: the
// covariance build, launch_kbuild's `tickets` argument) -- it must be the very buffer the step launches count in, or
// the counters are cleared here (a stale counter means a diagonal block factored twice or never).
int enqueue_potrf(cugp_gp* g, bool with_inverse, bool mark, const unsigned* zeroed_tickets)
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
    g->pf.eval_seq++;
    const unsigned* my_tickets = g->grp ? g->grp->tickets : g->dtickets;
    if (zeroed_tickets && zeroed_tickets == my_tickets) {}   // (the covariance build in front of it did that)
    else if (g->grp) HIPCHK(hipMemsetAsync(g->grp->tickets, 0, (size_t)g->grp->bt.count * ticket_count(nt) * sizeof(unsigned), m));
    else HIPCHK(hipMemsetAsync(g->dtickets, 0, (size_t)ticket_count(nt) * sizeof(unsigned), m));
    launch_potf2(g->dA, ld, 0, g->d16, g->d64, g->dlogdet, m, B(g));
    const bool zf = g->zfuse && !with_inverse;              // (LL-only: z = L^-1 y inside the panel-solve and step launches)
    g->pf.last_main = -1;
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
        TimedLaunch tl(g, m, sampled(g, kb + (int)g->pf.eval_seq, PROF_STRIDE), true);
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

static int phase_mark(cugp_gp* g, int i)
{
    if (g->prof >= 1) HIPCHK(hipEventRecord(g->pf.pev[i], g->stream));
    return CUGP_OK;
}

// K build + factorisation (+ inverse quantities, traces when want_grad); results land in dout.
// hd: the kernels read the hyper-scalars from device memory (a copy node refreshes it) -- the captured form.
static int record_eval(cugp_gp* g, bool want_grad, const HyperScalars* hd)
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
static int replay_eval(cugp_gp* g, hipGraphExec_t gexec[2], unsigned gepoch[2], bool want_grad)
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

static int enqueue_eval(cugp_gp* g, bool want_grad)
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
    g->pf.pev_valid = g->prof >= 1;
    return CUGP_OK;
}

// Gradient quantities from a factor that is already valid (a log-likelihood-only evaluation at the same data and
// hyper-parameters came first: Covsum::compute_loglikelihood then compute_gradient_loghyperparam, or the value and
// gradient halves of the evaluation-sparing line search): L^-1, K^-1, alpha, traces -- no rebuild of K, no second
// factorisation.  One stream (the factorisation it could have run beside is over).
static int enqueue_continue(cugp_gp* g)
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
    g->pf.pev_valid = false;
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
        g->tg.valid = false;                                 // (a new inverse: the multi-target results are stale)
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

// ---- the features' state (handle.h): everything a feature allocated, given up; the members are as after creation
static void free_all(std::initializer_list<double**> dev, double** pinned)
{
    for (double** p : dev) {
        if (*p) (void)hipFree(*p);
        *p = nullptr;
    }
    if (*pinned) (void)hipHostFree(*pinned);
    *pinned = nullptr;
}

void Targets::release()
{
    free_all({&y, &z, &a, &part, &out}, &hout);
    pred.release();
    m = mpad = 0;
    valid = false;
}

void Loo::release() { free_all({&pt, &out, &B, &P}, &hout); }

void JointCov::release()
{
    if (f) (void)cugp_destroy(f);
    if (ev) (void)hipEventDestroy(ev);
    f = nullptr;
    ev = nullptr;
    tiles = 0;
    scr.release();
    samp.release();
}

void Profile::release()
{
    if (dstamps) (void)hipFree(dstamps);
    dstamps = nullptr;
    for (hipEvent_t& e : pev) {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
    for (hipEvent_t e : kev) (void)hipEventDestroy(e);
    kev.clear();
}

}  // namespace cugp

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

// Rational quadratic (GPML covRQiso / covRQard; cugp.h): ard = 1 one length scale per dimension (nh = d + 3), ard = 0 one
// for all (nh = 4).  Either runs the ARD route.
int cugp_create_rq(int n, int d, int device, int npad_min, int ard, cugp_gp** out)
{
    if (!out || n <= 0 || d <= 0 || npad_min < 0)
        return fail(CUGP_ERR_INVALID, "cugp_create_rq: null out, or n, d not positive, or npad_min negative");
    if (ard != 0 && ard != 1) return fail(CUGP_ERR_INVALID, "cugp_create_rq: ard must be 0 (one length scale) or 1 (one per dimension)");
    return create_handle(n, d, device, npad_min, true, out, KERNEL_RQ, ard == 0);
}

int cugp::create_handle(int n, int d, int device, int npad_min, bool ard, cugp_gp** out, int kernel, bool tied)
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
    g->tied = ard && tied;
    if (ard) {
        g->nh = (g->tied ? 1 : d) + shape_count(kernel) + 2;
        g->ncol = d + shape_count(kernel) + 2;
        g->theta.assign(g->nh, 0.0); g->last_g.assign(g->nh, NAN);
    }
    const size_t nrow = ard ? (size_t)ARD_ROW_GRAD + g->nh : 8, ncol = g->ncol;
    g->nt = ((n > npad_min ? n : npad_min) + TILE - 1) / TILE;
    g->npad = g->nt * TILE;
    g->nblocks_trace = trace_num_blocks(g->npad);
    *out = nullptr;
    tune_defaults(g->tune);
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
    for (int i = 0; i <= NPHASE && e == hipSuccess; i++) e = hipEventCreate(&g->pf.pev[i]);
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
    g->cov.release();                                     // (destroys the factor handle, which synchronises its own stream first)
    g->tg.release();
    g->loo.release();
    g->pf.release();
    g->app.release();
    double* bufs[] = {g->dX, g->dy, g->dA, g->dT, g->dU, g->dKinv, g->dz, g->dalpha, g->dw, g->d16, g->dlogdet,
                      g->dpart, g->dout, g->d64};
    for (double* p : bufs)
        if (p) (void)hipFree(p);
    if (g->dtickets) (void)hipFree(g->dtickets);
    g->pred.release();
    if (g->hout) (void)hipHostFree(g->hout);
    if (g->hhs) (void)hipHostFree(g->hhs);
    if (g->dhs) (void)hipFree(g->dhs);
    for (hipGraphExec_t x : g->gexec)
        if (x) (void)hipGraphExecDestroy(x);
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
int cugp::set_theta(cugp_gp* g, const double* th)
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
// looked at before that), then an nh-wide handle (ARD, or rational quadratic in either form) and nh == the handle's
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
    if (nh != g->nh) {
        if (g->kernel == KERNEL_RQ) snprintf(buf, sizeof buf, "%s: nh = %d, the rational quadratic handle has %d hyper-parameters", call, nh, g->nh);
        else snprintf(buf, sizeof buf, "%s: nh = %d, the handle has d + 2 = %d hyper-parameters", call, nh, g->nh);
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

// g's factor handle (cov.f), created on first use for `tiles` tile rows or more: the joint predictive covariance and the
// Schur complement of cugp_append are written into its A and factored there
int cugp::cov_factor_handle(cugp_gp* g, int tiles)
{
    int rc;
    if (!g->cov.f || g->cov.tiles < tiles) {
        HIPCHK(hipStreamSynchronize(g->stream));
        if (g->cov.f) (void)cugp_destroy(g->cov.f);
        g->cov.f = nullptr;
        g->cov.tiles = 0;
        cugp_gp* f = nullptr;
        if ((rc = cugp_create(tiles * TILE, 1, g->device, &f))) return rc;
        // it never builds an inverse, so it launches no barrier grid: it takes no part in the device's budget of them
        g_live[f->device < 64 ? f->device : 63].fetch_sub(1, std::memory_order_relaxed);
        f->counted = false;
        f->overlap = false;
        f->is_factor = true;
        // (created before the two flags were set: a factor handle of TUNE_PRIO_MIN_NT tile rows got a prioritised stream)
        if ((rc = apply_stream_prio(f)) || (rc = ensure_factor_bufs(f))) { cugp_destroy(f); return rc; }
        g->cov.f = f;
        g->cov.tiles = tiles;
        if ((rc = use_device(g))) return rc;
    }
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

// ---------------------------------------------------------------- timing
int cugp_set_profiling(cugp_gp* g, int level)
{
    if (!g) return CUGP_ERR_INVALID;
    int rc;
    if ((rc = use_device(g))) return rc;
    if ((rc = fetch_eval(g))) return rc;
    g->prof = level;
    if (level >= 2 && g->pf.kev.empty()) {
        g->pf.kev.resize(MAX_KEV);
        g->pf.kev_kind.assign(MAX_KEV / 2, 0);
        g->pf.kev_prev.assign(MAX_KEV / 2, -1);
        g->pf.kev_flopv.assign(MAX_KEV / 2, 0.0);
        for (auto& e : g->pf.kev) HIPCHK(hipEventCreate(&e));
    }
    if (level >= 5 && !g->pf.dstamps) {
        HIPCHK(hipMalloc((void**)&g->pf.dstamps, (size_t)2 * STAMP_STRIDE * sizeof(unsigned long long)));
        g->pf.hstamps.assign((size_t)2 * STAMP_STRIDE, 0ull);
    }
    return CUGP_OK;
}

int cugp_get_phase_ms(cugp_gp* g, double ms[6])
{
    if (!g || !ms) return CUGP_ERR_INVALID;
    int rc;
    if ((rc = fetch_eval(g))) return rc;
    if (!g->pf.pev_valid) return fail(CUGP_ERR_INVALID, "profiling was off for the last evaluation");
    if ((rc = use_device(g))) return rc;
    for (int i = 0; i < 5; i++) {
        float t = 0;
        HIPCHK(hipEventElapsedTime(&t, g->pf.pev[i], g->pf.pev[i + 1]));
        ms[i] = t;
    }
    float t = 0;
    HIPCHK(hipEventElapsedTime(&t, g->pf.pev[0], g->pf.pev[5]));
    ms[5] = t;
    return CUGP_OK;
}

int cugp_get_kernel_stats_kind(cugp_gp* g, int kind, double* sum_ms, long long* launches, double* flop, int reset)
{
    if (!g || kind < 0 || kind >= KIND_COUNT) return CUGP_ERR_INVALID;
    int rc;
    if ((rc = fetch_eval(g))) return rc;
    if (sum_ms) *sum_ms = g->pf.kst_ms[kind];
    if (launches) *launches = g->pf.kst_launches[kind];
    if (flop) *flop = g->pf.kst_flop[kind];
    if (reset) { g->pf.kst_ms[kind] = 0; g->pf.kst_launches[kind] = 0; g->pf.kst_flop[kind] = 0; g->pf.kst_disp_ms[kind] = 0; }
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
    *sum_ms = g->pf.kst_disp_ms[kind];
    return CUGP_OK;
}

int cugp_get_kernel_stats(cugp_gp* g, double* sum_ms, long long* launches, double* flop, int reset)
{
    return cugp_get_kernel_stats_kind(g, 0, sum_ms, launches, flop, reset);
}

void* cugp_get_stream(cugp_gp* g) { return g ? (void*)g->stream : nullptr; }

// ---------------------------------------------------------------- optimiser glue
void cugp::objective_result(bool ok, double value, const double* grad, int nh, double* f, double* gr)
{
    *f = ok ? -1.0 * value : NAN;
    if (ok) std::copy(grad, grad + nh, gr);
    else std::fill(gr, gr + nh, NAN);
}

// (minimize.cpp; internal) cugp_cg_minimize_n's loop with the iterates as its record
extern "C" int cugp_cg_minimize_n_iterates(cugp_objective_n_fn fn, void* ctx, double* theta, int nh, int budget, double* rows,
                                int rows_cap, int* nevals, int* nrows);

int cugp::cg_iterates(cugp_objective_n_fn fn, void* ctx, double* x, int n, int budget, double* rows, int rows_cap, int* nevals,
                      int* nrows)
{
    int nr = 0;
    if (const int rc = cugp_cg_minimize_n_iterates(fn, ctx, x, n, budget, rows, rows_cap, nevals, &nr)) return rc;
    if (rows && nr < rows_cap) std::fill(rows + (size_t)nr * (n + 1), rows + (size_t)(nr + 1) * (n + 1), NAN);
    if (nrows) *nrows = nr;
    return CUGP_OK;
}

namespace {
// f = -LL and its gradient at th, over the handle's nh entries (NaN where the evaluation fails)
void gp_objective(void* ctx, const double* th, int nh, double* f, double* gr)
{
    cugp_gp* g = (cugp_gp*)ctx;
    const bool ok = set_theta(g, th) == CUGP_OK && cugp_loglik_grad(g, nullptr, nullptr) == CUGP_OK;
    objective_result(ok, g->last_ll, g->last_g.data(), nh, f, gr);
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
    if (const int rc = want_ard(g, g->nh, "cugp_cg_solve_ard")) return rc;
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

// ---------------------------------------------------------------- grouped evaluation (group.h; everything else of a group: group.cpp)
// the experts' device buffers into the group's table (after a buffer was allocated)
int cugp::write_group_table(cugp_group* gr)
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
bool cugp::same_loghyper(const cugp_group* gr)
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

int cugp_group_eval(cugp_group* gr, int want_grad, double* ll, double* g)
{
    if (!gr || !ll) return CUGP_ERR_INVALID;
    const int rc = cugp_group_enqueue(gr, want_grad);
    return rc ? rc : cugp_group_fetch(gr, ll, g);
}
