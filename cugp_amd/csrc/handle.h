// handle.h -- the handle and what more than one translation unit of the C-ABI needs ("source map").  Internal:
// not part of include/cugp.h, and group.h stays the BCM layer's interface.  Only what a second file really calls is
// declared here; every other helper is static or anonymous in its own file.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "../../include/cugp.h"
#include "group.h"
#include "kernels.h"

namespace cugp {

int fail(int code, const char* what, hipError_t e = hipSuccess);     // error text for cugp_last_error; returns `code`

#define HIPCHK(call)                                                        \
    do {                                                                    \
        hipError_t e_ = (call);                                             \
        if (e_ != hipSuccess) return fail(e_ == hipErrorOutOfMemory ? CUGP_ERR_NOMEM : CUGP_ERR_DEVICE, #call, e_); \
    } while (0)

constexpr int NPHASE = 6;
// kinds of timed launches (cugp_get_kernel_stats_kind): the kernels as rocprofv3 names them
enum { KIND_STEP = 0, KIND_WIDE = 1, KIND_BORDER4 = 2, KIND_BORDER2 = 3, KIND_LAUUM4 = 4, KIND_LAUUM2 = 5,
       KIND_LEVEL4 = 6, KIND_LEVEL2 = 7, KIND_BLOCK = 8, KIND_PREDICT = 9, KIND_BUILD = 10, KIND_TRSM = 11, KIND_COV = 12,
       KIND_PGRAD = 13, KIND_LOO = 14, KIND_COUNT = 15 };

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

// ---- the state of the optional features: plain members of the handle, each given up by its release() (cugp_destroy)
// multi-target regression (cugp_set_targets): m further target vectors over the same X and hyper-parameters, all
// target-major [mpad][npad] and zero beyond n and beyond m; mpad = m rounded up to 128 (k_predict_gemm's tiles)
struct Targets {
    int m = 0, mpad = 0;
    double *y = nullptr, *z = nullptr, *a = nullptr;   // Y, Z = Y L^-T, A = Z L^-1 (row t = alpha_t)
    double *part = nullptr;        // trace partials of the multi-target gradient pass (dpart's size)
    double *out = nullptr, *hout = nullptr;   // results row [LL, g (nh), LL_t (m)], device and pinned
    bool valid = false;            // Z, A and row hold for (data, hp, targets) -- read together with inverse_valid
    std::vector<double> row;
    Scratch pred;                  // cugp_predict_targets: test inputs, Ks, W, variance, partial means, means
    void release();
};

// leave-one-out cross-validation (cugp_loo): buffers of its own, created on first use -- no buffer any other call reads is written
struct Loo {
    double *pt = nullptr;          // [LOO_PT_ROWS][npad] per-point results, then b [npad], the tiles' shares of b [npad / 64][npad]
                                   // and the trace partials [nh][nblocks_trace]: one allocation
    double *out = nullptr, *hout = nullptr;   // results row [L_LOO, g (nh)], device and pinned
    double *B = nullptr, *P = nullptr;        // npad^2 each: K^-1 diag(sqrt c) and its product; first gradient call
    void release();
};

// joint predictive covariance (cugp_predict_cov / cugp_predict_sample), all created on first use
struct JointCov {
    cugp_gp* f = nullptr;          // factor handle: its A receives Sigma (ld = its npad), its own stream factors it
    int tiles = 0;                 // ... tile rows it was created for (it serves any smaller count)
    hipEvent_t ev = nullptr;       // "Sigma written" (this handle's stream -> f's)
    Scratch scr;                   // split-k partial products of k_predict_cov
    Scratch samp;                  // draws: normals Z, F = Z C^T (both [ns pad][ntpad]), packed samples
    void release();
};

// profiling (cugp_set_profiling; the level itself is the handle's `prof`)
struct Profile {
    hipEvent_t pev[NPHASE + 1] = {};
    bool pev_valid = false;
    std::vector<hipEvent_t> kev;   // start/stop pairs around MFMA launches (profiling level 2)
    std::vector<int> kev_kind;     // per pair: KIND_* above
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
    void release();
};

}  // namespace cugp

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
    double* hout = nullptr;        // pinned, 8 doubles (ARD: 8 + nh)
    int nblocks_trace = 0;
    // the nh log hyper-parameters and the gradient of the last evaluation: {log l, log sigma_f, log sigma_n}, or on an ARD
    // handle (cugp_create_ard; for life) [log l_1 .. log l_d, log sigma_f, log sigma_n].  hhs / dhs then hold the
    // hyper-scalars FOLLOWED by the d weights exp(-theta_c); result rows are 8 + nh doubles (kernels.h: ARD_ROW_GRAD)
    // A rational quadratic handle (cugp_create_rq, kernel == KERNEL_RQ) runs the ARD route whichever form it has: ard is
    // true, theta is [log l_1 .. log l_d | log l (tied), log alpha, log sigma_f, log sigma_n], and alpha with 0.5 / alpha
    // follow the d weights in hhs / dhs.  tied: one length scale, written into all d weights (nh = 4); the gradient
    // partials keep their d + 1 + 2 columns (ncol), only the final sums add the length columns up.
    bool ard = false;
    bool tied = false;
    int nh = 3;
    int ncol = 3;                  // columns of the trace partials: 3, ARD d + shape_count(kernel) + 2
    std::vector<double> theta = {0, 0, 0}, last_g = {NAN, NAN, NAN};
    // covariance family (cugp.h CUGP_KERNEL_*, kernels.h KERNEL_*), for life, ARD handles included.  Read wherever one of
    // the four passes that evaluate the kernel function is launched; nothing else depends on it.
    int kernel = cugp::KERNEL_SE;
    bool have_data = false;
    bool factor_valid = false;     // A holds L for (data, hp)
    bool inverse_valid = false;    // T, U, Kinv, alpha hold the inverse quantities for (data, hp)
    bool pending = false, pending_grad = false;
    bool zfuse = false;            // record_eval, LL-only: the forward substitution L z = y rides in the factorisation's launches
    bool vec_early = false;        // record_eval: z = L^-1 y, alpha = L^-T z go behind the last block's bordering
    bool vec_done = false;         // ... and were enqueued there
    const cugp::GroupCtx* grp = nullptr;  // non-null only inside cugp_group_eval
    Scratch pred;                   // prediction scratch (predict_passes: test inputs, cross-covariance, its product with L^-T, results)
    bool overlap = true;           // hand inverse blocks to the other streams while the factorisation runs
    // a single-stream evaluation is captured once as a HIP graph and replayed: one launch call instead of
    // ~60 (1500 rows) -- with 16 experts on a GPU the host's launch rate was the bound, not the device
    cugp::HyperScalars* dhs = nullptr;   // device copy of exp(2*theta): what the kernels of a captured evaluation read
    cugp::HyperScalars* hhs = nullptr;   // pinned staging for it (refreshed by a copy node at the head of the graph)
    hipGraphExec_t gexec[2] = {nullptr, nullptr};   // [0] log-likelihood only, [1] with gradient
    unsigned gepoch[2] = {0, 0};   // cfg_epoch the graph was captured under
    // launch-shape tuning of THIS handle (kernels.h TUNE_*): the process defaults as of the last sync_tuning(), except the
    // keys set for this handle alone (cugp_set_handle_tuning)
    int tune[cugp::TUNE_COUNT] = {};
    bool tune_own[cugp::TUNE_COUNT] = {};
    unsigned cfg_epoch = 1;        // bumped when a launch shape of this handle changed: captured graphs carry launch shapes
    bool counted = false;          // this handle is in g_live[device] (the budget of barrier grids, barrier_cap)
    int bar_quota = -1;            // barrier workgroups reserved for this handle from the device's pool; < 0: not yet asked for
    double last_ll = NAN, last_quad = NAN, last_logdet = NAN;
    int prof = 0;                  // profiling level
    cugp::Profile pf;
    cugp::JointCov cov;
    cugp::Targets tg;
    cugp::Loo loo;
    // appending observations (cugp_append)
    bool bcm_expert = false;       // expert of a cugp_bcm (the experts' common padded size carries n)
    int groups = 0;                // the live cugp_groups that hold the handle (a group's device table carries n)
    bool is_factor = false;        // the internal factor handle (cov.f) of another handle
    bool x_full = false;           // dX holds npad rows (grown by the first append; n rows until then)
    Scratch app;                   // one pass: B = k(Xb, X), P = B L^-T, V = P L^-1 ([128][npad] each) and Qt ([npad][128])
};

// several experts of equal shape evaluated by one sequence of launches (group.h; evaluated in cugp_capi.cpp)
struct cugp_group {
    std::vector<cugp_gp*> experts;
    cugp::GroupCtx ctx;
    cugp::ExpertPtrs* dtab = nullptr;
    bool tab_valid = false;
    hipGraphExec_t gexec[2] = {nullptr, nullptr};
    unsigned gepoch[2] = {0, 0};
    bool pending = false, pending_grad = false;   // an evaluation is enqueued and not yet fetched
    Scratch pred;                   // grouped prediction scratch (predict_passes: test inputs, [expert][ntpad][npad] Ks and W)
};

namespace cugp {

// ---- cugp_capi.cpp
int invalid_arg(const char* call, const char* what);                 // CUGP_ERR_INVALID, "<call>: <what>"
int need_device(const char* call);                                   // CUGP_ERR_NODEVICE where the process sees no GPU
inline int use_device(const cugp_gp* g) { HIPCHK(hipSetDevice(g->device)); return CUGP_OK; }
int ensure(double** p, size_t count);                                // *p, or `count` doubles of device memory
HyperScalars scalars(const cugp_gp* g);
int cov_fn(cugp_gp* g, hipStream_t s, const HyperScalars* hd, CovFn* cf);
int ensure_factor_bufs(cugp_gp* g);
int ensure_inverse_bufs(cugp_gp* g);
int create_handle(int n, int d, int device, int npad_min, bool ard, cugp_gp** out, int kernel = KERNEL_SE, bool tied = false);
int cov_factor_handle(cugp_gp* g, int tiles);
int apply_stream_prio(cugp_gp* g);
void sync_tuning(cugp_gp* g);
void tune_defaults(int out[TUNE_COUNT]);                             // the process defaults as they stand now
int set_theta(cugp_gp* g, const double* th);
int fetch_eval(cugp_gp* g);
void discard_eval(cugp_gp* g);
bool read_result_row(cugp_gp* g, double* row, bool grad);
bool barrier_expired(double* row);
int reset_stamps(cugp_gp* g);
void drain_kernel_events(cugp_gp* g);
int enqueue_potrf(cugp_gp* g, bool with_inverse, bool mark = false, const unsigned* zeroed_tickets = nullptr);
int enqueue_trtri(cugp_gp* g);
bool same_loghyper(const cugp_group* gr);
int write_group_table(cugp_group* gr);
// the tail of a call's launches: e, the first error so far (hipGetLastError or a copy's); else the wait for s.  A failure
// drains s and is reported under the call's name.
int sync_or_fail(hipStream_t s, const char* call, hipError_t e);
// the end of an objective callback of the minimisers: f = -value and nh gradient entries, or NaN everywhere (!ok)
void objective_result(bool ok, double value, const double* grad, int nh, double* f, double* gr);
// cugp_cg_minimize_n's loop with the iterates as its record (minimize.cpp: cugp_cg_minimize_n_iterates), rows of n + 1; the
// row behind the last one written (when there is room) gets NaN in every entry, so a caller can count them
int cg_iterates(cugp_objective_n_fn fn, void* ctx, double* x, int n, int budget, double* rows, int rows_cap, int* nevals,
                int* nrows = nullptr);
inline int tri_tiles(int n) { return n * (n + 1) / 2; }

// ---- la.cpp
int la_factor_inverse(cugp_gp* g, bool inverse);

// ---- predict.cpp
struct PredBufs { double *xt, *w, *mean, *var; };   // where predict_passes left the test inputs, W = Ks L^-T and the means / variances
int predict_passes(cugp_gp* g, Batch bt, const double* Xt, int nt, int chunk, Scratch& scr, double* rows, size_t rstride,
                   PredBufs* pb = nullptr, bool latent = false);
int pred_chunk_rows(const cugp_gp* g, int count, int nt);
int predict_grad_passes(cugp_gp* g, Batch bt, int tiles, const double* Xt, int nt, bool with_noise, bool want_var,
                        Scratch& scr, double* rows, size_t row_stride, double** rows_out = nullptr);
int sample_tail(cugp_gp* g, cugp_gp* f, const double* dm, int nt, int nsamples, const double* normals, double* samples,
                const char* call);

// ---- sparse.cpp: one evaluation of the sparse model with its rows sharded over ranks, in the phases that lie around the
// two exchanges of comm.cpp (cugp_sparse_sharded_bound_grad).  Everything runs on one stream, the
// lead's (the first local shard's inner handle's).
constexpr int SHARD_HDR = 16;      // doubles in front of a rank's block of exchange 1: ShardEval::header
struct ShardEval {
    cugp_sparse* const* sh = nullptr;   // this rank's shards, slot order; sh[0] is the lead
    int nlocal = 0, rank = 0, world = 1, per = 0, nshards = 0, what = 0, device = 0;
    const char* call = "";
    int m = 0, d = 0, mpad = 0, nh = 0;
    size_t slot1 = 0, slot2 = 0;        // doubles per shard in exchange 1: [P mpad^2 | q mpad | y'y | n]; in exchange 2: [S_uf nl + 1 | gZ m d]
    hipStream_t stream = nullptr;
    double* hsend = nullptr;            // pinned [SHARD_HDR + per]: this rank's header, its shards' row counts
    double* hall = nullptr;             // pinned [world][SHARD_HDR]: every rank's header as gathered
    int status = 0;                     // this rank's own failure so far: it still joins exchange 1
    bool kuu_pd = false, done = false;  // Kuu was positive definite; the results stand (no exchange 2 follows)
    bool agreed = false;                // every rank's header was read and found in order: the ranks go on in step
    CovFn cf;                           // the lead's inner handle's covariance descriptor, taken in phase 1
};
// the checks on this rank's list that need the lead's shape: nonzero only where the rank cannot even size its block
int sp_shard_begin(ShardEval& e);
// Kuu, every local shard's chunk loop into its slot of `send`, the header; a failure becomes e.status and all-ones slots
void sp_shard_stats(ShardEval& e, double* send);
// the sums over the shards, B, the wait, every rank's header read by every rank, B's factorisation, c'
int sp_shard_solve(ShardEval& e, const double* gathered, size_t rstride);
// the M-side products, every local shard's trace passes and its row of `send`
int sp_shard_rows(ShardEval& e, double* send);
// the sums over the shards' rows, the square's Z pass, the final sums, the wait; then (also behind e.done) the results
int sp_shard_finish(ShardEval& e, const double* gathered, size_t rstride);
int sp_shard_results(const ShardEval& e, double* F, double* g, double* gZ);

// While an API call enqueues for handle g the launchers of kernels.hip read g's tuning (thread-local pointer).
struct TuneScope {
    const int* prev;
    explicit TuneScope(cugp_gp* g) : prev(t_tune) { sync_tuning(g); t_tune = g->tune; }
    ~TuneScope() { t_tune = prev; }
};

// one timed launch: event pair + bookkeeping.  Levels 2 and 3 record an event in front of and behind the launch on its
// stream; level 4 hands the pair to the launch itself (hipExtLaunchKernelGGL: the dispatch's own begin / end, no extra
// packets on the stream -- the schedule of the timed pass, and the durations rocprofv3 --kernel-trace reports)
// level 5: no events at all -- the launch's own workgroups stamp a slot of pf.dstamps (kernels.hip LaunchStamp)
struct TimedLaunch {
    cugp_gp* g; hipStream_t s; bool on, ext;
    // chain: this launch goes out on the main stream directly behind the main stream's latest timed launch
    TimedLaunch(cugp_gp* g_, hipStream_t s_, bool want, bool chain = false)
        : g(g_), s(s_), on(want && g_->pf.kev_used + 2 <= (int)g_->pf.kev.size()), ext(g_->prof >= 4)
    {
        Profile& p = g->pf;
        if (!on) { if (chain) p.last_main = -1; return; }       // an untimed launch breaks the chain
        p.kev_prev[p.kev_used / 2] = chain ? p.last_main : -1;
        if (chain) p.last_main = p.kev_used / 2;
        if (g->prof >= 5) stamp_next_launch(p.dstamps + p.kev_used / 2);
        else if (ext) time_next_launch(p.kev[p.kev_used], p.kev[p.kev_used + 1]);
        else if (hipEventRecord(p.kev[p.kev_used], s) != hipSuccess) on = false;
    }
    ~TimedLaunch() { if (on && ext && timing_pending()) { time_next_launch(nullptr, nullptr); stamp_next_launch(nullptr); } }   // the launch did not happen
    void done(int kind, double flop)
    {
        Profile& p = g->pf;
        if (!on) return;
        if (ext) { if (timing_pending()) return; }            // (armed but not consumed: nothing was launched)
        else if (hipEventRecord(p.kev[p.kev_used + 1], s) != hipSuccess) return;
        p.kev_kind[p.kev_used / 2] = kind;
        p.kev_flopv[p.kev_used / 2] = flop;
        p.kev_used += 2;
    }
};

}  // namespace cugp
