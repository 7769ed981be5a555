// kernels.h -- internal launch interface between the C-ABI (cugp_capi.cpp and the files of DESIGN.md's source map) and
// the gfx950 kernels (kernels.hip).  Not part of the public boundary.
//
// The structs and constants below are also what the host checks of the emulable device code (cov_device.h,
// append_device.h) see: tools/host_emul.h includes this file without a HIP runtime, with hipStream_t and hipEvent_t as
// opaque pointers for the launcher prototypes, so no check keeps a copy of HyperScalars, ExpertPtrs, KERNEL_* or TILE.
#pragma once
#ifndef CUGP_HOST_EMUL
#include <hip/hip_runtime.h>
#endif

namespace cugp {

constexpr int TILE = 128;          // tile edge of every fp64 MFMA product and of the padded leading dimension

// launch-shape thresholds, adjustable at run time for A/B tuning.  Every handle carries its own copy (cugp_gp::tune):
// cugp_set_tuning changes the process defaults under a lock, a handle takes them over when it next enqueues (keys set
// with cugp_set_handle_tuning stay as set), and the launchers below read the copy of the handle whose API call is running
// on this thread (t_tune) -- so handles driven from different threads never see each other's settings change mid-call.
enum { TUNE_LAUUM_WM2_MAX = 0,   // K^-1 product: use 64x64 tiles when there are at most this many 128-tiles
       TUNE_TRTRI_WM2_MAX = 1,   // inverse level: same rule
       TUNE_SYRK_REM_MAX = 2,    // trailing update: split the last partial round into 64x64 quarters when it has at most this many tiles
       TUNE_PIPE_BLOCK = 3,      // inverse rows (tiles) handed to the other streams at a time while the factorisation runs; 0 = after it, < 0 = by size (cugp_pipe_block_for; expert groups: about nt/16)
       TUNE_BORDER_WM2_MAX = 4,  // bordering step 1 (uniform K): 64x64 tiles when there are at most this many 128-tiles
       TUNE_GRAPHS = 5,          // replay single-stream evaluations as a captured HIP graph (1) or launch by launch (0)
       TUNE_GROUP_OVERLAP = 6,   // grouped experts: inverse blocks on the other streams beside the factorisation (1) or after it (0)
       TUNE_GROUP_MAX_TILES = 7, // experts up to this many tiles share launches (default: all; with the inverse beside the factorisation grouping won at every size tried: 4 x 6000 rows 18.9 -> 18.3 ms, 2 x 8192 rows 23.6 -> 21.9 ms)
       TUNE_PANEL = 8,           // two-speed Cholesky: steps per panel (far columns get K = 128*this in one pass per panel); 1 = classic
       TUNE_NEAR_TILES = 9,      // ... tiles in the near window (updated every step, K = 128) at a panel's first step
       TUNE_PANEL_MIN_NT = 10,   // ... only from this many tiles on (small matrices are bound by the chain alone)
       TUNE_LAUUM_STREAM = 11,   // the K^-1 share of an inverse block on its own stream beside the next block's bordering: 0 never, 1 expert groups only, 2 always
       TUNE_FINALIZE_FUSE_MAX = 12, // gradient evaluations: the last block of k_trace takes the final sums (no k_finalize launch) when the trace launch has at most this many blocks; 0 = always the separate launch
       TUNE_SPLIT_REM_MAX = 13,  // uniform-K launches (block-wise K^-1 share, bordering, wide update): a last round of at most this many tiles runs as 64x64 quarters
       TUNE_STEP_QUARTER_MAX = 14, // step kernel: launches of at most this many 64x64 workgroups run ALL their tiles as quarters (chain-bound tail)
       TUNE_STREAM_PRIO = 15,    // stream priorities of a handle (its streams are created with the handle and re-created, where the answer changes, by cugp_set_data,
                                 // cugp_set_handle_tuning, cugp_set_overlap and on joining a group or a BCM -- never inside an evaluation).  0 = by the rule: the
                                 // factorisation's stream at the highest priority for a handle that is evaluated alone with the inverse beside the factorisation and
                                 // has at least TUNE_PRIO_MIN_NT tile rows.  Explicit: bit 0 = the factorisation's stream at the highest priority, bit 1 = the inverse
                                 // streams at the lowest, 4 = no priorities whatever the rule says (prioritised streams serialised grouped experts in round 3)
       TUNE_BARRIER_SPIN = 16,   // polls a workgroup of k_trtri_block spends at a stage barrier before it gives up (the evaluation then fails with CUGP_ERR_DEVICE instead of hanging); 0 = give up at once (test hook)
       TUNE_SUBPANEL = 17,       // near window in sub-panels of this many steps (1 to 4; must divide the panel, else 1): the step launch of a sub-panel's last step
                                 // updates the window with K = 128*this in ONE pass over its C tiles, the steps before it only the next column (left-looking inside the sub-panel)
       TUNE_ZFUSE = 18,          // LL-only evaluations: the forward substitution L z = y inside the factorisation's launches (1) or as 2 nt launches behind it (0)
       TUNE_PRED_CHUNK = 19,     // grouped prediction (cugp_group_predict_enqueue): test points per pass, in 64-row tiles; 0 = as many as keep the
                                 // passes' cross-covariance and product scratch within 1 GiB per group (the bits do not depend on it)
       TUNE_COV_SPLIT = 20,      // joint predictive covariance (k_predict_cov): 64x64 workgroup slots the launch aims to fill by splitting each
                                 // output tile's k range (128x128 workgroups count as two); 64x64 output tiles while the lower 128-tiles
                                 // are at most a quarter of it; 0 = 128x128 tiles, no split
       TUNE_PRIO_MIN_NT = 21,    // TUNE_STREAM_PRIO = 0: tile rows from which a lone handle's factorisation stream gets the highest priority (the chain's small launches
                                 // then wait less behind the 1000-workgroup launches of the inverse streams: 64 tiles -0.5 %, 79 -1.2 %, 128 -0.9 %; 32 and 47 tiles
                                 // gained nothing beyond their run-to-run spread)
       TUNE_WAVES8 = 22,         // the whole 128x128 tiles of the uniform-K launches (k_syrk_wide, k_lauum<4>, k_trtri_border<4> step 1) on eight waves
                                 // (512 threads, 32x64 outputs per wave; the last round's 64x64 quarters follow in a four-wave launch of their own): the same
                                 // bits; default 0 (measured: profiles/r07_ab_parts.txt)
       TUNE_COUNT = 23 };
extern const int g_tune_init[TUNE_COUNT];     // built-in defaults
extern thread_local const int* t_tune;        // the tuning the launchers on this thread read (a handle's copy, or the built-in defaults)
inline int tune(int key) { return t_tune[key]; }

// covariance family of a handle (cugp.h: CUGP_KERNEL_*), fixed when it is created
// KERNEL_COUNT: the kinds the isotropic / ARD / sparse create calls take.  KERNEL_RQ (rational quadratic) lies beyond it: it
// has a create call of its own (cugp_create_rq) because it carries a shape parameter, and no isotropic instantiation.
enum { KERNEL_SE = 0, KERNEL_MATERN32 = 1, KERNEL_MATERN52 = 2, KERNEL_COUNT = 3, KERNEL_RQ = 3 };
// hyper-parameters of a family that are neither a length scale nor a variance (RQ: alpha).  In theta they stand behind
// the length scales and in front of sigma_f, sigma_n; their device values follow the d weights in the staging area.
constexpr int shape_count(int kind) { return kind == KERNEL_RQ ? 1 : 0; }

// Batched launches: the experts of a BCM on one device have the same shapes, so one launch can serve all of
// them -- blockIdx.y picks the expert and the kernel takes its buffers from a device-resident table instead
// of its pointer arguments.  (16 experts x ~45 launches per evaluation from 16 streams were bounded by the
// command processor, not by the CUs.)
struct ExpertPtrs {
    double *A, *T, *U, *Kinv, *d16, *d64, *logdet, *y, *z, *alpha, *w, *part, *out;
    const double* X;
    unsigned* tickets;
    int n;
};
struct Batch {
    const ExpertPtrs* tab = nullptr;   // nullptr: one expert, buffers from the arguments
    int count = 1;
};

struct HyperScalars {              // exp(2*theta) evaluated on the host, as the reference does (covkernel.cpp:65-67)
    double ell_sq, signal_var, noise_var;
};

// The covariance function of a handle as the launchers see it.  The passes that evaluate it (build, cross-covariance,
// joint-covariance epilogue, gradient trace, multi-target gradient trace, test-input gradient) take one of these and launch
// the instantiation it names: each pass is ONE kernel template with one argument list, k_build / k_cross /
// k_predict_cov_finish / k_trace / k_trace_targets / k_predict_grad <ARD, KIND>, picked by one table (kernels.hip
// CUGP_COV_KERNEL) -- every instantiation with everything SE's launches carry (batched experts, ticket zeroing,
// device-resident hyper-scalars, stamps; the fused final sums are isotropic only).
//   h:   the hyper-scalars by value
//   hd:  (optional) the same in device memory, read INSTEAD of h by the passes a captured graph replays (build, trace,
//        k_finalize): the graph sees new hyper-parameters by one copy into that buffer
//   ard: one length scale per input dimension (GPML covSEard's convention; the reference has no counterpart):
//        k(x, x') = sf2 exp(-1/2 sum_c ((x_c - x'_c) w_c)^2) + sn2 delta, w_c = exp(-theta_c) evaluated on the host.  hd is
//        then mandatory and read by every pass: the hyper-scalars (ell_sq unused) directly followed by the d weights --
//        one staging area, one copy; the kernels ignore h.  Same tiles, stores and padding as the isotropic launches.
//        kind != KERNEL_SE: the Matern entry of the same weighted distance.  Batched
//        experts (build, cross-covariance, trace; not the joint-covariance epilogue) read the GROUP's one copy -- the lead
//        expert's hd -- since the experts of a group share their hyper-parameters.  An ARD descriptor without hd is a
//        programming error -- asserted, so checked only in builds without NDEBUG (the library's own build has none).
//   kind == KERNEL_RQ: k = sf2 (1 + s / (2 alpha))^-alpha of the weighted squared distance s (cov_device.h rq_entry); always
//        the ARD route.  Staging area: [HyperScalars][w_1 .. w_d][alpha, 0.5 / alpha], still one copy.  Gradient partials:
//        [d length columns][shape_count(kind) shape columns][sum W o K][tr W].
//   tied: the d weights are one length scale's (theta holds it once: nh = 1 + shape_count + 2).  The N^2 passes are the ARD
//        ones; the final sums add the d length columns' results in index order into the one component.
struct CovFn {
    int kind = KERNEL_SE;
    bool ard = false;
    HyperScalars h = {};
    const HyperScalars* hd = nullptr;
    bool tied = false;
};

// ---- covariance (N1) ----
// lower 64x64 tiles of K (+ mirror when `full`), padding rows/cols >= n set to identity
void launch_kbuild(const double* X, int n, int d, int npad, const CovFn& cf, double* K, bool full, hipStream_t s,
                   Batch bt = {}, unsigned* tickets = nullptr);
                   // tickets: the factorisation's arrival counters -- 2 * npad/128 per expert ([0, nt) the step tickets of
                   // k_syrk_step, [nt, 2 nt) the stage counters of k_trtri_block) --, zeroed by the launch when given
// S[i][j] = |x_i - x_j|^2 / c, zero diagonal, full symmetric (N2, covkernel.cpp:130-157)
void launch_sqdist(const double* X, int n, int d, int npad, double c, double* S, hipStream_t s);
// Ks[t][i] = sf2 * exp(-0.5*|x_i - xt_t|^2 / l^2), row-major nt_pad x npad (pad = 0)   (N12)
// bt (batched): blockIdx.y = expert, X and n from the table, Ks[expert][ntpad][npad]
void launch_kcross(const double* X, int n, int d, int npad, const double* Xt, int nt, int ntpad,
                   const CovFn& cf, double* Ks, hipStream_t s, Batch bt = {});

// ---- blocked right-looking Cholesky (N4) on the lower triangle of A (npad x npad, ld = npad) ----
// (definitions: chol_gfx950.h, each launcher behind its kernel)
// d16: 16x16 diagonal inverses [nt][8][256]; d64: the two 64x64 diagonal inverses of each block [nt][2][4096]
void launch_potf2(double* A, int ld, int kb, double* d16, double* d64, double* logdet_part, hipStream_t s,
                  Batch bt = {});
// zv / wv (when given): the forward substitution L z = y rides along -- one more workgroup computes z_kb = L_kk^-1 w_kb
// from the block's 64x64 inverses (w: the running right-hand side, y at first); kb = nt - 1 launches that workgroup alone
void launch_trsm_inv64(double* A, const double* d64, int ld, int kb, int nt, hipStream_t s, Batch bt = {},
                       double* zv = nullptr, const double* wv = nullptr);   // 3-phase, 64x64 inverses
// trailing update of step kb fused with the factorisation of diagonal block kb+1 (tickets[kb] must be 0)
// wcol > 0: only the tile columns [kb+1, kb+1+wcol) (two-speed form: the near window)
// ks: first k tile of the pass (sub-panels: the k tiles [ks, kb], at most SUBPANEL_MAX of them); < 0: kb alone
constexpr int SUBPANEL_MAX = 4;
void launch_syrk_step(double* A, int ld, int kb, int nt, double* d16, double* d64, double* logdet_part,
                      unsigned* tickets, hipStream_t s, Batch bt = {}, int wcol = 0, int ks = -1,
                      const double* zv = nullptr, double* wv = nullptr);
                      // zv / wv (when given): nt - kb - 1 more workgroups apply w_i -= L(i,kb) z_kb to the rows below
// wide trailing update: tile columns [ca, cb) (rows >= column) -= L(., k tiles [k0, k0+kw)) L(.)^T; returns tiles
int launch_syrk_wide(double* A, int ld, int nt, int k0, int kw, int ca, int cb, int rev, hipStream_t s, Batch bt = {});

// ---- triangular inverse by recursive doubling (N7) and K^-1 = U U^T (N8) ----
// (definitions: inverse_gfx950.h, each launcher behind its kernel)
void launch_trtri_diag(const double* A, int ld, int kb, int nblocks, const double* d64, double* T, double* U,
                       hipStream_t s, Batch bt = {});
// inverse of the hand-over block of rows [a, a + wb) in one launch: diagonal-tile inverses + every doubling level inside
// the block (k_trtri_block; wb <= TRTRI_BLOCK_MAX_TILES).  ctr: the block's stage counter (zero before the launch; batched:
// tickets[ctr_off] of every expert); poison: log-determinant shares (entry a becomes NaN if a stage wait ran out)
// gcap: most workgroups the launch may hold at its stage barriers (the caller's share of the device's budget for
// barrier grids, cugp_capi.cpp: barrier_cap); hstat: pinned host word ([expert][8] doubles, entry 6) that is set when a
// stage wait ran out -- the evaluation's fetch then returns CUGP_ERR_DEVICE
constexpr int TRTRI_BLOCK_MAX_TILES = 16;
constexpr int TRTRI_BLOCK_MAXWG = 64;
int launch_trtri_block(const double* L, const double* d64, double* T, double* U, int ld, int a, int wb, unsigned* ctr,
                       double* poison, int ctr_off, hipStream_t s, Batch bt = {}, int gcap = TRTRI_BLOCK_MAXWG,
                       double* hstat = nullptr);
// off: element offset of the diagonal sub-matrix (nt tiles) the level works on inside L, T, U
// (these four return the edge of the output tiles they launched with, in 32s: 4 = 128x128, 2 = 64x64, 0 = nothing)
int launch_trtri_level(const double* L, double* T, double* U, int ld, int nt, int s, int step, hipStream_t st,
                       Batch bt = {}, size_t off = 0);
// bordering step 1, one k chunk: Wt(tj < c1, ti in [ra, ra+rw)) (+)= sum_{k in [max(tj,c0), c1)} U[tj][k] L[ti][k]
int launch_trtri_border1(const double* L, double* T, double* U, int ld, int ra, int rw, int c0, int c1,
                         hipStream_t st, Batch bt = {});
// bordering step 2: rows [a, a+w) of the inverse from their finished Wt and the block's own inverse
int launch_trtri_border2(const double* L, double* T, double* U, int ld, int a, int w, hipStream_t st,
                         Batch bt = {});
// Kinv(lower tiles < a+w) (+)= contribution of inverse rows [a, a+w); a = 0, w = nt: the whole product
int launch_lauum(const double* U, double* Kinv, int ld, int a, int w, hipStream_t s, Batch bt = {});

// ---- prediction products ----
// W[t][i] = sum_{k<=i} Ks[t][k] T[i][k]   (nt_pad x npad, row-major)
// batched: blockIdx.y = expert, T from the table, Ks and W [expert][ntt * 128][ld]; every expert's tiles sum the same k
// range in the same order as its single launch, so each expert's bits are those of cugp_predict
void launch_predict_gemm(const double* Ks, const double* T, double* W, int ld, int ntt, int nt, hipStream_t s,
                         Batch bt = {});
// joint predictive covariance (cugp_predict_cov / cugp_predict_sample).  Shape of the product P = W W^T over the lower
// tiles of an ntpad x ntpad result against n training rows: output tiles of 32 * wm (tiles of them), the k range [0, kend)
// in split chunks of kstep (tuning key TUNE_COV_SPLIT); the caller provides split - 1 scratch slots of ntpad^2 doubles
struct CovShape { int wm, tiles, kend, kstep, split; };
CovShape predict_cov_shape(int ntpad, int n);
// chunk 0 of every tile -> A (ld = ntpad), chunk s > 0 -> scr + (s - 1) * ntpad^2; W: [ntpad][ld]
void launch_predict_cov(const double* W, int ld, int ntpad, const CovShape& c, double* A, double* scr, hipStream_t s);
// A (lower 64x64 tiles, in place) = k(Xt,Xt) (+ sn2 on the diagonal when with_noise) + jitter I - (A + scr[0] + ...
// + scr[nscr - 1]), identity beyond nt; tickets (when given): the factorisation's arrival counters, zeroed
void launch_predict_cov_finish(const double* Xt, int nt, int d, int ntpad, const CovFn& cf, bool with_noise,
                               double jitter, double* A, const double* scr, int nscr, unsigned* tickets, hipStream_t s);
// strict upper triangle of the nt diagonal 128x128 tiles of A := 0
void launch_zero_upper_diag(double* A, int ld, int nt, hipStream_t s);
// out[s * nt + t] = mean[t] + F[s * ld + t]   (s < ns, t < nt)
void launch_sample_finish(const double* F, int ld, const double* mean, int nt, int ns, double* out, hipStream_t s);
// mean / var (may be null) and, when rows is given, the product-of-experts exchange rows: 1/var at rows[t], mean/var at
// rows[rhalf + t] (batched: expert e's at rows + e * rstride; alpha from the table, Ks and W [expert][ntpad][npad])
void launch_predict_finish(const double* Ks, const double* W, const double* alpha, int n, int npad, int ntest,
                           HyperScalars h, double* mean, double* var, hipStream_t s, double* rows = nullptr,
                           size_t rstride = 0, int rhalf = 0, int ntpad = 0, Batch bt = {});
// ---- gradients of the prediction with respect to the test inputs (cugp_predict_grad) ----
// Per 64 x 64 (test x training) tile the partial sums over the tile's training rows of (G alpha_i)(x*_c - x_ic) and, V
// given, (G V_ti)(x*_c - x_ic):  part[(ti * 2 + q) * pstride + t * d + c], ti < predict_grad_tiles(n), q = 0 mean / 1
// variance, t < nt, pstride >= nt * d.  Xt: the pass's nt test points; Ks (k_cross's output) and V = W L^-1
// (launch_targets_alpha(W, U, V, npad, rows of the pass padded to 128)) are [>= nt rounded up to 64][npad]; V null: the
// mean's sums alone.  The finish adds the tiles in index order and writes dmean = -s_c sum, dvar = 2 s_c sum, packed
// [nt][d] (either may be null; dvar only where the tile launch had V).
constexpr int predict_grad_tiles(int n) { return (n + 63) / 64; }
void launch_predict_grad(const double* X, int n, int d, int npad, const double* Xt, int nt, const CovFn& cf,
                         const double* Ks, const double* V, const double* alpha, double* part, size_t pstride,
                         hipStream_t s);
void launch_predict_grad_finish(const double* part, size_t pstride, int n, int nt, int d, const CovFn& cf, double* dmean,
                                double* dvar, hipStream_t s);
// The same for the experts of a group in ONE launch each (blockIdx.y = expert; X, n, alpha, U from the table bt), the
// passes of cugp_group_predict_grad_enqueue.  Ks, W, V: [expert][cpad][npad] slices (kslice = cpad * npad doubles);
// partial sums: [expert][tiles_max * 2][pstride], tiles_max = the most 64-row training tiles of any expert -- every
// expert sums its own count.  Rows: expert e's outputs at (pointer) + e * row_stride.
//   finish_mv:     m and v themselves (k_predict_finish's sums) -> mean[e * row_stride + t], var[...]
//   targets_alpha: V = W L^-1 per expert (k_targets_alpha's tile pairing and k ranges; m = cpad)
//   grad:          k_predict_grad_batched<ARD, KIND>; V null: the mean's sums alone
//   grad_finish:   dmean / dvar (dvar may be null) packed [nt][d] per expert
void launch_predict_finish_mv(const double* Ks, const double* W, int npad, int ntest, HyperScalars h, double* mean,
                              double* var, size_t row_stride, int ntpad, hipStream_t s, Batch bt);
void launch_targets_alpha_batched(const double* Z, double* A, int npad, int m, hipStream_t s, Batch bt);
void launch_predict_grad_batched(int d, int npad, const double* Xt, int nt, const CovFn& cf, const double* Ks,
                                 const double* V, size_t kslice, double* part, size_t pstride, int tiles_max,
                                 hipStream_t s, Batch bt);
void launch_predict_grad_finish_batched(const double* part, size_t pstride, int tiles_max, int nt, int d, const CovFn& cf,
                                        double* dmean, double* dvar, size_t row_stride, hipStream_t s, Batch bt);
// combined prediction and its test-input gradients over a gathered buffer of gradient rows ([world][rstride]: {status,
// count, [per] x [m nt | v nt | dmean nt d | dvar nt d]}): out = [mean nt | var nt | dmean nt d | dvar nt d | world x
// {status, count}]; mode -1 .. 3 (CUGP_COMBINE_REFERENCE .. CUGP_COMBINE_RBCM)
void launch_poe_reduce_grad(const double* g, size_t rstride, int world, int K, int nt, int d, int mode, double sf2,
                            double sn2, int with_noise, int want_dvar, double* out, hipStream_t s);
// product of experts over a gathered exchange buffer ([world][rstride]: {status, count, [per][2][nt]}): out = [mean nt |
// var nt | world x {status, count}], experts summed in global order (expert k = rank k mod world's slot k / world)
void launch_poe_reduce(const double* g, size_t rstride, int world, int K, int nt, double* out, hipStream_t s);
// the same buffer and output with LATENT rows (1/var_f, mean/var_f) combined by rule `mode` (CUGP_COMBINE_*: 0 PoE, 1 gPoE,
// 2 BCM, 3 rBCM); sf2: the latent prior variance at a test point, sn2 added to the variance when with_noise
void launch_poe_reduce_mode(const double* g, size_t rstride, int world, int K, int nt, int mode, double sf2, double sn2,
                            int with_noise, double* out, hipStream_t s);

// ---- vector kernels ----
void launch_trmv_lower(const double* T, int ld, int npad, const double* x, double* z, hipStream_t s,
                       Batch bt = {});                                                                 // z = T x
void launch_trmv_upper(const double* U, int ld, int npad, const double* x, double* a, hipStream_t s,
                       Batch bt = {});                                                                 // a = U x
void launch_trsv_lower(const double* A, const double* T, int ld, int nt, const double* y, double* z,
                       hipStream_t s, Batch bt = {});                                                  // L z = y
void launch_copy_y_to_w(int npad, hipStream_t s, Batch bt);                                            // batched only
// gradient traces (N10+N11 fused): partial sums per block into part[3*nblocks]
int trace_num_blocks(int npad);
// out (when given): the launch also FINISHES the evaluation -- its last block (an arrival ticket, zero before the launch)
// takes the final sums and writes out[0..5] (and hout) as launch_finalize would: z, logdet_part as there; batched:
// taken from the experts' table, ticket = tickets[2 nt] of every expert
// ARD: part[ard_part_columns(cf, d) * trace_num_blocks(npad)]; results row out / hout (both mandatory, ARD_ROW_GRAD + nh
// doubles, nh = ard_num_hyper(cf, d)): [0] LL, [4] y'K^-1y, [5] log|K|, [6] status word (as the isotropic row),
// [ARD_ROW_GRAD + c] g_c, c = 0 .. nh - 1.  Always two launches (k_trace<true, KIND>, k_finalize_ard or its tied form):
// there is no fused form of the final sums, and ticket is not used.  Batched: grids (blocks, experts) and (1, experts);
// part and out from the table, hout[expert][ARD_ROW_GRAD + nh].
constexpr int ARD_ROW_GRAD = 8;
// columns of an nh-wide handle's gradient partials, and the entries of its theta
inline int ard_part_columns(const CovFn& cf, int d) { return d + shape_count(cf.kind) + 2; }
inline int ard_num_hyper(const CovFn& cf, int d) { return (cf.tied ? 1 : d) + shape_count(cf.kind) + 2; }
void launch_trace(const double* X, int n, int d, int npad, const CovFn& cf, const double* Kinv, const double* alpha,
                  double* part, hipStream_t s, Batch bt = {}, const double* z = nullptr,
                  const double* logdet_part = nullptr, double* out = nullptr, double* hout = nullptr,
                  unsigned* ticket = nullptr);
// arrival counters per expert: [0, nt) step tickets, [nt, 2 nt) stage counters of k_trtri_block, [2 nt] k_trace's fused finalize
constexpr int ticket_count(int nt) { return 2 * nt + 1; }
// out[0..3] = LL, g0, g1, g2  (LL only when part == nullptr)
void launch_finalize(const double* z, int npad, int n, const double* logdet_part, int nt, const double* part,
                     int nblocks, HyperScalars h, double* out, double* hout, hipStream_t s,
                     const HyperScalars* hd = nullptr, Batch bt = {});   // hout: pinned host copy of the results ([expert][8]) or null
// ---- multi-target regression (cugp_set_targets): everything target-major [mpad][npad], zero beyond n and beyond m ----
// Z = Y L^-T is launch_predict_gemm(Y, T, Z, ...) as it stands (mpad a multiple of 128).
// A[t][j] = sum_{k >= j} Z[t][k] U[j][k]: row t = alpha_t = K^-1 y_t (64-row target tiles: the first (m + 63) / 64 of them)
void launch_targets_alpha(const double* Z, const double* U, double* A, int npad, int m, hipStream_t s);
// gradient traces of the summed objective, W = m K^-1 - sum_t alpha_t alpha_t^T, K^-1 read once: partial sums per block in
// launch_trace's layouts (isotropic part[3 * nblocks], ARD part[ard_part_columns * nblocks]; nblocks = trace_num_blocks(npad))
void launch_trace_targets(const double* X, int n, int d, int npad, const CovFn& cf, const double* Kinv, const double* A,
                          int m, double* part, hipStream_t s);
// one workgroup: out / hout (pinned) [0] LL = sum_t LL_t, [1 + c] the nh components of the gradient of -LL (nh = 3, ARD
// ard_num_hyper), [1 + nh + t] LL_t = -0.5 (z_t'z_t + logdet + n * 1.83787); logdet NaN (no factor): every entry NaN
void launch_finalize_targets(const double* Z, int npad, int n, int d, int m, double logdet, const double* part,
                             const CovFn& cf, double* out, double* hout, hipStream_t s);
// mean[t * nt + i] = sum_k A[t][k] Ks[i][k] (Ks [ntpad][npad], pad = 0): 64x64 output tiles, the k range in chunks of
// TARGETS_MEAN_KSTEP whatever m is, partial products in P (targets_mean_split(npad) * ((m + 63) / 64 * 64) * ntpad doubles),
// added in chunk order by a second launch
constexpr int TARGETS_MEAN_KSTEP = 512;
int targets_mean_split(int npad);
void launch_targets_mean(const double* A, const double* Ks, double* P, int npad, int m, int nt, int ntpad, double* mean,
                         hipStream_t s);
// ---- appending observations (cugp_append): one bordering step by the k <= 128 new rows [r0, r0 + k) of ONE tile row ----
// P = B L^-T and V = P L^-1 ([128][ld], zero beyond row k and column r0); Cf = chol(S) and Ci = its inverse (lower, ld =
// 128, identity beyond k, Ci zero above the diagonal), flog[0] = sum log C_ii -- the factor handle's A, T and logdet.
// Writes rows [r0, r0 + k) of A (P | C), T (Q | C^-1, Q = -C^-1 V) and Kinv (C^-T Q | C^-T C^-1), the same columns of U,
// z[r0 ..] = zb = C^-1 (y[r0 ..] - P z), alpha[r0 ..] = C^-T zb, logdet[r0 / 128] += flog[0], and Qt ([npad][128]):
// Qt[j][i] = Q[i][j], zero beyond k and for the rows j in [r0, r0 rounded up to 64).
void launch_append_border(const double* P, const double* V, const double* Cf, const double* Ci, const double* flog, int r0,
                          int k, int ld, double* A, double* T, double* U, double* Kinv, const double* y, double* z,
                          double* alpha, double* logdet, double* Qt, hipStream_t s);
// lower 64x64 tiles of Kinv[0, r0) += Q'Q (fp64 MFMA, Qt as both operands, k rounded up to 16) and alpha[0, r0) += Q' zb
void launch_append_kinv(const double* Qt, int r0, int k, int ld, double* Kinv, const double* zb, double* alpha,
                        hipStream_t s);
// ---- leave-one-out cross-validation (cugp_loo; loo_device.h): plain launches on s, fixed-order sums ----
// pt: [LOO_PT_ROWS][npad] -- mean, variance, log predictive density, a = alpha / kappa, s = sqrt(c), zero beyond n; then
// one workgroup adds the densities: out[0] = hout[0] = L_LOO (out: device row, hout: pinned)
constexpr int LOO_PT_ROWS = 5;
void launch_loo_point(const double* Kinv, const double* alpha, const double* y, int n, int npad, double* pt, double* out,
                      double* hout, hipStream_t s);
// Bm (full npad x npad) = K^-1 diag(s) from the lower 64x64 tiles of K^-1, zero beyond n; b = K^-1 a through the tiles'
// shares bpart ([npad / 64][npad]), added in tile order
void launch_loo_mirror_scale(const double* Kinv, const double* pt, int n, int npad, double* Bm, double* bpart, double* b,
                             hipStream_t s);
// P (lower 128-tiles, diagonal tiles complete) = Bm Bm^T, K = npad for every tile; returns the tile edge in 32s (4 or 2)
int launch_loo_product(const double* Bm, double* P, int npad, hipStream_t s);
// gradient pass over the lower tiles of P with W_loo = P - b alpha^T - alpha b^T (part: (nl + 2) * trace_num_blocks(npad),
// nl = 1 or ARD's d + shape_count) and its final sums: out[1 ..] = hout[1 ..] = the nh components of d(-L_LOO) / dtheta
void launch_trace_loo(const double* X, int n, int d, int npad, const CovFn& cf, const double* P, const double* alpha,
                      const double* b, double* part, double* out, double* hout, hipStream_t s);
// ---- sparse variational GP regression on inducing points (cugp_sparse_*; sparse_device.h) ----
// The schedule of pass `pass` over n data rows in chunks of chunk_rows (0: SPARSE_CHUNK_DEFAULT) against mpad padded
// inducing points -- what cugp_sparse_plan reports: the chunk's rows [r0, r0 + count), cpad = count rounded up to 128
// (the k range of its Gram launch), and that launch's split: workgroup (tile, s) sums k in [s kstep, min((s + 1) kstep,
// cpad)).  The split aims at SPARSE_GRAM_SLOTS 128x128 workgroups (two per CU) with at least 256 k each, at most 64 ways,
// its scratch (split * mpad^2 doubles) within 1 GiB.  Pure arithmetic.
constexpr int SPARSE_CHUNK_DEFAULT = 16384;
constexpr int SPARSE_GRAM_SLOTS = 512;
struct SparseShape { int chunks, r0, count, cpad, split, kstep; };
SparseShape sparse_shape(int n, int mpad, int chunk_rows, int pass);
// P (lower 128-tiles of mpad^2, diagonal tiles complete) = (first ? 0 : P) + W^T W, W: [c.cpad][mpad] (k_sparse_gram: the
// split-k partial tiles into scr, c.split * mpad^2 doubles; k_sparse_gram_finish adds them in index order)
void launch_sparse_gram(const double* W, int mpad, const SparseShape& c, double* P, double* scr, bool first, hipStream_t s);
// Bm (lower 128-tiles, diagonal tiles complete) = I + P / s2
void launch_sparse_form_b(const double* P, int mpad, double s2, double* Bm, hipStream_t s);
void launch_sparse_transpose(const double* src, double* dst, int mpad, double scale, hipStream_t s);   // dst = scale src^T
// G ([cpad][mpad]) = W R^T: the plain NT product on the tile (k_test_gemm), K = mpad
void launch_sparse_weights(const double* W, const double* R, double* G, int cpad, int mpad, hipStream_t s);
// the rectangular gradient pass (k_trace_cross<ARD, KIND>) over the rows_pad / 64 x mpad / 64 tiles of G, w = G + yv bv^T
// (yv null: none); partials part[c * pstride + pofs + block], c = 0 .. nl (nl = 1 or ARD's d; column nl: sum w o K)
void launch_trace_cross(const double* Xr, int nr, int rows_pad, const double* Z, int m, int d, int mpad, const CovFn& cf,
                        const double* G, const double* yv, const double* bv, double* part, size_t pstride, size_t pofs,
                        hipStream_t s);
// The gradient with respect to the inducing inputs (sparse_z_device.h): one pass of
// k_trace_cross_z<ARD, KIND> over the rows_pad / 64 x mpad / 64 tiles of G (w = G + yv bv^T; yv null: none) and
// k_trace_cross_z_finish behind it.  Workgroup (column tile, range) sums `per` consecutive row tiles; the ranges per column
// tile aim at SPARSE_Z_SLOTS workgroups (two per CU) of at least 256 rows, their partial blocks (ranges * m * d doubles in part) within 1 GiB:
// sparse_z_shape is a pure function of (rows_pad, mpad, d).  acc ([m][d]): the running sums over the passes (first: it
// starts from zero); last: out[j d + c] = hout[..] = -(s_c acc), the gradient of -F.
constexpr int SPARSE_Z_SLOTS = 512;
struct SparseZShape { int row_tiles, per, ranges; };
SparseZShape sparse_z_shape(int rows_pad, int mpad, int d);
void launch_trace_cross_z(const double* Xr, int nr, int rows_pad, const double* Z, int m, int d, int mpad, const CovFn& cf,
                          const double* G, const double* yv, const double* bv, double* part, double* acc, bool first,
                          bool last, double* out, double* hout, hipStream_t s);
// mean = Vt c' / s2, var = sf2 - |Wt_t|^2 + |Vt_t|^2 + noise per test row (Wt, Vt: [>= nt][mpad])
void launch_sparse_predict_finish(const double* Wt, const double* Vt, const double* cp, int mpad, int nt, double sf2,
                                  double s2, double noise, double* mean, double* var, hipStream_t s);
// ---- joint covariance and input gradients of the sparse prediction ----
// partial products Wt Wt^T - Vt Vt^T of the lower tiles in launch_predict_cov's layout and split (c from
// predict_cov_shape(ntpad, mpad)); launch_predict_cov_finish follows it.  Wt, Vt: [ntpad][ld], zero beyond row nt and column m
void launch_sparse_predict_cov(const double* Wt, const double* Vt, int ld, int ntpad, const CovShape& c, double* A,
                               double* scr, hipStream_t s);
// D = Wt - T over `rows` rows of mpad (D null: left out) and (a given) a[i] = bp[i] / s2 for i < m, 0 up to mpad
void launch_sparse_predict_diff(const double* Wt, const double* T, double* D, int mpad, int rows, const double* bp, double s2,
                                int m, double* a, hipStream_t s);
// ---- what reads the labels of the sparse model: p targets over one set of inducing points (cugp_sparse_*_targets), and
// the handle's own y as p = 1 (sparse_targets_device.h): Y [p][ystride] target-major, every row zero
// padded to the chunks' 128-row tiles; Q, C', Gamma', Beta', Bs [>= p][mpad] ----
// Q[t] (mpad) = (first ? 0 : Q[t]) + W^T y_t for every target, W read once per group of 8 targets; Y: the chunk's first row
// of target 0; part: p * (cpad / 128) * mpad doubles, the slabs' shares, added in slab order
void launch_sparse_wty_targets(const double* W, int mpad, int cpad, const double* Y, size_t ystride, int p, double* part,
                               double* Q, bool first, hipStream_t s);
void launch_sparse_yy_targets(const double* Y, size_t ystride, int n, int p, double* out, hipStream_t s);   // out[t] = y_t'y_t
// H = p (I - B^-1) - sum_t gamma_t gamma_t^T, H2 = H - p P / s2 (full mpad^2, zero beyond m; gamma_t = Gm[t] / s2),
// Bs[t] = Bt[t] / s2^2
void launch_sparse_h_targets(const double* Binv, const double* P, const double* Gm, const double* Bt, int p, int m, int mpad,
                             double s2, double* H, double* H2, double* Bs, hipStream_t s);
// G ([cpad][mpad], in place) += sum_t y_t Bs[t]^T over its first nr rows and m columns, t ascending
void launch_sparse_weights_targets(double* G, int cpad, int mpad, const double* Y, size_t ystride, const double* Bs, int p,
                                   int nr, int m, hipStream_t s);
// Cs ([rows][mpad], rows = p rounded up to 64) = C' / s2, zero beyond p: the first operand of launch_targets_mean
void launch_sparse_scale_targets(const double* Cm, int p, int rows, int m, int mpad, double s2, double* Cs, hipStream_t s);
// what the last launch of an evaluation reads beside the trace partials
struct SparseFinalTargets {
    const double *P, *Binv;        // ld x ld: their diagonals
    const double *Cp, *Gm;         // C' and Gamma', [p][ld] (Gm is read for the gradient only)
    const double *logdet;          // the factor of B: one share sum log L_ii per 128-tile
    const double *yy;              // y_t'y_t, p of them
    int m, ld, nt, p;
    double n, sf2, s2, log_s2;     // N as a double, exp(2 theta_f), exp(2 theta_n), 2 theta_n
};
// one workgroup: out / hout [0] F = sum_t F_t, (part_uf given) [1 ..] the nl + 2 components of d(-F) / dtheta,
// [1 + nl + 2 + t] F_t
void launch_sparse_finalize_targets(const SparseFinalTargets& f, const double* part_uf, size_t nb_uf, const double* part_uu,
                                    size_t nb_uu, int nl, double* out, double* hout, hipStream_t s);
// ---- the sparse model with its rows sharded over ranks (cugp_sparse_sharded_*; sparse_shard_device.h)
// out[e] = sum over the shards k = 0 .. nshards - 1, in that order, of entry off + e of shard k's slot (rank k % world's
// block at src + (k % world) * rstride: [hdr | slots of `slot` doubles], slot k / world), e < len
void launch_sparse_shard_reduce(const double* src, size_t rstride, size_t hdr, size_t slot, size_t off, size_t len, int world,
                                int nshards, double* out, hipStream_t s);
// out[c] = the sum of column c of a shard's trace partials (c <= nl) in k_sparse_finalize_targets' order; one workgroup
void launch_sparse_shard_sums(const double* part_uf, size_t nb_uf, int nl, double* out, hipStream_t s);
// SparseFinalTargets at p = 1 with y'y and N on the device: yyn = {y'y, N}, both summed over the shards
struct SparseFinalSharded {
    const double *P, *Binv, *Cp, *Gm, *logdet, *yyn;
    int m, ld, nt;
    double sf2, s2, log_s2;
};
// one workgroup: launch_sparse_finalize_targets' results at p = 1 from the reduced sums suf[nl + 1] of the rectangle
// (NULL: F only) and the square's partials
void launch_sparse_finalize_sharded(const SparseFinalSharded& f, const double* suf, const double* part_uu, size_t nb_uu, int nl,
                                    double* out, double* hout, hipStream_t s);
// profiling level 4: the NEXT launch of a timed kernel (trailing updates, inverse products, k_trtri_block,
// k_predict_gemm) on this thread carries these events as the dispatch's own start / stop (hipExtLaunchKernelGGL)
void time_next_launch(hipEvent_t start, hipEvent_t stop);
// profiling level 5: the next launch of a timed kernel (the same set, and k_build) on this thread leaves its first
// workgroup's start in slot[0] and its last workgroup's end in slot[STAMP_STRIDE] (s_memrealtime, 100 MHz ticks); the
// caller has set slot[0] = ~0 and slot[STAMP_STRIDE] = 0
constexpr int STAMP_STRIDE = 2048;
void stamp_next_launch(unsigned long long* slot);
bool timing_pending();   // still armed: the launch it was meant for did not happen
// per-device function attributes (dynamic LDS sizes) for the current device; the launchers do it lazily, a
// stream capture must not.  Returns the hipError_t of a failed hipFuncSetAttribute (0 = fine).
int prepare_kernels();

// test hook: C[m x n] = A[m x k] * B[n x k]^T on the MFMA tile path (all multiples of 128 / 16)
void launch_test_gemm_nt(const double* A, const double* B, double* C, int m, int n, int k, hipStream_t s);
// peak probe: `iters` dependent-free fp64 MFMAs per wave; returns nothing, timed by the caller
void launch_mfma_peak(double* sink, int blocks, int iters, hipStream_t s);

}  // namespace cugp
