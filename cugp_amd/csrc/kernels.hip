// kernels.hip -- hand-written gfx950 (CDNA4, wave64) kernels for the GP hot path.
//
// Path (reference file:line each kernel replaces):
//   k_build        SE+noise covariance          cpp_serial_gp/covkernel.cpp:64-102, cuda_scalingdist/cuda_gp.cu:232-281
//                  (every pass that evaluates the covariance function -- k_build, k_cross, k_predict_cov_finish, k_trace,
//                  k_trace_targets, k_predict_grad -- is one template <bool ARD, int KIND>: SE, Matern 3/2 and 5/2, each
//                  isotropic or with one length scale per dimension, from one body per pass)
//   potf2 / trsm / syrk_step / syrk_wide   blocked right-looking Cholesky (near window per step, far columns once per
//                  panel)   common/matrixops.cpp:68-108, cpp_matrixalgebra/blocked_cholesky.cpp:221-262,
//                  cuda_src/cuda_gp.cu:1237-1308
//   trtri_*        L^-1 by recursive doubling   common/matrixops.cpp:330-340, cuda_src/cuda_gp.cu:1854-1915 (TMI)
//   lauum          K^-1 = L^-T L^-1             common/matrixops.cpp:383-435, cuda_src/cuda_gp.cu:119-136
//   trmv / trace / finalize   alpha, y'K^-1 y, log|K|, gradient traces   covkernel.cpp:118-129,162-263
//   kcross / predict_*        predictive mean / variance                 covkernel.cpp:105-116,277-323
//
// Everything dense runs through ONE fp64 MFMA tile product (v_mfma_f64_16x16x4_f64):
//   C[128x128] = sum_k A[i][k] * B[j][k]   ("NT": both operands row-major with k contiguous)
// 4 waves per workgroup in a 2x2 grid, 64x64 per wave = 4x4 MFMA tiles (64 fp64 accumulators
// per lane), K staged 16 deep through LDS, double-buffered, global loads for stage t+1 in
// flight while stage t is multiplied.  LDS image: [k-pair plane, padded by 16 B][row][2 doubles]
// -- fragment reads are 256 contiguous bytes per 32 lanes (conflict-free ds_read_b64) at one
// per-lane base + immediate offsets (no address arithmetic in the loop: VALU issue costs MFMA
// issue on gfx950), staging writes (8 lanes = 8 planes of one row) land on 8 different 16-B slots
// (two rows of a 16-lane group overlap in 7 of them: 2-way, the ~5 % SQ_LDS_BANK_CONFLICT of the tile kernels;
// a 32-byte pad removes the overlap and changes no timing: the K loop does not wait for these writes).
//
// Matrices are npad x npad row-major with npad = ceil(n/128)*128; the padding of K is the
// identity, so every kernel works on whole tiles and the factor, inverse, log-determinant and
// traces of the leading n x n block are unchanged.
//
// Two kinds of device code, two kinds of file, told apart by the suffix; this file keeps only what all of them share.
//   *_device.h   what a host can emulate -- plain fp64 arithmetic, barriers and wave shuffles: the covariance helpers, the
//                ARD trace, the test-input gradient (cov_device.h), the append kernels (append_device.h) and their like.
//                The host checks (tools/*_host_check.cpp) compile the same headers behind tools/host_emul.h, 256 host
//                threads per workgroup under AddressSanitizer, before a new pass first meets a GPU.
//   *_gfx950.h   what needs the device -- MFMA, atomics, stamps, inline assembly -- by stage, and with each kernel its
//                LAUNCHER directly behind it: the grid a launcher builds and the blockIdx decoding of its kernel are one
//                contract.  tile_ (the product), eval_, chol_, inverse_ (one evaluation), predict_, dense_features_ and
//                sparse_gfx950.h, the last three the device side of predict.cpp, dense_features.cpp and sparse.cpp.
// An emulable header cannot hold a launcher (the host checks compile it): the launchers of its kernels stand in the
// *_gfx950.h of the same feature, which this file includes directly behind the emulable header.
// Every header states what must be declared where it is included, is included inside namespace cugp and includes nothing
// itself: this file holds every #include, one translation unit as before (the map, the order).
// A kernel's dynamic-LDS size is a named constant pinned to its number by a static_assert beside it;
// tools/kernel_resources.py reads the launch lines and those asserts.
#include "kernels.h"

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <cassert>
#include <cstdlib>

namespace cugp {

typedef double d4 __attribute__((ext_vector_type(4)));
typedef double d2 __attribute__((ext_vector_type(2)));

// A pointer read out of the experts' table (ExpertPtrs) is a generic pointer to the compiler: every access through it
// became a FLAT instruction, and flat loads count against lgkmcnt as well as vmcnt -- each wait for an LDS fragment
// read also waited for the global loads meant to stay in flight behind the MFMAs.  Round-tripping it through the
// global address space lets the address-space inference make it (and the select with the kernel argument) global.
template <class T>
__device__ __forceinline__ T* GP(T* p)
{
    // (through an integer: a plain generic -> global -> generic cast pair is folded away before the inference runs)
    return (T*)(__attribute__((address_space(1))) T*)(unsigned long long)p;
}

// Diagnostic build only (tools/wgtimes.hip, -DCUGP_WGTIMES): every workgroup of the kernels below leaves
// {kind | param << 8, start, end (s_memrealtime, 100 MHz), shader cycles lived (s_memtime)} in a side buffer -- when the workgroups of a launch were
// dispatched and how long each ran, i.e. whether a launch that took long beside other streams WAITED for workgroup
// slots or RAN slowly.  Nothing of it exists in the product build.
#ifdef CUGP_WGTIMES
constexpr unsigned WGT_CAP = 1u << 19;
__device__ unsigned long long g_wgt[4 * WGT_CAP];
__device__ unsigned g_wgt_n;
struct WgTimer {
    unsigned long long t0, c0, tag;
    __device__ __forceinline__ WgTimer(int kind, int param) : t0(__builtin_amdgcn_s_memrealtime()), c0(__builtin_amdgcn_s_memtime()), tag((unsigned long long)kind | (unsigned long long)param << 8) {}
    __device__ __forceinline__ ~WgTimer()
    {
        if (threadIdx.x == 0) {
            const unsigned i = atomicAdd(&g_wgt_n, 1u);
            if (i < WGT_CAP) {
                g_wgt[4 * i] = tag; g_wgt[4 * i + 1] = t0; g_wgt[4 * i + 2] = __builtin_amdgcn_s_memrealtime();
                g_wgt[4 * i + 3] = __builtin_amdgcn_s_memtime() - c0;          // shader cycles the workgroup lived
            }
        }
    }
};
#define WGT(name, kind, param) WgTimer name(kind, param)
void wgt_reset() { const unsigned z = 0; (void)hipMemcpyToSymbol(HIP_SYMBOL(g_wgt_n), &z, sizeof z); }
unsigned wgt_fetch(unsigned long long* out, unsigned cap)
{
    unsigned n = 0;
    (void)hipMemcpyFromSymbol(&n, HIP_SYMBOL(g_wgt_n), sizeof n);
    if (n > WGT_CAP) n = WGT_CAP;
    if (n > cap) n = cap;
    (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wgt), (size_t)n * 32);
    return n;
}
#else
#define WGT(name, kind, param)
#endif
enum { WGT_TRSM = 0, WGT_DIAGUPD = 1, WGT_POTF2 = 2, WGT_STEPTILE = 3, WGT_BORDER = 4, WGT_LAUUM = 5, WGT_LEVEL = 6,
       WGT_TRTRI_DIAG = 7, WGT_WIDE = 8 };

// Profiling level 5 (handle.h TimedLaunch): a timed launch carries a slot in a device buffer and every workgroup
// of it leaves its start in slot[0] (atomic min) and its end in slot[STAMP_STRIDE] (atomic max), on the chip-wide 100 MHz
// clock (s_memrealtime): launch duration = first workgroup's first instruction .. last workgroup's last, with NOTHING
// added to the stream -- the schedule is the untimed one (an event pair around a launch costs ~5 us of device time and
// brackets the dispatch gap in front of it; hipExtLaunchKernelGGL's own start / stop events still slow the evaluation
// by 3 %).  What rocprofv3 adds to this figure is the dispatch's ramp and drain, 1-3 us per launch.  slot == nullptr:
// one scalar compare per workgroup.
struct LaunchStamp {
    unsigned long long* p;
    // every: stamp one workgroup in `every` (and the last 64 of the grid): a launch of thousands of SHORT workgroups
    // (k_build: 8256 of ~2 us) would otherwise spend its time queueing 16k atomics on two words (+25 %)
    __device__ __forceinline__ explicit LaunchStamp(unsigned long long* p_, unsigned every = 1)
        : p((p_ && (every <= 1 || blockIdx.x % every == 0 || blockIdx.x + 64 >= gridDim.x)) ? p_ : nullptr)
    {
        // (workgroups are dispatched in index order: the launch's first instruction is one of the first workgroups')
        if (p && threadIdx.x == 0 && blockIdx.x < 64 && blockIdx.y == 0)
            __hip_atomic_fetch_min(p, (unsigned long long)__builtin_amdgcn_s_memrealtime(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __device__ __forceinline__ ~LaunchStamp()
    {
        if (p && threadIdx.x == 0)
            __hip_atomic_fetch_max(p + STAMP_STRIDE, (unsigned long long)__builtin_amdgcn_s_memrealtime(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};

// ------------------------------------------------------------------------------------------
// launch machinery: what every launcher needs above it
// ------------------------------------------------------------------------------------------
// Per-launch timing without extra packets on the stream (profiling level 4, handle.h TimedLaunch): the next launch
// of a timed kernel on this thread goes out through hipExtLaunchKernelGGL with a start / stop event pair, which take
// the dispatch's OWN begin / end timestamps -- what rocprofv3 --kernel-trace reports for it.  (An event pair recorded
// around the launch, level 3, brackets the ~6 us between the record in front of it and its first workgroup as well
// and costs ~5 us of device time per pair.)
thread_local hipEvent_t t_ev0 = nullptr, t_ev1 = nullptr;
thread_local unsigned long long* t_stamp = nullptr;        // level 5: the next timed launch's slot (LaunchStamp)
void time_next_launch(hipEvent_t start, hipEvent_t stop) { t_ev0 = start; t_ev1 = stop; }
void stamp_next_launch(unsigned long long* slot) { t_stamp = slot; }
bool timing_pending() { return t_ev0 != nullptr || t_stamp != nullptr; }
static inline unsigned long long* take_stamp() { unsigned long long* p = t_stamp; t_stamp = nullptr; return p; }
#define CUGP_LAUNCH(kernel, grid, block, lds, stream, ...)                                          \
    do {                                                                                            \
        if (t_ev0) {                                                                                \
            hipEvent_t e0_ = t_ev0, e1_ = t_ev1;                                                    \
            t_ev0 = t_ev1 = nullptr;                                                                \
            hipExtLaunchKernelGGL(kernel, grid, block, lds, stream, e0_, e1_, 0, __VA_ARGS__);      \
        } else {                                                                                    \
            hipLaunchKernelGGL(kernel, grid, block, lds, stream, __VA_ARGS__);                      \
        }                                                                                           \
    } while (0)

const int g_tune_init[TUNE_COUNT] = {768, 1200, 384, -1, 511, 1, 1, 1 << 20, 16, 500, 32, 1, 2100, 256, 1536, 0, 1 << 21, 1, 1, 0,
                                      1024, 64, 0};   // defaults chosen by interleaved A/B runs (tools/ab.py)
thread_local const int* t_tune = g_tune_init;

static inline int tri_count(int n) { return n * (n + 1) / 2; }

static inline bool is_ard(const CovFn& cf)
{
    assert(!cf.ard || cf.hd);
    return cf.ard;
}
// the ARD weights, which lie behind the hyper-scalars in device memory; null for an isotropic descriptor
static inline const double* ard_weights_ptr(const CovFn& cf) { return is_ard(cf) ? (const double*)(cf.hd + 1) : nullptr; }

// The one table of the covariance passes' instantiations: CUGP_COV_KERNEL(cf, k_<pass>) is k_<pass><ARD, KIND> of the
// descriptor (every instantiation of a pass has one type, so the selection is an expression).
// CUGP_COV_KERNEL3 is the table of the three families that have isotropic and ARD instantiations alike; the sparse
// passes, which no rational quadratic model launches, pick from it.  CUGP_COV_KERNEL adds <true, KERNEL_RQ> (an RQ
// descriptor is always ARD: its isotropic form ties the weights, it has no kernels of its own).
#define CUGP_COV_KERNEL(cf, stem) ((cf).kind == KERNEL_RQ ? (assert(is_ard(cf)), stem<true, KERNEL_RQ>) : CUGP_COV_KERNEL3(cf, stem))
#define CUGP_COV_KERNEL3(cf, stem)                                                                       \
    (is_ard(cf) ? ((cf).kind == KERNEL_MATERN32   ? stem<true, KERNEL_MATERN32>                          \
                   : (cf).kind == KERNEL_MATERN52 ? stem<true, KERNEL_MATERN52> : stem<true, KERNEL_SE>) \
                : ((cf).kind == KERNEL_MATERN32   ? stem<false, KERNEL_MATERN32>                         \
                   : (cf).kind == KERNEL_MATERN52 ? stem<false, KERNEL_MATERN52> : stem<false, KERNEL_SE>))
// defined at the end of this file (it names kernels of every stage); the launchers in the headers call it
static void set_big_lds();
// the workgroup's dynamic LDS in an emulable header (append_device.h: k_append_kinv's tile product; the host shim: a null pointer)
#define CUGP_DYN_LDS(name) extern __shared__ __attribute__((aligned(16))) char name[]

// ---- the device code, in dependency order (in front of each #include: what the header provides) ----
// BK, Geo, GEMM_LDS; bpos, opaque_tid, tile_stage_mma, tile_nt, plan_ksplit, acc_zero, tile_load / _store / _accum_store /
// _store_t; tile_nt8, tile_out8, acc_zero8; tile_tn; k_test_gemm, k_mfma_peak and their launchers
#include "tile_gfx950.h"
// tri_index, wave_sum; KT, DC, col4, sqdist_4x4, DivBy, ard_weights, div_prepare, div_by, matern_entry, ard_entry,
// ShapeArgs, shape_args, rq_entry, kernel_value; TGT_CHUNK, targets_outer_4x4; trace_ard_body; predict_grad_body, k_predict_grad, k_predict_grad_finish
#include "cov_device.h"
// k_predict_grad_batched, k_predict_grad_finish_batched, k_poe_reduce_grad: the product of experts' test-input gradient
#include "bcm_grad_device.h"
// k_predict_gemm, k_predict_cov, k_predict_cov_finish, k_zero_upper_diag, k_sample_finish, k_predict_finish,
// k_predict_finish_mv, k_poe_reduce, k_poe_reduce_mode, predict_cov_shape and every prediction launcher, those of the two
// emulable headers above included
#include "predict_gfx950.h"
// k_build, k_cross; k_trmv_*, k_copy_y_to_w, k_trsv_*; finalize_sums, trace_body, k_finalize, k_trace, k_finalize_ard; launchers
#include "eval_gfx950.h"
// the Cholesky: trap_index, MT .. POTF2_LDS, k_trsm_inv64, k_potf2, k_syrk_step, k_syrk_wide*, split_round and their launchers
#include "chol_gfx950.h"
// the inverse: k_trtri_level, k_trtri_border*, k_trtri_diag, k_trtri_block, k_lauum* and their launchers
#include "inverse_gfx950.h"
// appending observations (cugp_append): k_append_border, k_append_kinv (emulable; needs the tile product and CUGP_DYN_LDS)
#include "append_device.h"
// leave-one-out (cugp_loo): k_loo_point, k_loo_sum, k_loo_mirror_scale, k_loo_bsum, k_trace_loo, k_loo_finalize (emulable)
#include "loo_device.h"
// multi-target regression: k_targets_alpha, k_targets_alpha_batched, k_targets_mean, k_trace_targets, k_finalize_targets;
// k_loo_product; the launchers of these and of the two emulable headers above
#include "dense_features_gfx950.h"
// sparse variational GP regression on inducing points (cugp_sparse_*): k_sparse_gram_finish, k_sparse_form_b,
// k_sparse_transpose, k_trace_cross, k_sparse_predict_finish (emulable)
#include "sparse_device.h"
// the gradient with respect to the inducing inputs: k_trace_cross_z, k_trace_cross_z_finish (emulable)
#include "sparse_z_device.h"
// what reads the labels (the handle's own y as one target, or p targets): k_sparse_wty_targets and its finish, k_sparse_yy_,
// k_sparse_h_, k_sparse_weights_, k_sparse_scale_ and k_sparse_finalize_targets (emulable)
#include "sparse_targets_device.h"
// the input gradients of the sparse prediction: k_sparse_predict_diff (emulable)
#include "sparse_predict_device.h"
// the rows sharded over ranks: k_sparse_shard_reduce, k_sparse_shard_sums, k_sparse_finalize_sharded (emulable)
#include "sparse_shard_device.h"
// k_sparse_predict_cov, k_sparse_gram, sparse_shape, sparse_z_shape and every sparse launcher, those of the five emulable
// headers above included
#include "sparse_gfx950.h"

// hipFuncAttributeMaxDynamicSharedMemorySize applies to the CURRENT device only: one flag per device, and a
// failure is kept (the launch that follows would be rejected) and reported by prepare_kernels().
static unsigned long long g_attr_done = 0;              // bit per device ordinal (< 64)
static hipError_t g_attr_err = hipSuccess;
static void set_big_lds()
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev > 63) dev = 63;
    if (g_attr_done >> dev & 1ull) return;
    hipError_t e = hipSuccess;
    auto attr = [&](const void* f, int bytes) {
        const hipError_t r = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        if (r != hipSuccess && e == hipSuccess) e = r;
    };
    attr((const void*)k_potf2, POTF2_LDS);
    attr((const void*)k_syrk_step, STEP_LDS);
    attr((const void*)k_syrk_wide, GEMM_LDS);
    const void* gemm4[] = {(const void*)k_trtri_level<4>, (const void*)k_trtri_border<4>, (const void*)k_lauum<4>,
                           (const void*)k_test_gemm, (const void*)k_predict_cov<4>, (const void*)k_loo_product<4>,
                           (const void*)k_sparse_gram, (const void*)k_sparse_predict_cov<4>};
    for (const void* f : gemm4) attr(f, GEMM_LDS);
    for (const void* f : {(const void*)k_syrk_wide8, (const void*)k_lauum8, (const void*)k_trtri_border8}) attr(f, GEMM_LDS);
    attr((const void*)k_trtri_diag, TRTRI_LDS);
    attr((const void*)k_trtri_block, TRTRI_BLOCK_LDS);
    attr((const void*)k_trsm_inv64, TRSM_LDS);
    if (e != hipSuccess) { g_attr_err = e; return; }
    g_attr_done |= 1ull << dev;
}

int prepare_kernels() { set_big_lds(); return (int)g_attr_err; }

}  // namespace cugp
