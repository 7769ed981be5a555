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
// Two kinds of device code, two kinds of file, told apart by the suffix.
//   *_device.h   what a host can emulate -- plain fp64 arithmetic, barriers and wave shuffles: the covariance helpers, the
//                ARD trace, the test-input gradient (cov_device.h), the append kernels (append_device.h) and their like.
//                The host checks (tools/*_host_check.cpp) compile the same headers behind tools/host_emul.h, 256 host
//                threads per workgroup under AddressSanitizer, before a new pass first meets a GPU.
//   *_gfx950.h   what needs the device -- MFMA, atomics, stamps, inline assembly -- by stage, and with each kernel its
//                LAUNCHER in the same file: the grid a launcher builds and the blockIdx decoding of its kernel are one
//                contract.  So far the Cholesky (chol_gfx950.h) and the inverse (inverse_gfx950.h); the tile product, the
//                covariance, vector, finalize, prediction and feature kernels and their launchers are still in this file.
// Every header states what must be declared where it is included, is included inside namespace cugp and includes nothing
// itself: this file holds every #include, one translation unit as before.  A kernel's dynamic-LDS size is a named constant
// pinned to its number by a static_assert beside it; tools/kernel_resources.py reads the launch lines and those asserts.
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

// The one table of the covariance passes' instantiations: CUGP_COV_KERNEL(cf, k_<pass>) is k_<pass><ARD, KIND> of the
// descriptor (every instantiation of a pass has one type, so the selection is an expression).
#define CUGP_COV_KERNEL(cf, stem)                                                                        \
    (is_ard(cf) ? ((cf).kind == KERNEL_MATERN32   ? stem<true, KERNEL_MATERN32>                          \
                   : (cf).kind == KERNEL_MATERN52 ? stem<true, KERNEL_MATERN52> : stem<true, KERNEL_SE>) \
                : ((cf).kind == KERNEL_MATERN32   ? stem<false, KERNEL_MATERN32>                         \
                   : (cf).kind == KERNEL_MATERN52 ? stem<false, KERNEL_MATERN52> : stem<false, KERNEL_SE>))
// defined with the launchers at the end of this file (it names kernels of every stage); the launchers in the headers call it
static void set_big_lds();

// tri_index, wave_sum; KT, DC, col4, sqdist_4x4, DivBy, ard_weights, div_prepare, div_by, matern_entry, ard_entry,
// kernel_value; TGT_CHUNK, targets_outer_4x4; trace_ard_body; predict_grad_body, k_predict_grad, k_predict_grad_finish.
// Needs kernels.h, d2, d4 and GP (above) and nothing below.
#include "cov_device.h"
// k_predict_grad_batched, k_predict_grad_finish_batched, k_poe_reduce_grad: the product of experts' test-input gradient
#include "bcm_grad_device.h"

// ------------------------------------------------------------------------------------------
// fp64 MFMA tile product
// ------------------------------------------------------------------------------------------
constexpr int BK = 16;                       // k depth per LDS stage
// geometry of a tile product whose waves hold WM x WM MFMA tiles each (block edge 32*WM: 128 or 64)
template <int WM> struct Geo {
    static constexpr int BT = 32 * WM;               // block tile edge
    static constexpr int PLANE = BT * 16 + 16;       // bytes per k-pair plane (BT rows x 2 doubles) + 16 B pad:
                                                     // 8 staging lanes (8 planes of one row) hit 8 different 16-B slots
    static constexpr int OPER = (BK / 2) * PLANE;    // bytes per operand per stage
    static constexpr int STAGE = 2 * OPER;           // A + B
    static constexpr int LDS = 2 * STAGE;            // double buffered: 66048 B (WM=4, dynamic LDS) / 33280 B (WM=2)
};
constexpr int GEMM_LDS = Geo<4>::LDS;
static_assert(GEMM_LDS == 66048, "dynamic LDS of a 128x128 tile product (tools/kernel_resources.py reads this line)");
static_assert(Geo<2>::LDS == 33280, "dynamic LDS of a 64x64 tile product");

// diagonal-block kernels work on 16x16 micro tiles (one MFMA tile)
constexpr int MT = 16;                             // micro tile (one MFMA tile)
constexpr int MTS = MT * (MT + 1);                 // doubles per LDS micro tile, rows padded to 17
constexpr int NMT = TILE / MT;                     // 8 micro tiles per edge
constexpr int NLT = NMT * (NMT + 1) / 2;           // 36 lower micro tiles
constexpr int POTF2_LDS = (NLT * MTS + TILE) * 8;  // tiles + 1/L_ii  = 79360 B
static_assert(POTF2_LDS == 79360, "dynamic LDS of the diagonal-block Cholesky");

// B-operand rows are stored permuted inside each wave's column range so that MFMA tiles n = 2p, 2p+1
// of a wave produce ADJACENT output columns in one lane (16-byte global accesses in the epilogue)
// while the fragment reads stay 256 contiguous bytes: tile row R -> LDS position bpos(R).
template <int WM>
__device__ __forceinline__ int bpos(int R)
{
    const int q = R & (16 * WM - 1);
    return (R - q) + (((q >> 5) * 2 + (q & 1)) * 16) + ((q & 31) >> 1);
}

// threadIdx.x behind an optimisation barrier: inside a persistent tile loop (k_syrk_wide) the compiler would
// otherwise hoist every per-thread address of the tile product out of the loop and keep them all live across
// the accumulator load / store, which overflows the 256-register budget of 2 workgroups per CU into scratch.
__device__ __forceinline__ int opaque_tid()
{
    int t = threadIdx.x;
    asm volatile("" : "+v"(t));
    return t;
}

// One K stage (16 deep) of MFMAs out of LDS buffer `cur`.  Measured on gfx950: every VALU instruction a wave
// issues between fp64 MFMAs costs MFMA issue time (pure MFMA stream 74 TF/s, +1 VALU per MFMA 62, +4: 55),
// so the loop body carries NO address arithmetic: fragment addresses are one per-lane base + immediates.
template <int WM>
__device__ __forceinline__ void tile_stage_mma(const char* __restrict__ cur, int abase, int bbase,
                                               d4 (&acc)[WM][WM])
{
    typedef Geo<WM> G;
#pragma unroll
    for (int kk = 0; kk < BK / 4; kk++) {
        double a[WM], b[WM];
#pragma unroll
        for (int m = 0; m < WM; m++) {
            a[m] = *(const double*)(cur + abase + kk * 2 * G::PLANE + m * 256);
            b[m] = *(const double*)(cur + bbase + kk * 2 * G::PLANE + m * 256);
        }
#pragma unroll
        for (int m = 0; m < WM; m++)
#pragma unroll
            for (int n = 0; n < WM; n++)
                acc[m][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[m], b[n], acc[m][n], 0, 0, 0);
    }
}

// acc[m][n] += (NEGA ? -1 : 1) * A(i0.., kbeg..kend) * B(j0.., kbeg..kend)^T ; Ag -> A[i0][0], Bg -> B[j0][0];
// kbeg, kend multiples of BK.  All 256 threads must call (barriers inside).  WM (deduced from acc) is the
// number of 16x16 MFMA tiles per wave per dimension: 4 -> 128x128 block, 2 -> 64x64 block.
// LDS image per operand and stage: [k-pair plane (padded by 16 B)][row][2 doubles].
#ifdef CUGP_TILE_STAMPS   // diagnostic build only (tools/gemm_k_bench.hip): where a tile's time goes
__device__ unsigned long long g_tile_stamps[64];
__device__ int g_tile_stamp_on;                          // stamps inside tile_nt only while this is set
#define TILE_STAMP(i)                                                              \
    do {                                                                           \
        if (threadIdx.x == 0 && blockIdx.x == 200) {                               \
            g_tile_stamps[i] = __builtin_readcyclecounter();                       \
            g_tile_stamps[32 + i] = __builtin_amdgcn_s_memrealtime();              \
        }                                                                          \
    } while (0)
#else
#define TILE_STAMP(i)
#endif

template <bool NEGA, int WM>
__device__ __forceinline__ void tile_nt(const double* __restrict__ Ag, int lda, const double* __restrict__ Bg,
                                        int ldb, int kbeg, int kend, d4 (&acc)[WM][WM], char* smem)
{
    typedef Geo<WM> G;
    const int t = opaque_tid();
    const int lane = t & 63, wave = t >> 6;
    const int wr = wave >> 1, wc = wave & 1;

    // staging map: WM chunks of 16 B per operand per thread; 8 consecutive lanes cover one row's 128 B
    const int srow = t >> 3, skp = t & 7;                 // + 32 rows per q
    const double* ag = Ag + (size_t)srow * lda + 2 * skp;
    const double* bg = Bg + (size_t)srow * ldb + 2 * skp;
    d2 ra[WM], rb[WM];
    int wa[WM], wb[WM];                                   // LDS byte offsets of my staging chunks
#pragma unroll
    for (int q = 0; q < WM; q++) {
        wa[q] = skp * G::PLANE + (srow + 32 * q) * 16;
        wb[q] = G::OPER + skp * G::PLANE + bpos<WM>(srow + 32 * q) * 16;
    }
    // fragment bases: lane (fr = lane & 15, fk = lane >> 4) reads row fr (+16 m) of k-pair plane (2 kk + fk/2)
    const int fr = lane & 15, fk = lane >> 4;
    const int abase = (fk >> 1) * G::PLANE + (wr * 16 * WM + fr) * 16 + (fk & 1) * 8;
    const int bbase = G::OPER + (fk >> 1) * G::PLANE + (wc * 16 * WM + fr) * 16 + (fk & 1) * 8;

    const int nk = (kend - kbeg) / BK;
    if (nk <= 0) return;

#pragma unroll
    for (int q = 0; q < WM; q++) {
        ra[q] = *(const d2*)(ag + (size_t)(32 * q) * lda + kbeg);
        rb[q] = *(const d2*)(bg + (size_t)(32 * q) * ldb + kbeg);
    }
#pragma unroll
    for (int q = 0; q < WM; q++) {
        *(d2*)(smem + wa[q]) = NEGA ? -ra[q] : ra[q];
        *(d2*)(smem + wb[q]) = rb[q];
    }
    __syncthreads();
#ifdef CUGP_TILE_STAMPS
    if (g_tile_stamp_on) TILE_STAMP(1);
#endif

    // two stages per trip so both LDS buffers are compile-time offsets (no address arithmetic in the loop)
#define CUGP_STAGE(HALF, MORE, KNEXT)                                                              \
    do {                                                                                           \
        const char* cur_ = smem + (HALF) * G::STAGE;                                               \
        char* nxt_ = smem + (1 - (HALF)) * G::STAGE;                                               \
        const bool more_ = (MORE);                                                                 \
        if (more_) {                                                                               \
            const int k_ = (KNEXT);                                                                \
            _Pragma("unroll") for (int q = 0; q < WM; q++) {                                       \
                ra[q] = *(const d2*)(ag + (size_t)(32 * q) * lda + k_);                            \
                rb[q] = *(const d2*)(bg + (size_t)(32 * q) * ldb + k_);                            \
            }                                                                                      \
        }                                                                                          \
        tile_stage_mma<WM>(cur_, abase, bbase, acc);                                               \
        if (more_) {                                                                               \
            _Pragma("unroll") for (int q = 0; q < WM; q++) {                                       \
                *(d2*)(nxt_ + wa[q]) = NEGA ? -ra[q] : ra[q];                                      \
                *(d2*)(nxt_ + wb[q]) = rb[q];                                                      \
            }                                                                                      \
        }                                                                                          \
        __syncthreads();                                                                           \
    } while (0)

    int kt = 0;
    for (; kt + 1 < nk; kt += 2) {
        CUGP_STAGE(0, true, kbeg + (kt + 1) * BK);
        CUGP_STAGE(1, kt + 2 < nk, kbeg + (kt + 2) * BK);
    }
    if (kt < nk) CUGP_STAGE(0, false, 0);
#undef CUGP_STAGE
}

template <int WM>
__device__ __forceinline__ void acc_zero(d4 (&acc)[WM][WM])
{
#pragma unroll
    for (int m = 0; m < WM; m++)
#pragma unroll
        for (int n = 0; n < WM; n++) acc[m][n] = (d4){0.0, 0.0, 0.0, 0.0};
}

// accumulator element (m,n,r) of this lane is C[row][col]: f64 16x16x4 C/D map (col = lane&15,
// row = (lane>>4) + 4*r inside a 16x16 tile) composed with the B-row permutation above, so tiles
// n = 2p and 2p+1 hold columns 2*(lane&15) and 2*(lane&15)+1 of the 32-column group p.
#define ACC_ROW(m, r) (wr * 16 * WM + (m) * 16 + (lane >> 4) + 4 * (r))
#define ACC_COL2(np) (wc * 16 * WM + (np) * 32 + 2 * (lane & 15))

// acc = C   (the K loop then accumulates straight onto it: no read-modify-write epilogue).  The product form of rounds
// 1-4; since round 5 the library's kernels use tile_accum_store below (tools/wide_bench.hip keeps both side by side).
// STREAM: the tile is touched once per launch -> non-temporal accesses keep the shared operand panels in L2
template <bool STREAM = false, int WM>
__device__ __forceinline__ void tile_load(const double* __restrict__ C, int ldc, d4 (&acc)[WM][WM])
{
    const int tid = opaque_tid();
    const int lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
#pragma unroll
    for (int m = 0; m < WM; m++)
#pragma unroll
        for (int r = 0; r < 4; r++)
#pragma unroll
            for (int np = 0; np < WM / 2; np++) {
                const d2* src = (const d2*)(C + (size_t)ACC_ROW(m, r) * ldc + ACC_COL2(np));
                const d2 v = STREAM ? __builtin_nontemporal_load(src) : *src;
                acc[m][2 * np][r] = v[0];
                acc[m][2 * np + 1][r] = v[1];
            }
}

// C = alpha * acc
template <bool STREAM = false, int WM>
__device__ __forceinline__ void tile_store(double* __restrict__ C, int ldc, const d4 (&acc)[WM][WM], double alpha)
{
    const int tid = opaque_tid();
    const int lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
#pragma unroll
    for (int m = 0; m < WM; m++)
#pragma unroll
        for (int r = 0; r < 4; r++)
#pragma unroll
            for (int np = 0; np < WM / 2; np++)
            {
                d2* dst = (d2*)(C + (size_t)ACC_ROW(m, r) * ldc + ACC_COL2(np));
                const d2 v = (d2){alpha * acc[m][2 * np][r], alpha * acc[m][2 * np + 1][r]};
                if (STREAM) __builtin_nontemporal_store(v, dst);
                else *dst = v;
            }
}

// C += SIGN * acc, the C tile read in the EPILOGUE (round 5).  The accumulators start from zero and the K loop runs
// first; then one row group m of the wave at a time -- 16 doubles per lane in flight -- is read, updated and written.
// The product form (acc = C in front of the K loop, tile_load) held the first MFMA back until all 128 KB of the tile
// had arrived, in a burst with the launch's other workgroups and with the first operand stage; here the K loop starts
// at once and the C traffic of a workgroup overlaps the K loop of the other workgroup on its CU.  Measured
// (tools/wide_bench.hip, trailing-update form, 1596 tiles): K = 256 52.8 -> 54.7 TF/s, K = 512 56.4 -> 59.3, K = 1024
// 59.0 -> 61.4, K = 2048 54.4 -> 56.3, K = 128 44.6 -> 45.2; with neither read nor write 61.4 / 62.5 / 62.9 / 56.9 /
// 59.2.  Plain accesses: non-temporal ones lost 1-3 TF/s in this form.  One more rounding per entry and pass than the
// product form (the sum is formed first, then added), for every kernel alike.
template <int SIGN, int WM>
__device__ __forceinline__ void tile_accum_store(double* __restrict__ C, int ldc, const d4 (&acc)[WM][WM])
{
    const int tid = opaque_tid();
    const int lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
#pragma unroll
    for (int m = 0; m < WM; m++) {
        d2 v[4][WM / 2];
#pragma unroll
        for (int r = 0; r < 4; r++)
#pragma unroll
            for (int np = 0; np < WM / 2; np++)
                v[r][np] = *(const d2*)(C + (size_t)ACC_ROW(m, r) * ldc + ACC_COL2(np));
#pragma unroll
        for (int r = 0; r < 4; r++)
#pragma unroll
            for (int np = 0; np < WM / 2; np++) {
                d2* dst = (d2*)(C + (size_t)ACC_ROW(m, r) * ldc + ACC_COL2(np));
                if (SIGN > 0) *dst = (d2){v[r][np][0] + acc[m][2 * np][r], v[r][np][1] + acc[m][2 * np + 1][r]};
                else *dst = (d2){v[r][np][0] - acc[m][2 * np][r], v[r][np][1] - acc[m][2 * np + 1][r]};
            }
    }
}

// Ct[col][row] = alpha*acc  (transposed store).  The tile is turned through LDS (free after the K loop)
// in two halves of 16*WM rows so that global stores are whole runs of that many doubles; the LDS image
// [col][16*WM rows] is XOR-swizzled on the row index so the accumulator-layout writes do not pile onto
// one bank.  All 256 threads must call.
template <int WM>
__device__ __forceinline__ void tile_store_t(double* __restrict__ Ct, int ldc, const d4 (&acc)[WM][WM], double alpha,
                                             char* smem)
{
    constexpr int RH = 16 * WM, BT = 32 * WM;            // rows per half, block edge
    constexpr int LPC = RH / 2, CPP = 256 / LPC;         // lanes per column-row, column-rows per pass
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    double* sd = (double*)smem;
#pragma unroll
    for (int h = 0; h < 2; h++) {
        __syncthreads();
        if (wr == h) {
#pragma unroll
            for (int m = 0; m < WM; m++)
#pragma unroll
                for (int n = 0; n < WM; n++)
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const int col = ACC_COL2(n >> 1) + (n & 1);
                        const int rr = m * 16 + (lane >> 4) + 4 * r;
                        sd[col * RH + (rr ^ ((col >> 1) & 15))] = alpha * acc[m][n][r];
                    }
        }
        __syncthreads();
        const int rr = (t % LPC) * 2;
#pragma unroll
        for (int pass = 0; pass < BT / CPP; pass++) {
            const int col = pass * CPP + t / LPC;
            const int sw = (col >> 1) & 15;
            const d2 v = (d2){sd[col * RH + (rr ^ sw)], sd[col * RH + ((rr + 1) ^ sw)]};
            *(d2*)(Ct + (size_t)col * ldc + h * RH + rr) = v;
        }
    }
}

// ---- the 128x128 product's second geometry: 8 waves (TUNE_WAVES8) ----
// 512 threads, waves 4 x 2, 32 x 64 outputs per wave (2 x 4 MFMA tiles, 32 accumulators), the LDS image of the 4-wave
// product (Geo<4>, the same dynamic LDS).  Two such workgroups put FOUR waves on every SIMD, so while one workgroup is
// in its prologue or epilogue the other still has two waves per SIMD issuing MFMAs.  Every output entry is the same
// chain of MFMA accumulations over k as in the 4-wave product and meets C in the same epilogue expression: the same
// bits.  Used by the uniform-K launches (k_syrk_wide8, k_lauum8, k_trtri_border8: bordering step 1); the 64x64 quarters
// of a launch's last round (split_round) stay on four waves, in a launch of their own behind it (k_*_rest).
template <bool NEGA>
__device__ __forceinline__ void tile_nt8(const double* __restrict__ Ag, int lda, const double* __restrict__ Bg, int ldb,
                                         int kbeg, int kend, d4 (&acc)[2][4], char* smem)
{
    typedef Geo<4> G;
    const int t = opaque_tid();
    const int lane = t & 63, wave = t >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int srow = t >> 3, skp = t & 7;                 // 64 rows per pass, 2 passes
    const double* ag = Ag + (size_t)srow * lda + 2 * skp;
    const double* bg = Bg + (size_t)srow * ldb + 2 * skp;
    d2 ra[2], rb[2];
    int wa[2], wb[2];
#pragma unroll
    for (int q = 0; q < 2; q++) {
        wa[q] = skp * G::PLANE + (srow + 64 * q) * 16;
        wb[q] = G::OPER + skp * G::PLANE + bpos<4>(srow + 64 * q) * 16;
    }
    const int fr = lane & 15, fk = lane >> 4;
    const int abase = (fk >> 1) * G::PLANE + (wr * 32 + fr) * 16 + (fk & 1) * 8;
    const int bbase = G::OPER + (fk >> 1) * G::PLANE + (wc * 64 + fr) * 16 + (fk & 1) * 8;
    const int nk = (kend - kbeg) / BK;
    if (nk <= 0) return;
#pragma unroll
    for (int q = 0; q < 2; q++) {
        ra[q] = *(const d2*)(ag + (size_t)(64 * q) * lda + kbeg);
        rb[q] = *(const d2*)(bg + (size_t)(64 * q) * ldb + kbeg);
    }
#pragma unroll
    for (int q = 0; q < 2; q++) {
        *(d2*)(smem + wa[q]) = NEGA ? -ra[q] : ra[q];
        *(d2*)(smem + wb[q]) = rb[q];
    }
    __syncthreads();
#define CUGP_STAGE8(HALF, MORE, KNEXT)                                                              \
    do {                                                                                            \
        const char* cur_ = smem + (HALF) * G::STAGE;                                                \
        char* nxt_ = smem + (1 - (HALF)) * G::STAGE;                                                \
        const bool more_ = (MORE);                                                                  \
        if (more_) {                                                                                \
            const int k_ = (KNEXT);                                                                 \
            _Pragma("unroll") for (int q = 0; q < 2; q++) {                                         \
                ra[q] = *(const d2*)(ag + (size_t)(64 * q) * lda + k_);                             \
                rb[q] = *(const d2*)(bg + (size_t)(64 * q) * ldb + k_);                             \
            }                                                                                       \
        }                                                                                           \
        _Pragma("unroll") for (int kk = 0; kk < BK / 4; kk++) {                                     \
            double a[2], b[4];                                                                      \
            _Pragma("unroll") for (int m = 0; m < 2; m++) a[m] = *(const double*)(cur_ + abase + kk * 2 * G::PLANE + m * 256); \
            _Pragma("unroll") for (int n = 0; n < 4; n++) b[n] = *(const double*)(cur_ + bbase + kk * 2 * G::PLANE + n * 256); \
            _Pragma("unroll") for (int m = 0; m < 2; m++)                                           \
                _Pragma("unroll") for (int n = 0; n < 4; n++)                                       \
                    acc[m][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[m], b[n], acc[m][n], 0, 0, 0); \
        }                                                                                           \
        if (more_) {                                                                                \
            _Pragma("unroll") for (int q = 0; q < 2; q++) {                                         \
                *(d2*)(nxt_ + wa[q]) = NEGA ? -ra[q] : ra[q];                                       \
                *(d2*)(nxt_ + wb[q]) = rb[q];                                                       \
            }                                                                                       \
        }                                                                                           \
        __syncthreads();                                                                            \
    } while (0)
    int kt = 0;
    for (; kt + 1 < nk; kt += 2) {
        CUGP_STAGE8(0, true, kbeg + (kt + 1) * BK);
        CUGP_STAGE8(1, kt + 2 < nk, kbeg + (kt + 2) * BK);
    }
    if (kt < nk) CUGP_STAGE8(0, false, 0);
#undef CUGP_STAGE8
}

// the 8-wave epilogues.  SIGN 0: C = acc (tile_store with alpha = 1); +1 / -1: C += / -= acc, the C tile read here, one
// row group of the wave at a time (tile_accum_store)
template <int SIGN>
__device__ __forceinline__ void tile_out8(double* __restrict__ C, int ldc, const d4 (&acc)[2][4])
{
    const int tid = opaque_tid();
    const int lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
#pragma unroll
    for (int m = 0; m < 2; m++) {
        double* const c0 = C + (size_t)(wr * 32 + m * 16 + (lane >> 4)) * ldc + wc * 64 + 2 * (lane & 15);
        d2 v[4][2];
        if (SIGN != 0) {
#pragma unroll
            for (int r = 0; r < 4; r++)
#pragma unroll
                for (int np = 0; np < 2; np++) v[r][np] = *(const d2*)(c0 + (size_t)(4 * r) * ldc + np * 32);
        }
#pragma unroll
        for (int r = 0; r < 4; r++)
#pragma unroll
            for (int np = 0; np < 2; np++) {
                d2* dst = (d2*)(c0 + (size_t)(4 * r) * ldc + np * 32);
                if (SIGN == 0) *dst = (d2){acc[m][2 * np][r], acc[m][2 * np + 1][r]};
                else if (SIGN > 0) *dst = (d2){v[r][np][0] + acc[m][2 * np][r], v[r][np][1] + acc[m][2 * np + 1][r]};
                else *dst = (d2){v[r][np][0] - acc[m][2 * np][r], v[r][np][1] - acc[m][2 * np + 1][r]};
            }
    }
}

__device__ __forceinline__ void acc_zero8(d4 (&acc)[2][4])
{
#pragma unroll
    for (int m = 0; m < 2; m++)
#pragma unroll
        for (int n = 0; n < 4; n++) acc[m][n] = (d4){0.0, 0.0, 0.0, 0.0};
}

// ---- prediction: W[t][i] = sum_{k <= i} Ks[t][k] * T[i][k] ----
// T = L^-1 is lower triangular: row tile i needs k < (i + 1) * tile only, so the work per output tile grows linearly
// with i.  Rounds 1-4 gave every 128x128 output tile a workgroup of its own: 512 workgroups for 1000 test points at
// N = 8192, one round of the chip, whose duration is the LONGEST tile's (K = 8192) while the average is half of it --
// 45 TF/s = 0.58 of peak.  Round 5: 64x64 output tiles in PAIRS (row tile p with row tile n64 - 1 - p, the long one
// first): every workgroup does K = (n64 + 1) * 64 in all, 1024 equal workgroups, four per CU.  The same per-element
// sums in the same order (the k range of a tile ends at its own diagonal; what the 128-tile form added beyond it were
// exact zeros of T): bit-identical results.
// bt (batched): blockIdx.y selects the expert -- T from its table entry, Ks and W its [ntt64 * 64][ld] slices
__global__ __launch_bounds__(256, 2) void k_predict_gemm(const double* __restrict__ Ks, const double* __restrict__ T,
                                                         double* __restrict__ W, int ld, int ntt64, int n64,
                                                         unsigned long long* stamp, const ExpertPtrs* __restrict__ bt)
{
    LaunchStamp stamp_(stamp);
    if (bt) {
        const size_t off = (size_t)blockIdx.y * ntt64 * 64 * ld;
        T = GP(bt[blockIdx.y].T); Ks += off; W += off;
    }
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tt = blockIdx.x % ntt64, p = blockIdx.x / ntt64;
#pragma unroll 1
    for (int h = 0; h < 2; h++) {
        const int ti = h == 0 ? n64 - 1 - p : p;
        d4 acc[2][2];
        acc_zero(acc);
        tile_nt<false>(Ks + (size_t)tt * 64 * ld, ld, T + (size_t)ti * 64 * ld, ld, 0, (ti + 1) * 64, acc, smem);
        tile_store(W + (size_t)tt * 64 * ld + ti * 64, ld, acc, 1.0);
    }
}

// ---- plain NT product for tests ----
__global__ __launch_bounds__(256, 2) void k_test_gemm(const double* __restrict__ A, const double* __restrict__ B,
                                                      double* __restrict__ C, int n, int k, int mt)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int ti = blockIdx.x % mt, tj = blockIdx.x / mt;
    d4 acc[4][4];
    acc_zero(acc);
    tile_nt<false>(A + (size_t)ti * TILE * k, k, B + (size_t)tj * TILE * k, k, 0, k, acc, smem);
    tile_store(C + (size_t)ti * TILE * n + tj * TILE, n, acc, 1.0);
}

__global__ __launch_bounds__(256) void k_mfma_peak(double* sink, int iters)
{
    d4 acc[8];
    const double a = 1.0 + threadIdx.x * 1e-9, b = 1.0 - threadIdx.x * 1e-9;
#pragma unroll
    for (int i = 0; i < 8; i++) acc[i] = (d4){0.0, 0.0, 0.0, 0.0};
    for (int it = 0; it < iters; it++) {
#pragma unroll
        for (int i = 0; i < 8; i++) acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[i], 0, 0, 0);
    }
    double s = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) s += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
    if (s == 12345.678) sink[blockIdx.x * 256 + threadIdx.x] = s;
}

// ------------------------------------------------------------------------------------------
// SE covariance build: 64x64 tile per 256-thread workgroup, 4x4 outputs per thread, X tiles in LDS
// (the tile geometry KT, DC, col4, the squared distances and the per-entry formulas: cov_device.h)
// ------------------------------------------------------------------------------------------
// The passes that evaluate the covariance function are ONE kernel template each, k_<pass><ARD, KIND>, with one argument
// list: the hyper-scalars by value (h) and in device memory (hd).  Isotropic: hd is optional -- when given it is read
// INSTEAD of h, so that a captured graph of the evaluation is replayed with new hyper-parameters by refreshing that one
// buffer instead of every kernel's arguments (build and trace; the other passes take h).  ARD: hd is mandatory, h is
// ignored, the d per-dimension weights lie behind the hyper-scalars and ell_sq is not read: K = sf2 exp(-acc / 2) (or the
// Matern entry) of the weighted squared distance, no division.  cov_kernel (at the launchers) maps a CovFn to the instantiation.
//
// k_build: lower 64x64 tiles of K (+ mirror when full == 1); full == 2 (isotropic SE only): the squared-distance
// intermediate of launch_sqdist.  Batched experts, ticket zeroing, device-resident hyper-scalars and stamps in every
// instantiation.
template <bool ARD, int KIND>
__device__ __forceinline__ void build_body(const double* __restrict__ X, int n, int d, int npad,
                                           HyperScalars h_arg, const HyperScalars* __restrict__ hd,
                                           double* __restrict__ K, int full, unsigned* __restrict__ tickets,
                                           const ExpertPtrs* __restrict__ bt, unsigned long long* stamp)
{
    LaunchStamp stamp_(stamp, 16);
    if (bt) {
        X = GP(bt[blockIdx.y].X); n = bt[blockIdx.y].n; K = GP(bt[blockIdx.y].A);
        if (tickets) tickets = GP(bt[blockIdx.y].tickets);
    }
    // tickets (when given): the factorisation's per-step arrival counters, zeroed here instead of by a memset node in
    // front of the factorisation (one launch boundary less on a chain that small matrices are bound by)
    // (2 per tile row: [0, nt) the step tickets of k_syrk_step, [nt, 2 nt) the stage counters of k_trtri_block; [2 nt]: the
    //  arrival counter of k_trace's fused finalize)
    if (tickets && blockIdx.x == 0)
        for (int i = threadIdx.x; i < ticket_count(npad / TILE); i += 256) tickets[i] = 0u;
    const HyperScalars h = (ARD || hd) ? *hd : h_arg;
    __shared__ double xs[KT][DC + 1], ys[KT][DC + 1];
    __shared__ double ws[DC];
    int ti, tj;
    tri_index(blockIdx.x, ti, tj);
    const int i0 = ti * KT, j0 = tj * KT;
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    double d2v[4][4];
    sqdist_4x4<ARD>(X, X, n, n, d, i0, j0, xs, ys, d2v, ARD ? ard_weights(hd) : nullptr, ws);
    double out[4][4];
    const DivBy dl = div_prepare(h.ell_sq);
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const int i = i0 + ty * 4 + a, j = j0 + col4(tx, b);
            const bool in = i < n && j < n;
            double v;
            if (!ARD && full == 2) {
                v = (i == j) ? 0.0 : div_by(d2v[a][b], dl);    // covkernel.cpp:143-151 (squared distance / c)
            } else {
                v = kernel_value<ARD, KIND>(d2v[a][b], dl, h.signal_var);   // covkernel.cpp:89
                if (i == j) v += h.noise_var;                            // covkernel.cpp:93-94
            }
            out[a][b] = in ? v : ((i == j) ? 1.0 : 0.0);                // identity padding
        }
#pragma unroll
    for (int a = 0; a < 4; a++) {
        double* p = K + (size_t)(i0 + ty * 4 + a) * npad + j0 + tx * 2;
        *(d2*)p = (d2){out[a][0], out[a][1]};
        *(d2*)(p + 32) = (d2){out[a][2], out[a][3]};
    }
    if (full && ti != tj) {
#pragma unroll
        for (int b = 0; b < 4; b++) {
            double* p = K + (size_t)(j0 + col4(tx, b)) * npad + i0 + ty * 4;
            *(d2*)p = (d2){out[0][b], out[1][b]};
            *(d2*)(p + 2) = (d2){out[2][b], out[3][b]};
        }
    }
}

template <bool ARD, int KIND>
__global__ __launch_bounds__(256) void k_build(const double* __restrict__ X, int n, int d, int npad,
                                               HyperScalars h_arg, const HyperScalars* __restrict__ hd,
                                               double* __restrict__ K, int full, unsigned* __restrict__ tickets,
                                               const ExpertPtrs* __restrict__ bt, unsigned long long* stamp)
{
    build_body<ARD, KIND>(X, n, d, npad, h_arg, hd, K, full, tickets, bt, stamp);
}

// k_cross: Ks[t][i] = k(xt_t, x_i) (no noise, covkernel.cpp:105-116); zero padding
// bt (batched): blockIdx.y selects the expert -- X, n from its table entry, Ks = the expert's [ntpad][npad] slice
template <bool ARD, int KIND>
__device__ __forceinline__ void cross_body(const double* __restrict__ X, int n, int d, int npad,
                                           const double* __restrict__ Xt, int nt, int ntpad, const HyperScalars& h,
                                           const double* __restrict__ wts,
                                           double* __restrict__ Ks, const ExpertPtrs* __restrict__ bt)
{
    if (bt) {
        X = GP(bt[blockIdx.y].X); n = bt[blockIdx.y].n;
        Ks += (size_t)blockIdx.y * ntpad * npad;
    }
    __shared__ double xs[KT][DC + 1], ys[KT][DC + 1];
    const int tiles_i = npad / KT;
    const int tt = blockIdx.x / tiles_i, ti = blockIdx.x % tiles_i;
    const int t0 = tt * KT, i0 = ti * KT;
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    double d2v[4][4];
    // the reference subtracts X[i] - xtest (covkernel.cpp:112); squares are sign-independent but keep the order
    __shared__ double ws[DC];
    sqdist_4x4<ARD>(Xt, X, nt, n, d, t0, i0, xs, ys, d2v, wts, ws);
    const DivBy dl = div_prepare(h.ell_sq);
#pragma unroll
    for (int a = 0; a < 4; a++) {
        const int tr = t0 + ty * 4 + a;
        double o[4];
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const int i = i0 + col4(tx, b);
            o[b] = (tr < nt && i < n) ? kernel_value<ARD, KIND>(d2v[a][b], dl, h.signal_var) : 0.0;
        }
        double* p = Ks + (size_t)tr * npad + i0 + tx * 2;
        *(d2*)p = (d2){o[0], o[1]};
        *(d2*)(p + 32) = (d2){o[2], o[3]};
    }
}

template <bool ARD, int KIND>
__global__ __launch_bounds__(256) void k_cross(const double* __restrict__ X, int n, int d, int npad,
                                               const double* __restrict__ Xt, int nt, int ntpad, HyperScalars h_arg,
                                               double* __restrict__ Ks, const ExpertPtrs* __restrict__ bt,
                                               const HyperScalars* __restrict__ hd)
{
    cross_body<ARD, KIND>(X, n, d, npad, Xt, nt, ntpad, ARD ? *hd : h_arg, ARD ? ard_weights(hd) : nullptr, Ks, bt);
}

// ---- joint predictive covariance (cugp_predict_cov): Sigma = k(Xt,Xt) (+ sn2 I) - W W^T, W = Ks L^-T ----
// Product: P = W W^T over the lower BT-tiles of the nt x nt result.  W ([ntpad][ld], k_predict_gemm's output) is exactly
// zero in its columns >= n (Ks is zero there and the padding rows of L^-1 are identity) and its rows >= nt (Ks rows are
// zero there): no masking, and the k range ends at kend = n rounded up to BK.  Few tiles cannot fill the chip, so the k
// range of a tile is split into `split` chunks of kstep: workgroup (tile, s) writes its partial product to P (s = 0, the
// factor handle's A, ld = ldp) or to scratch slot s - 1 (pstride doubles apart, same layout).  k_predict_cov_finish adds
// the chunks in index order: the bits do not depend on which workgroup ends first.
template <int WM>
__global__ __launch_bounds__(256, 2) void k_predict_cov(const double* __restrict__ W, int ld, int kend, int kstep,
                                                        int split, double* __restrict__ P, double* __restrict__ scr,
                                                        size_t pstride, int ldp, unsigned long long* stamp)
{
    LaunchStamp stamp_(stamp);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int BT = 32 * WM;
    const int tile = blockIdx.x / split, s = blockIdx.x % split;
    int ti, tj;
    tri_index(tile, ti, tj);
    const int k0 = s * kstep, k1 = k0 + kstep < kend ? k0 + kstep : kend;
    d4 acc[WM][WM];
    acc_zero(acc);
    tile_nt<false>(W + (size_t)ti * BT * ld, ld, W + (size_t)tj * BT * ld, ld, k0, k1, acc, smem);
    double* C = s == 0 ? P : scr + (size_t)(s - 1) * pstride;
    tile_store(C + (size_t)ti * BT * ldp + tj * BT, ldp, acc, 1.0);
}

// Epilogue, on the lower 64x64 tiles that k_build writes (the layout the Cholesky reads): A = kss (+ sn2 + jitter on the
// diagonal) - (P_0 + P_1 + ...), in place over P_0; kss = sf2 exp(-|xt_i - xt_j|^2 / (2 l^2)) by k_build's formula and
// squared-distance order; padding rows / columns >= nt become identity.  tickets (when given): the factorisation's
// arrival counters, zeroed as k_build does.
template <bool ARD, int KIND>
__device__ __forceinline__ void predict_cov_finish_body(const double* __restrict__ Xt, int nt, int d, int ntpad,
                                                        const HyperScalars& h, const double* __restrict__ wts,
                                                        int with_noise, double jitter,
                                                        double* __restrict__ A, const double* __restrict__ scr,
                                                        size_t pstride, int nscr, unsigned* __restrict__ tickets)
{
#pragma clang fp contract(off)
    if (tickets && blockIdx.x == 0)
        for (int i = threadIdx.x; i < ticket_count(ntpad / TILE); i += 256) tickets[i] = 0u;
    __shared__ double xs[KT][DC + 1], ys[KT][DC + 1];
    int ti, tj;
    tri_index(blockIdx.x, ti, tj);
    const int i0 = ti * KT, j0 = tj * KT;
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    double d2v[4][4];
    __shared__ double ws[DC];
    sqdist_4x4<ARD>(Xt, Xt, nt, nt, d, i0, j0, xs, ys, d2v, wts, ws);
    const DivBy dl = div_prepare(h.ell_sq);
#pragma unroll
    for (int a = 0; a < 4; a++) {
        const int i = i0 + ty * 4 + a;
        const size_t off = (size_t)i * ntpad + j0 + tx * 2;
        d2 p01 = *(const d2*)(A + off), p23 = *(const d2*)(A + off + 32);
        for (int s = 0; s < nscr; s++) {
            const double* q = scr + (size_t)s * pstride + off;
            p01 = p01 + *(const d2*)q;
            p23 = p23 + *(const d2*)(q + 32);
        }
        const double p[4] = {p01[0], p01[1], p23[0], p23[1]};
        double o[4];
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const int j = j0 + col4(tx, b);
            double v = kernel_value<ARD, KIND>(d2v[a][b], dl, h.signal_var);
            if (i == j) {
                if (with_noise) v += h.noise_var;
                v += jitter;
            }
            o[b] = (i < nt && j < nt) ? v - p[b] : ((i == j) ? 1.0 : 0.0);
        }
        *(d2*)(A + off) = (d2){o[0], o[1]};
        *(d2*)(A + off + 32) = (d2){o[2], o[3]};
    }
}

template <bool ARD, int KIND>
__global__ __launch_bounds__(256) void k_predict_cov_finish(const double* __restrict__ Xt, int nt, int d, int ntpad,
                                                            HyperScalars h_arg, int with_noise, double jitter,
                                                            double* __restrict__ A, const double* __restrict__ scr,
                                                            size_t pstride, int nscr, unsigned* __restrict__ tickets,
                                                            const HyperScalars* __restrict__ hd)
{
    predict_cov_finish_body<ARD, KIND>(Xt, nt, d, ntpad, ARD ? *hd : h_arg, ARD ? ard_weights(hd) : nullptr, with_noise,
                                       jitter, A, scr, pstride, nscr, tickets);
}

// The Cholesky writes the lower triangle only: the strict upper part of every 128x128 diagonal tile still holds Sigma,
// and k_predict_gemm reads its diagonal 64-tiles whole.  Zeroed here, one workgroup per diagonal tile.
__global__ __launch_bounds__(256) void k_zero_upper_diag(double* __restrict__ A, int ld)
{
    double* T = A + (size_t)blockIdx.x * TILE * ld + (size_t)blockIdx.x * TILE;
    for (int e = threadIdx.x; e < TILE * TILE; e += 256) {
        const int r = e / TILE, c = e % TILE;
        if (c > r) T[(size_t)r * ld + c] = 0.0;
    }
}

// posterior draws: out[s * nt + t] = mean[t] + F[s][t]   (F = Z C^T, k_predict_gemm over the factor)
__global__ __launch_bounds__(256) void k_sample_finish(const double* __restrict__ F, int ld, const double* __restrict__ mean,
                                                       int nt, int ns, double* __restrict__ out)
{
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)nt * ns) return;
    const size_t s = idx / nt, t = idx % nt;
    out[idx] = mean[t] + F[s * ld + t];
}

// ------------------------------------------------------------------------------------------
// The Cholesky and the inverse, each kernel with its launcher (need everything above: cov_device.h, the tile product
// in both geometries, the launch machinery)
// ------------------------------------------------------------------------------------------
#include "chol_gfx950.h"
#include "inverse_gfx950.h"


// ------------------------------------------------------------------------------------------
// vector kernels
// ------------------------------------------------------------------------------------------
// z[i] = sum_{k < (ti+1)*128} T[i][k] x[k]  (one wave per row; the diagonal tile is zero above the diagonal)
__global__ __launch_bounds__(256) void k_trmv_lower(const double* __restrict__ T, int ld, int npad,
                                                    const double* __restrict__ x, double* __restrict__ z,
                                                    const ExpertPtrs* __restrict__ bt)
{
    if (bt) { T = GP(bt[blockIdx.y].T); x = GP(bt[blockIdx.y].y); z = GP(bt[blockIdx.y].z); }
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= npad) return;
    const int kend = (row / TILE + 1) * TILE;
    const double* tr = T + (size_t)row * ld;
    double s = 0.0;
    for (int k = lane * 2; k < kend; k += 128) {
        d2 v = *(const d2*)(tr + k), xv = *(const d2*)(x + k);
        s += v[0] * xv[0] + v[1] * xv[1];
    }
    s = wave_sum(s);
    if (lane == 0) z[row] = s;
}

// a[i] = sum_{k >= ti*128} U[i][k] x[k]
__global__ __launch_bounds__(256) void k_trmv_upper(const double* __restrict__ U, int ld, int npad,
                                                    const double* __restrict__ x, double* __restrict__ a,
                                                    const ExpertPtrs* __restrict__ bt)
{
    if (bt) { U = GP(bt[blockIdx.y].U); x = GP(bt[blockIdx.y].z); a = GP(bt[blockIdx.y].alpha); }
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= npad) return;
    const int kbeg = (row / TILE) * TILE;
    const double* ur = U + (size_t)row * ld;
    double s = 0.0;
    for (int k = kbeg + lane * 2; k < npad; k += 128) {
        d2 v = *(const d2*)(ur + k), xv = *(const d2*)(x + k);
        s += v[0] * xv[0] + v[1] * xv[1];
    }
    s = wave_sum(s);
    if (lane == 0) a[row] = s;
}

// w = y for every expert of a batched launch (the forward substitution consumes w)
__global__ __launch_bounds__(256) void k_copy_y_to_w(int npad, const ExpertPtrs* __restrict__ bt)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < npad) GP(bt[blockIdx.y].w)[i] = GP(bt[blockIdx.y].y)[i];
}

// blocked forward substitution L z = y (LL-only path): step kb = (1) z_kb = T_kk w_kb, (2) w[rows below] -= L21 z_kb
__global__ __launch_bounds__(256) void k_trsv_diag(const double* __restrict__ T, int ld, int kb,
                                                   const double* __restrict__ w, double* __restrict__ z,
                                                   const ExpertPtrs* __restrict__ bt)
{
    if (bt) { T = GP(bt[blockIdx.y].T); w = GP(bt[blockIdx.y].w); z = GP(bt[blockIdx.y].z); }
    // z_kb = T_kk w_kb (128x128, lower): two threads per row, 64 columns each, 16-byte loads
    __shared__ double ws[TILE];
    const int k0 = kb * TILE, t = threadIdx.x;
    if (t < TILE) ws[t] = w[k0 + t];
    __syncthreads();
    const int r = t >> 1, h = t & 1;
    const double* tr = T + (size_t)(k0 + r) * ld + k0 + h * 64;
    double s0 = 0.0, s1 = 0.0;
#pragma unroll 8
    for (int c = 0; c < 64; c += 2) {
        const d2 v = *(const d2*)(tr + c);
        s0 = __builtin_fma(v[0], ws[h * 64 + c], s0);
        s1 = __builtin_fma(v[1], ws[h * 64 + c + 1], s1);
    }
    double sum = s0 + s1;
    sum += __shfl_xor(sum, 1, 64);
    if (h == 0) z[k0 + r] = sum;
}

__global__ __launch_bounds__(256) void k_trsv_update(const double* __restrict__ A, int ld, int kb, int npad,
                                                     const double* __restrict__ z, double* __restrict__ w,
                                                     const ExpertPtrs* __restrict__ bt)
{
    if (bt) { A = GP(bt[blockIdx.y].A); z = GP(bt[blockIdx.y].z); w = GP(bt[blockIdx.y].w); }
    const int k0 = kb * TILE;
    const int row = k0 + TILE + blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= npad) return;
    const double* ar = A + (size_t)row * ld + k0;
    d2 v = *(const d2*)(ar + lane * 2), xv = *(const d2*)(z + k0 + lane * 2);
    double s = wave_sum(v[0] * xv[0] + v[1] * xv[1]);
    if (lane == 0) w[row] -= s;
}

// Final sums of an evaluation by ONE workgroup of NTHR threads, in the order 1024 threads would take them whatever NTHR
// is (so the stand-alone k_finalize, 1024 threads, and the last block of k_trace, 256 threads, give the same bits):
// virtual thread v = 0..1023 sums the entries i = v, v + 1024, ... ascending, then the halving tree red[v] += red[v + w],
// w = 512 .. 1.  A real thread takes the virtual threads t, t + NTHR, ... and the tree levels above NTHR in registers.
// HANDED: the trace partials were written by other workgroups of this launch -- agent-scope loads.
// red: 5 * NTHR / ... doubles of LDS: [5][NTHR].
constexpr int FIN_THREADS = 1024;     // one workgroup; at N = 8192 it sums 3 x 8256 trace partials and 8192 squares (23 us with 256 threads)
template <int NTHR, bool HANDED>
__device__ __forceinline__ void finalize_sums(const double* __restrict__ z, int npad, int n,
                                              const double* __restrict__ logdet_part, int nt,
                                              const double* __restrict__ part, int nblocks, HyperScalars h,
                                              double* __restrict__ out, double* __restrict__ hout, double* red)
{
    constexpr int V = FIN_THREADS / NTHR;              // virtual threads per real thread
    const int t = threadIdx.x;
    double acc[5][V];
#pragma unroll
    for (int j = 0; j < V; j++) {
        const int v = t + j * NTHR;
        double q = 0.0, ld = 0.0, s0 = 0.0, s1 = 0.0, s2 = 0.0;
        for (int i = v; i < npad; i += FIN_THREADS) q += z[i] * z[i];
        for (int i = v; i < nt; i += FIN_THREADS) ld += logdet_part[i];
        if (part)
            for (int i0 = v; i0 < nblocks; i0 += 4 * FIN_THREADS) {
                // four entries' loads in flight before the first is added (agent-scope loads one by one cost a memory
                // latency each: 40 us for the 8256 partials of an 8192-row matrix); the sums are taken in order
                double p[4][3];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int i = i0 + u * FIN_THREADS;
                    const double* pp = part + (size_t)(i < nblocks ? i : v) * 3;
#pragma unroll
                    for (int c = 0; c < 3; c++)
                        p[u][c] = HANDED ? __hip_atomic_load(pp + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : pp[c];
                }
#pragma unroll
                for (int u = 0; u < 4; u++)
                    if (i0 + u * FIN_THREADS < nblocks) { s0 += p[u][0]; s1 += p[u][1]; s2 += p[u][2]; }
            }
        acc[0][j] = q; acc[1][j] = ld; acc[2][j] = s0; acc[3][j] = s1; acc[4][j] = s2;
    }
    // tree levels w >= NTHR: red[v] += red[v + w] pairs virtual threads of the SAME real thread (v and v + w differ by a multiple of NTHR)
#pragma unroll
    for (int w = V / 2; w > 0; w >>= 1)
#pragma unroll
        for (int c = 0; c < 5; c++)
#pragma unroll
            for (int j = 0; j < w; j++) acc[c][j] += acc[c][j + w];
    __syncthreads();                                   // (red may alias LDS the caller used before)
#pragma unroll
    for (int c = 0; c < 5; c++) red[c * NTHR + t] = acc[c][0];
    __syncthreads();
    for (int w = NTHR / 2; w > 0; w >>= 1) {
        if (t < w)
            for (int c = 0; c < 5; c++) red[c * NTHR + t] += red[c * NTHR + t + w];
        __syncthreads();
    }
    if (t == 0) {
        const double quad = red[0], logdet = 2 * red[NTHR];
        out[0] = -0.5 * (quad + logdet + n * 1.83787);
        if (part) {
            const double s1 = red[2 * NTHR], s2 = red[3 * NTHR], s3 = red[4 * NTHR];
            out[1] = s1 / 2.0;
            out[2] = (2.0 * s2 - 2.0 * h.noise_var * s3) / 2.0;
            out[3] = (2.0 * h.noise_var * s3) / 2.0;
        }
        out[4] = quad;
        out[5] = logdet;
        if (hout)
            for (int i = 0; i < 6; i++) hout[i] = out[i];
    }
}

// what the last block of k_trace needs to finish the evaluation (out == nullptr: no fused finalize)
struct FinalizeArgs {
    const double* z; const double* logdet_part; int nt; double* out; double* hout; unsigned* ticket;
};

// gradient traces, fused: for every lower 64x64 tile recompute k(xi,xj) and |xi-xj|^2/l^2, read K^-1 once,
// W = K^-1 - alpha alpha^T, accumulate  s1 = sum W*K*S, s2 = sum W*K, s3 = sum_i W_ii  (off-diagonal tiles x2)
// KIND: s1 is sum W o dK/dlog l -- SE's K o S, or a Matern kind's dk of matern_entry (one exp(-a) for k and dk; zero on
// the diagonal, where a = 0); s2, s3 and everything behind the sums keep their meaning
// TARGETS (multi-target regression, k_trace_targets): the same tile, thread layout, entry formulas, doubling of the
// off-diagonal entries, diagonal handling and partial sums (part[3 * block + c]) with W = m K^-1 - sum_t alpha_t alpha_t^T
// from the target-major AV ([m][npad]) in place of K^-1 - alpha alpha^T.  K^-1 is read once whatever m is; no N x N
// intermediate is written.  Single handle, h by value, always the separate final sums (bt, hd and fin.out null).
template <int KIND, bool TARGETS>
__device__ __forceinline__ void trace_body(const double* __restrict__ X, int n, int d, int npad,
                                           HyperScalars h_arg, const HyperScalars* __restrict__ hd,
                                           const double* __restrict__ Kinv, const double* __restrict__ AV, int m,
                                           double* __restrict__ part, const ExpertPtrs* __restrict__ bt,
                                           FinalizeArgs fin)
{
    if (!TARGETS && bt) {
        const ExpertPtrs& e = bt[blockIdx.y];
        X = GP(e.X); n = e.n; Kinv = GP(e.Kinv); AV = GP(e.alpha); part = GP(e.part);
        if (fin.out) {
            fin.z = GP(e.z); fin.logdet_part = GP(e.logdet); fin.out = GP(e.out); fin.ticket = GP(e.tickets) + 2 * fin.nt;
            if (fin.hout) fin.hout += (size_t)blockIdx.y * 8;
        }
    }
    const HyperScalars h = hd ? *hd : h_arg;
    // (one buffer: the two X tiles of the squared distances, later the [5][256] sums of the fused finalize)
    __shared__ double lds[2 * KT * (DC + 1)];
    static_assert(2 * KT * (DC + 1) >= 5 * 256, "the fused finalize reduces in the X tiles' LDS");
    double (&xs)[KT][DC + 1] = *reinterpret_cast<double (*)[KT][DC + 1]>(lds);
    double (&ys)[KT][DC + 1] = *reinterpret_cast<double (*)[KT][DC + 1]>(lds + KT * (DC + 1));
    __shared__ double red[3][4];
    int ti, tj;
    tri_index(blockIdx.x, ti, tj);
    const int i0 = ti * KT, j0 = tj * KT;
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    double d2v[4][4], S[4][4];
    sqdist_4x4(X, X, n, n, d, i0, j0, xs, ys, d2v);
    if constexpr (TARGETS) {
        __shared__ __attribute__((aligned(16))) double la[TGT_CHUNK][KT], lb[TGT_CHUNK][KT];
        targets_outer_4x4(AV, npad, m, i0, j0, la, lb, S);
    }
    double s1 = 0.0, s2 = 0.0, s3 = 0.0;
    const DivBy dl = div_prepare(h.ell_sq);
    const double dm = (double)m;
    double aj[4];
    if constexpr (!TARGETS) {
#pragma unroll
        for (int b = 0; b < 4; b++) aj[b] = AV[j0 + col4(tx, b)];
    }
#pragma unroll
    for (int a = 0; a < 4; a++) {
        const int i = i0 + ty * 4 + a;
        const double ai = TARGETS ? 0.0 : AV[i];
        const double* kr = Kinv + (size_t)i * npad + j0 + tx * 2;
        d2 k01 = *(const d2*)kr, k23 = *(const d2*)(kr + 32);
        const double kv[4] = {k01[0], k01[1], k23[0], k23[1]};
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const int j = j0 + col4(tx, b);
            if (i < n && j < n && (ti != tj || j <= i)) {
                double w;
                if constexpr (TARGETS) w = dm * kv[b] - S[a][b];
                else w = kv[b] - ai * aj[b];
                if constexpr (KIND == KERNEL_SE) {
                    double kse = h.signal_var * exp(div_by(-d2v[a][b] * 0.5, dl));
                    const double sd = div_by(d2v[a][b], dl);
                    if (i == j) {
                        kse += h.noise_var;
                        s1 += w * (kse * sd);
                        s2 += w * kse;
                        s3 += w;
                    } else {
                        s1 += 2.0 * (w * (kse * sd));
                        s2 += 2.0 * (w * kse);
                    }
                } else {
                    double kf, dk, hh;
                    matern_entry<KIND>(div_by(d2v[a][b], dl), h.signal_var, kf, dk, hh);
                    if (i == j) {
                        kf += h.noise_var;
                        s1 += w * dk;
                        s2 += w * kf;
                        s3 += w;
                    } else {
                        s1 += 2.0 * (w * dk);
                        s2 += 2.0 * (w * kf);
                    }
                }
            }
        }
    }
    s1 = wave_sum(s1); s2 = wave_sum(s2); s3 = wave_sum(s3);
    if ((t & 63) == 0) { red[0][t >> 6] = s1; red[1][t >> 6] = s2; red[2][t >> 6] = s3; }
    __syncthreads();
    if (!fin.out) {
        if (t < 3) part[(size_t)blockIdx.x * 3 + t] = (red[t][0] + red[t][1]) + (red[t][2] + red[t][3]);
        return;
    }
    // Fused finalize (round 6): the partial sums leave write-through, the block draws a ticket, and the LAST block of the
    // launch (of this expert) goes on to the final sums and the scalar formulas -- what k_finalize did as one more launch
    // behind this one (a kernel boundary and a 1-workgroup launch on the serial tail of every evaluation: ~9 us of a
    // 590-us evaluation at 1500 rows).  The hand-off is the step kernel's (k_syrk_step): write-through (agent-scope)
    // stores by lanes of wave 0, that wave's vmcnt(0), one relaxed agent-scope ticket; the last arriver reads every
    // partial with agent-scope loads.  Same sums in the same order as k_finalize: identical bits.
    __shared__ unsigned s_ticket;
    if (t < 3) __hip_atomic_store(part + (size_t)blockIdx.x * 3 + t, (red[t][0] + red[t][1]) + (red[t][2] + red[t][3]),
                                  __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (t < 64) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (t == 0) s_ticket = __hip_atomic_fetch_add(fin.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (s_ticket != gridDim.x - 1) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (t == 0) *fin.ticket = 0u;                          // (ready for the next evaluation; nobody else touches it any more)
    finalize_sums<256, true>(fin.z, npad, n, fin.logdet_part, fin.nt, part, (int)gridDim.x, h, fin.out, fin.hout, lds);
}

// single workgroup: deterministic final sums and the scalar formulas
//   LL = -0.5 (z'z + 2 sum log L_ii + n * 1.83787)                     covkernel.cpp:127
//   g0 = s1/2, g1 = (2 s2 - 2 sn2 s3)/2, g2 = (2 sn2 s3)/2              covkernel.cpp:244-261
__global__ __launch_bounds__(FIN_THREADS) void k_finalize(const double* __restrict__ z, int npad, int n,
                                                  const double* __restrict__ logdet_part, int nt,
                                                  const double* __restrict__ part, int nblocks,
                                                  HyperScalars h_arg, const HyperScalars* __restrict__ hd,
                                                  double* __restrict__ out, double* __restrict__ hout,
                                                  const ExpertPtrs* __restrict__ bt)
{
    // hout: the same 6 results straight into the caller's pinned host buffer ([expert][8]) -- visible to the host
    // when the launch has completed, no copy node (and its ~10-us boundary) behind the evaluation
    if (bt) {
        const ExpertPtrs& e = bt[blockIdx.y];
        z = GP(e.z); n = e.n; logdet_part = GP(e.logdet); out = GP(e.out);
        if (part) part = GP(e.part);
        if (hout) hout += (size_t)blockIdx.y * 8;
    }
    const HyperScalars h = hd ? *hd : h_arg;
    __shared__ double red[5 * FIN_THREADS];
    finalize_sums<FIN_THREADS, false>(z, npad, n, logdet_part, nt, part, nblocks, h, out, hout, red);
}

// k_trace: the gradient pass of a single-target evaluation.  ARD (trace_ard_body: cov_device.h): always followed by
// k_finalize_ard (fin is not read).
template <bool ARD, int KIND>
__global__ __launch_bounds__(256) void k_trace(const double* __restrict__ X, int n, int d, int npad,
                                               HyperScalars h_arg, const HyperScalars* __restrict__ hd,
                                               const double* __restrict__ Kinv, const double* __restrict__ alpha,
                                               double* __restrict__ part, const ExpertPtrs* __restrict__ bt,
                                               FinalizeArgs fin)
{
    if constexpr (ARD) trace_ard_body<KIND, false>(X, n, d, npad, hd, Kinv, alpha, 1, part, bt);
    else trace_body<KIND, false>(X, n, d, npad, h_arg, hd, Kinv, alpha, 1, part, bt, fin);
}

// k_trace_targets: the same for the summed objective of m targets (A: [m][npad], row t = alpha_t); k_finalize_targets follows
template <bool ARD, int KIND>
__global__ __launch_bounds__(256) void k_trace_targets(const double* __restrict__ X, int n, int d, int npad,
                                                       HyperScalars h, const double* __restrict__ Kinv,
                                                       const double* __restrict__ A, int m, double* __restrict__ part,
                                                       const HyperScalars* __restrict__ hd)
{
    if constexpr (ARD) trace_ard_body<KIND, true>(X, n, d, npad, hd, Kinv, A, m, part, nullptr);
    else trace_body<KIND, true>(X, n, d, npad, h, nullptr, Kinv, A, m, part, nullptr, FinalizeArgs{});
}

// Final sums of an ARD gradient evaluation, one workgroup.  LL, y'K^-1y and log|K| by finalize_sums (the isotropic
// order and bits); then wave w takes the columns w, w + 16, ... of the trace partials: lane l adds the blocks l, l + 64,
// ... ascending, the lanes by wave_sum -- a fixed order whatever the timing.  Results row (out, hout): [0] LL, [4] quad,
// [5] log|K|, [6] status word, [8 + c] the d + 2 gradient components:
//   g_c = S_c / 2 (c < d), g_d = (2 s2 - 2 sn2 s3) / 2, g_{d+1} = (2 sn2 s3) / 2   (the last two as k_finalize's g1, g2)
// bt (batched): grid (1, experts) -- z, n, logdet_part, part and out from the expert's table entry, hout + expert * hstride
__global__ __launch_bounds__(FIN_THREADS) void k_finalize_ard(const double* __restrict__ z, int npad, int n, int d,
                                                              const double* __restrict__ logdet_part, int nt,
                                                              const double* __restrict__ part, int nblocks,
                                                              const HyperScalars* __restrict__ hd,
                                                              double* __restrict__ out, double* __restrict__ hout,
                                                              size_t hstride, const ExpertPtrs* __restrict__ bt)
{
    if (bt) {
        const ExpertPtrs& e = bt[blockIdx.y];
        z = GP(e.z); n = e.n; logdet_part = GP(e.logdet); part = GP(e.part); out = GP(e.out);
        hout += (size_t)blockIdx.y * hstride;
    }
    const HyperScalars h = *hd;
    __shared__ double red[5 * FIN_THREADS];
    finalize_sums<FIN_THREADS, false>(z, npad, n, logdet_part, nt, nullptr, 0, h, out, hout, red);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    for (int c = wave; c < d + 2; c += FIN_THREADS / 64) {
        const double* col = part + (size_t)c * nblocks;
        double s = 0.0;
        for (int i = lane; i < nblocks; i += 64) s += col[i];
        s = wave_sum(s);
        if (lane == 0 && c < d) { out[8 + c] = s / 2.0; hout[8 + c] = s / 2.0; }
        if (lane == 0 && c >= d) red[16 + (c - d)] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double s2 = red[16], s3 = red[17];
        const double gf = (2.0 * s2 - 2.0 * h.noise_var * s3) / 2.0, gn = (2.0 * h.noise_var * s3) / 2.0;
        out[8 + d] = gf; out[9 + d] = gn;
        hout[8 + d] = gf; hout[9 + d] = gn;
    }
}

// one expert's row of the product-of-experts exchange (BCM.cpp:51-55): 1/v and (1/v) m, rounded separately as the host
// loop of cugp_bcm_predict_partial does (IEEE division, no contraction)
__device__ __forceinline__ void poe_row(double m, double v, double* __restrict__ p, double* __restrict__ pm)
{
#pragma clang fp contract(off)
    const double inv = 1.0 / v;
    *p = inv;
    *pm = inv * m;
}

// mean[t] = Ks[t] . alpha ; var[t] = sf2 + sn2 - |W[t]|^2        covkernel.cpp:314-319
// mean / var may be null; rows (when given): 1/var[t] -> rows[t], mean[t]/var[t] -> rows[rhalf + t] (poe_row).
// bt (batched): blockIdx.y selects the expert -- alpha from its table entry, Ks and W its [ntpad][npad] slices,
// rows + blockIdx.y * rstride its rows
__global__ __launch_bounds__(256) void k_predict_finish(const double* __restrict__ Ks, const double* __restrict__ W,
                                                        const double* __restrict__ alpha, int n, int npad,
                                                        int ntest, HyperScalars h, double* __restrict__ mean,
                                                        double* __restrict__ var, double* __restrict__ rows,
                                                        size_t rstride, int rhalf, int ntpad,
                                                        const ExpertPtrs* __restrict__ bt)
{
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= ntest) return;
    if (bt) {
        const size_t off = (size_t)blockIdx.y * ntpad * npad;
        alpha = GP(bt[blockIdx.y].alpha); Ks += off; W += off;
        rows += (size_t)blockIdx.y * rstride;
    }
    const double* kr = Ks + (size_t)row * npad;
    const double* wr = W + (size_t)row * npad;
    double m = 0.0, q = 0.0;
    for (int k = lane * 2; k < npad; k += 128) {
        d2 kv = *(const d2*)(kr + k), av = *(const d2*)(alpha + k), wv = *(const d2*)(wr + k);
        m += kv[0] * av[0] + kv[1] * av[1];
        q += wv[0] * wv[0] + wv[1] * wv[1];
    }
    m = wave_sum(m); q = wave_sum(q);
    if (lane == 0) {
        const double v = h.signal_var + h.noise_var - q;
        if (mean) { mean[row] = m; var[row] = v; }
        if (rows) poe_row(m, v, rows + row, rows + rhalf + row);
    }
}

// k_predict_finish for the experts of a group, leaving m and v THEMSELVES in the expert's rows (the batched form above
// writes only 1/v and m/v): blockIdx.y selects the expert -- alpha from its table entry, Ks and W its [ntpad][npad]
// slices -- and row t's mean goes to mean[blockIdx.y * row_stride + t], its variance to var[...] alike.  The sums are
// k_predict_finish's own, the same loop and the same wave_sum (repeated, not shared through a function: inlining one
// into k_predict_finish reordered its instructions, and the kernels that exist keep theirs): every expert's m and v
// carry cugp_predict's bits, with noise_var = 0 in h cugp_predict_latent's.
__global__ __launch_bounds__(256) void k_predict_finish_mv(const double* __restrict__ Ks, const double* __restrict__ W,
                                                           int npad, int ntest, HyperScalars h, double* __restrict__ mean,
                                                           double* __restrict__ var, size_t row_stride, int ntpad,
                                                           const ExpertPtrs* __restrict__ bt)
{
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= ntest) return;
    const size_t off = (size_t)blockIdx.y * ntpad * npad + (size_t)row * npad;
    const double* __restrict__ alpha = GP(bt[blockIdx.y].alpha);
    const double* kr = Ks + off;
    const double* wr = W + off;
    double m = 0.0, q = 0.0;
    for (int k = lane * 2; k < npad; k += 128) {
        d2 kv = *(const d2*)(kr + k), av = *(const d2*)(alpha + k), wv = *(const d2*)(wr + k);
        m += kv[0] * av[0] + kv[1] * av[1];
        q += wv[0] * wv[0] + wv[1] * wv[1];
    }
    m = wave_sum(m); q = wave_sum(q);
    if (lane == 0) {
        mean[(size_t)blockIdx.y * row_stride + row] = m;
        var[(size_t)blockIdx.y * row_stride + row] = h.signal_var + h.noise_var - q;
    }
}

// Product of experts over the gathered exchange buffer (comm.cpp: cugp_bcm_predict_allgather).  g: [world][rstride]
// doubles, rank r's block = {status, local expert count, [per][2][nt] rows: 1/v, m/v}.  Test point t sums over the
// experts k = 0..K-1 in GLOBAL order -- expert k is rank k mod world's (k / world)-th -- then var = 1/sum, mean =
// var * sum (BCM.cpp:51-60), the same operations in the same order as cugp_bcm_predict_partial + cugp_poe_finish.
// out: [mean nt | var nt | world x {status, count}].
__global__ __launch_bounds__(256) void k_poe_reduce(const double* __restrict__ g, size_t rstride, int world, int K,
                                                    int nt, double* __restrict__ out)
{
#pragma clang fp contract(off)
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (blockIdx.x == 0)
        for (int r = threadIdx.x; r < world; r += 256) {
            out[2 * (size_t)nt + 2 * r] = g[(size_t)r * rstride];
            out[2 * (size_t)nt + 2 * r + 1] = g[(size_t)r * rstride + 1];
        }
    if (t >= nt) return;
    double sp = 0.0, spm = 0.0;
    for (int k = 0; k < K; k++) {
        const double* b = g + (size_t)(k % world) * rstride + 2 + (size_t)(k / world) * 2 * nt;
        sp = sp + b[t];
        spm = spm + b[nt + t];
    }
    const double tv = 1.0 / sp;
    out[t] = tv * spm;
    out[nt + t] = tv;
}

// The weighted combinations of LATENT expert distributions (include/cugp.h: CUGP_COMBINE_*; comm.cpp, bcm.cpp).  g and
// out as k_poe_reduce's, the rows here p_k = 1/var_f,k and pm_k = m_k/var_f,k (k_predict_finish with noise_var = 0).  Per
// test point, experts in global order, every operation rounded on its own:
//   beta_k = 1 (mode 0 POE, 2 BCM) | RN(1 / K) (1 gPoE) | 1/2 log(sf2 p_k) (3 rBCM)
//   sp += beta_k p_k, spm += beta_k pm_k, sb += beta_k;   prec = sp (+ (1 - sb) / sf2 for modes 2, 3)
//   var_f = 1 / prec, mean = var_f spm, var = var_f (+ sn2 when with_noise)
// cugp_poe_combine (bcm.cpp) is the host twin: the same operations in the same order.
__global__ __launch_bounds__(256) void k_poe_reduce_mode(const double* __restrict__ g, size_t rstride, int world, int K,
                                                         int nt, int mode, double sf2, double sn2, int with_noise,
                                                         double* __restrict__ out)
{
#pragma clang fp contract(off)
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (blockIdx.x == 0)
        for (int r = threadIdx.x; r < world; r += 256) {
            out[2 * (size_t)nt + 2 * r] = g[(size_t)r * rstride];
            out[2 * (size_t)nt + 2 * r + 1] = g[(size_t)r * rstride + 1];
        }
    if (t >= nt) return;
    const double bg = 1.0 / (double)K;
    double sp = 0.0, spm = 0.0, sb = 0.0;
    for (int k = 0; k < K; k++) {
        const double* b = g + (size_t)(k % world) * rstride + 2 + (size_t)(k / world) * 2 * nt;
        const double p = b[t], pm = b[nt + t];
        double beta = 1.0;
        if (mode == 1) beta = bg;
        else if (mode == 3) beta = 0.5 * log(sf2 * p);
        sp = sp + beta * p;
        spm = spm + beta * pm;
        sb = sb + beta;
    }
    double prec = sp;
    if (mode >= 2) prec = sp + (1.0 - sb) / sf2;
    const double tv = 1.0 / prec;
    out[t] = tv * spm;
    out[nt + t] = with_noise ? tv + sn2 : tv;
}

// ------------------------------------------------------------------------------------------
// Multi-target regression: m target vectors over the handle's one factorisation (cugp_set_targets).  Everything is
// target-major, [mpad][npad] with zeros beyond n and beyond m: Y the targets, Z = Y L^-T (k_predict_gemm as it stands),
// A = Z L^-1 (row t = alpha_t, k_targets_alpha), then ONE pass over K^-1 for the gradient of the summed objective
// (k_trace_targets), the final sums (k_finalize_targets) and the means A Ks^T (k_targets_mean).
// The kernels have bodies of their own: the single-target kernels above keep their instructions.
// ------------------------------------------------------------------------------------------

// A[t][j] = sum_{k >= j} Z[t][k] U[j][k], U = L^-T row-major and upper triangular.  Column tile tj (64 wide) takes the k
// range from its own diagonal, tj * 64, to npad: U's diagonal 128x128 tiles hold exact zeros below the diagonal
// (trtri_diag_body writes every entry of them, 0.0 where the row index exceeds the column's), so the second 64-column half
// of a 128-tile may start at its own first column; tiles LEFT of the diagonal tile are never written and never read here.
// The work of a column tile falls linearly with tj, so the tiles run in pairs (tj = p, the long one, then n64 - 1 - p):
// every workgroup sums (n64 + 1) * 64 k in all, as k_predict_gemm's pairs do.  Grid: m64 * n64 / 2.
__global__ __launch_bounds__(256, 2) void k_targets_alpha(const double* __restrict__ Z, const double* __restrict__ U,
                                                          double* __restrict__ A, int ld, int m64, int n64)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tt = blockIdx.x % m64, p = blockIdx.x / m64;
#pragma unroll 1
    for (int h = 0; h < 2; h++) {
        const int tj = h == 0 ? p : n64 - 1 - p;
        d4 acc[2][2];
        acc_zero(acc);
        tile_nt<false>(Z + (size_t)tt * 64 * ld, ld, U + (size_t)tj * 64 * ld, ld, tj * 64, n64 * 64, acc, smem);
        tile_store(A + (size_t)tt * 64 * ld + tj * 64, ld, acc, 1.0);
    }
}

// k_targets_alpha for the experts of a group (V = W L^-1 of cugp_bcm_predict_grad): the same tile pairing and k ranges,
// blockIdx.y selects the expert -- U from its table entry, Z and A its [m64 * 64][ld] slices.
__global__ __launch_bounds__(256, 2) void k_targets_alpha_batched(const double* __restrict__ Z, double* __restrict__ A,
                                                                  int ld, int m64, int n64,
                                                                  const ExpertPtrs* __restrict__ bt)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const size_t off = (size_t)blockIdx.y * m64 * 64 * ld;
    const double* __restrict__ U = GP(bt[blockIdx.y].U);
    Z += off; A += off;
    const int tt = blockIdx.x % m64, p = blockIdx.x / m64;
#pragma unroll 1
    for (int h = 0; h < 2; h++) {
        const int tj = h == 0 ? p : n64 - 1 - p;
        d4 acc[2][2];
        acc_zero(acc);
        tile_nt<false>(Z + (size_t)tt * 64 * ld, ld, U + (size_t)tj * 64 * ld, ld, tj * 64, n64 * 64, acc, smem);
        tile_store(A + (size_t)tt * 64 * ld + tj * 64, ld, acc, 1.0);
    }
}

// Partial means P_s[t][i] = sum_{k in chunk s} A[t][k] Ks[i][k]: an NT product of two k-contiguous operands, 64x64 output
// tiles, the k range in chunks of kstep (a function of nothing but the launch's npad, so that a target's bits do not
// depend on how many targets there are).  P: [split][m64 * 64][ntpad].  Grid: m64 * nt64 * split.
__global__ __launch_bounds__(256, 2) void k_targets_mean(const double* __restrict__ A, const double* __restrict__ Ks,
                                                         double* __restrict__ P, int ld, int m64, int nt64, int kstep,
                                                         size_t pstride, int ntpad)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tt = blockIdx.x % m64, r = blockIdx.x / m64, ii = r % nt64, s = r / nt64;
    const int k0 = s * kstep, k1 = k0 + kstep < ld ? k0 + kstep : ld;
    d4 acc[2][2];
    acc_zero(acc);
    tile_nt<false>(A + (size_t)tt * 64 * ld, ld, Ks + (size_t)ii * 64 * ld, ld, k0, k1, acc, smem);
    tile_store(P + (size_t)s * pstride + (size_t)tt * 64 * ntpad + ii * 64, ntpad, acc, 1.0);
}

// mean[t * nt + i] = P_0[t][i] + P_1[t][i] + ... in chunk order, packed [m][nt]
__global__ __launch_bounds__(256) void k_targets_mean_finish(const double* __restrict__ P, size_t pstride, int split,
                                                             int ntpad, int m, int nt, double* __restrict__ mean)
{
#pragma clang fp contract(off)
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)m * nt) return;
    const size_t t = e / nt, i = e - t * nt;
    const double* p = P + t * ntpad + i;
    double s = p[0];
    for (int c = 1; c < split; c++) s = s + p[(size_t)c * pstride];
    mean[e] = s;
}

// Final sums of a multi-target evaluation, one workgroup.  Results row (out, and hout pinned): [0] LL = sum_t LL_t added
// in target order, [1 + c] the nh gradient components of -LL, [1 + nh + t] LL_t.
//   quad_t = z_t'z_t: wave t mod 16 takes target t -- lane l adds the squares l, l + 64, ... of row t of Z ascending, the
//     lanes by wave_sum: an order that depends neither on m nor on where the target stands
//   LL_t = -0.5 (quad_t + log|K| + n * 1.83787), log|K| the handle's own (by value: the host holds it after the evaluation)
//   isotropic (d_ard < 0): the three trace sums in finalize_sums' order (thread v adds the blocks v, v + 1024, ...
//     ascending, then the halving tree) and k_finalize's formulas; ARD: k_finalize_ard's columns, order and formulas
// A covariance that could not be factored has log|K| = NaN: every result is then NaN (the header's convention).
__global__ __launch_bounds__(FIN_THREADS) void k_finalize_targets(const double* __restrict__ Z, int npad, int n, int m,
                                                                  double logdet, const double* __restrict__ part,
                                                                  int nblocks, int d_ard, HyperScalars h_arg,
                                                                  const HyperScalars* __restrict__ hd,
                                                                  double* __restrict__ out, double* __restrict__ hout)
{
#pragma clang fp contract(off)
    const HyperScalars h = hd ? *hd : h_arg;
    const int nh = d_ard >= 0 ? d_ard + 2 : 3;
    __shared__ double red[3 * FIN_THREADS];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const bool dead = logdet != logdet;
    double* ll_each = out + 1 + nh;
    for (int tg = wave; tg < m; tg += FIN_THREADS / 64) {
        const double* zr = Z + (size_t)tg * npad;
        double q = 0.0;
        for (int i = lane; i < npad; i += 64) q = q + zr[i] * zr[i];
        q = wave_sum(q);
        if (lane == 0) ll_each[tg] = -0.5 * (q + logdet + n * 1.83787);
    }
    if (d_ard < 0) {
        double s[3] = {0.0, 0.0, 0.0};
        for (int i = t; i < nblocks; i += FIN_THREADS)
#pragma unroll
            for (int c = 0; c < 3; c++) s[c] = s[c] + part[(size_t)i * 3 + c];
#pragma unroll
        for (int c = 0; c < 3; c++) red[c * FIN_THREADS + t] = s[c];
        __syncthreads();
        for (int w = FIN_THREADS / 2; w > 0; w >>= 1) {
            if (t < w)
                for (int c = 0; c < 3; c++) red[c * FIN_THREADS + t] += red[c * FIN_THREADS + t + w];
            __syncthreads();
        }
        if (t == 0) {
            const double s1 = red[0], s2 = red[FIN_THREADS], s3 = red[2 * FIN_THREADS];
            out[1] = dead ? logdet : s1 / 2.0;
            out[2] = dead ? logdet : (2.0 * s2 - 2.0 * h.noise_var * s3) / 2.0;
            out[3] = dead ? logdet : (2.0 * h.noise_var * s3) / 2.0;
        }
    } else {
        const int d = d_ard;
        for (int c = wave; c < d + 2; c += FIN_THREADS / 64) {
            const double* col = part + (size_t)c * nblocks;
            double s = 0.0;
            for (int i = lane; i < nblocks; i += 64) s += col[i];
            s = wave_sum(s);
            if (lane == 0 && c < d) out[1 + c] = dead ? logdet : s / 2.0;
            if (lane == 0 && c >= d) red[c - d] = s;
        }
        __syncthreads();
        if (t == 0) {
            const double s2 = red[0], s3 = red[1];
            out[1 + d] = dead ? logdet : (2.0 * s2 - 2.0 * h.noise_var * s3) / 2.0;
            out[2 + d] = dead ? logdet : (2.0 * h.noise_var * s3) / 2.0;
        }
    }
    __syncthreads();
    // (the row was written by other waves of this workgroup: agent-scope loads, past the vector cache)
    double ll = 0.0;
    for (int t0 = 0; t0 < m; t0 += FIN_THREADS) {          // LL_t through LDS, FIN_THREADS at a time; thread 0 adds in target order
        __syncthreads();
        if (t0 + t < m) red[t] = __hip_atomic_load(ll_each + t0 + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        if (t == 0) {
            const int cnt = (m - t0 < FIN_THREADS) ? (m - t0) : FIN_THREADS;
            for (int i = 0; i < cnt; i++) ll = ll + red[i];
        }
    }
    if (t == 0) {
        out[0] = ll;
        hout[0] = ll;
    }
    for (int i = 1 + t; i < 1 + nh + m; i += FIN_THREADS)
        hout[i] = __hip_atomic_load(out + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ------------------------------------------------------------------------------------------
// Appending observations (cugp_append): k_append_border, k_append_kinv
// ------------------------------------------------------------------------------------------
// (needs the tile product above and cov_device.h; CUGP_DYN_LDS: the dynamic LDS of k_append_kinv's tile product)
#define CUGP_DYN_LDS(name) extern __shared__ __attribute__((aligned(16))) char name[]
#include "append_device.h"

// ------------------------------------------------------------------------------------------
// Leave-one-out cross-validation (cugp_loo): k_loo_point, k_loo_sum, k_loo_mirror_scale, k_loo_bsum, k_trace_loo,
// k_loo_finalize (loo_device.h: a host can emulate them) and the one product that needs the device, k_loo_product
// ------------------------------------------------------------------------------------------
#include "loo_device.h"

// P (lower tiles, diagonal tiles complete) = B B^T over the whole k range: lauum_tile's shape with a = 0, w = nt and a
// uniform K = ld for every tile.  Plain stores (tile_store): nothing is accumulated, no tile is touched twice.
template <int WM>
__device__ __forceinline__ void loo_product_tile(const double* __restrict__ Bm, double* __restrict__ P, int ld, int tile,
                                                 int sub, char* smem)
{
    constexpr int SUB = 4 / WM, BT = 32 * WM;
    int ti, tj;
    tri_index(tile, ti, tj);
    const int si = (sub / SUB) * BT, sj = (sub % SUB) * BT;
    d4 acc[WM][WM];
    acc_zero(acc);
    tile_nt<false>(Bm + (size_t)(ti * TILE + si) * ld, ld, Bm + (size_t)(tj * TILE + sj) * ld, ld, 0, ld, acc, smem);
    tile_store(P + (size_t)(ti * TILE + si) * ld + tj * TILE + sj, ld, acc, 1.0);
}

// k_lauum's two tile sizes: WM = 2 -- every tile as four 64x64 workgroups; WM = 4 -- the first nfull tiles as 128x128
// workgroups, the partly empty last round as 64x64 quarters (split_round)
template <int WM>
__global__ __launch_bounds__(256, 2) void k_loo_product(const double* __restrict__ Bm, double* __restrict__ P, int ld,
                                                        int nfull)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if (WM == 2) {
        loo_product_tile<2>(Bm, P, ld, blockIdx.x >> 2, blockIdx.x & 3, smem);
    } else if ((int)blockIdx.x < nfull) {
        loo_product_tile<4>(Bm, P, ld, blockIdx.x, 0, smem);
    } else {
        const int y = blockIdx.x - nfull;
        loo_product_tile<2>(Bm, P, ld, nfull + (y >> 2), y & 3, smem);
    }
}

// ------------------------------------------------------------------------------------------
// Sparse variational GP regression on inducing points (cugp_sparse_*): k_sparse_gram_finish, k_sparse_form_b,
// k_sparse_transpose, k_trace_cross, k_sparse_predict_finish (sparse_device.h: a host can emulate them) and the one new
// product, k_sparse_gram; the gradient with respect to the inducing inputs: k_trace_cross_z, k_trace_cross_z_finish
// (sparse_z_device.h, emulable as well)
// ------------------------------------------------------------------------------------------
#include "sparse_device.h"
#include "sparse_z_device.h"
// what reads the labels -- the handle's own y as one target, or p targets over the same inducing points: k_sparse_wty_targets
// and its finish, k_sparse_yy_targets, k_sparse_h_targets, k_sparse_weights_targets, k_sparse_scale_targets,
// k_sparse_finalize_targets (emulable as well)
#include "sparse_targets_device.h"
// the input gradients of the sparse prediction: k_sparse_predict_diff (emulable as well)
#include "sparse_predict_device.h"

// ---- joint predictive covariance of the sparse model (cugp_sparse_predict_cov):
//      cov = k(Xt,Xt) (+ s2 I) - (Wt Wt^T - Vt Vt^T),  Wt = Ks Lu^-T,  Vt = Wt LB^-T ----
// The sibling of k_predict_cov: the same lower BT-tiles, split of the k range, partial products to P (s = 0) or to scratch
// slot s - 1, and k_predict_cov_finish behind it unchanged.  One set of accumulators takes both products of a workgroup's
// k range, + Wt[ti] Wt[tj]^T first, then - Vt[ti] Vt[tj]^T (tile_nt<true> negates the A operand while staging it: the MFMA
// loop is the same code, no VALU work between the MFMAs is added, and the accumulators are neither stored nor reloaded in
// between).  Wt and Vt ([ntpad][ld], k_predict_gemm's outputs) are exact zeros in their columns >= m (Ks is zero there and
// the padding rows of Lu^-1 and LB^-1 are identity: DESIGN.md section 25 says so for W_c) and in their rows >= nt: relied
// on, not masked.
template <int WM>
__global__ __launch_bounds__(256, 2) void k_sparse_predict_cov(const double* __restrict__ Wt, const double* __restrict__ Vt,
                                                               int ld, int kend, int kstep, int split,
                                                               double* __restrict__ P, double* __restrict__ scr,
                                                               size_t pstride, int ldp, unsigned long long* stamp)
{
    LaunchStamp stamp_(stamp);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int BT = 32 * WM;
    const int tile = blockIdx.x / split, s = blockIdx.x % split;
    int ti, tj;
    tri_index(tile, ti, tj);
    const int k0 = s * kstep, k1 = k0 + kstep < kend ? k0 + kstep : kend;
    d4 acc[WM][WM];
    acc_zero(acc);
    tile_nt<false>(Wt + (size_t)ti * BT * ld, ld, Wt + (size_t)tj * BT * ld, ld, k0, k1, acc, smem);
    tile_nt<true>(Vt + (size_t)ti * BT * ld, ld, Vt + (size_t)tj * BT * ld, ld, k0, k1, acc, smem);
    double* C = s == 0 ? P : scr + (size_t)(s - 1) * pstride;
    tile_store(C + (size_t)ti * BT * ldp + tj * BT, ldp, acc, 1.0);
}

// acc[m][n] += sum_{k in [kbeg, kend)} W[k][i0 + ..] W[k][j0 + ..]: the TN sibling of tile_nt -- the contraction index k is
// the SLOW index of the one row-major operand W ([k][ld]; Ag -> W[0][i0], Bg -> W[0][j0]).  The LDS image, the fragment
// reads and the MFMA loop are tile_nt's (tile_stage_mma: one per-lane base + immediates, no address arithmetic between
// MFMAs); only the staging differs.  A thread takes one k PAIR (rows 2 kp, 2 kp + 1 of the stage) and one column pair per
// 64 output rows: two 16-byte loads -- the 8 lanes of a column pair read 16 B of 16 different rows, a wave 128 contiguous
// bytes of each of 16 rows, whole cache lines -- are turned in registers into the two 16-byte LDS entries
// [plane kp][row i][k even, k odd] of the columns i, i + 1.  The 8 lanes of a ds_write_b128 group hold the 8 planes of ONE
// row, 16 B apart modulo 128 (PLANE = rows * 16 + 16): no bank conflict, where lanes on consecutive rows of one plane
// (32 B apart) would pair up on every bank.  The global addresses advance by one pointer add per row and stage.
// kbeg, kend multiples of BK.  All 256 threads must call (barriers inside).
template <int WM>
__device__ __forceinline__ void tile_tn(const double* __restrict__ Ag, const double* __restrict__ Bg, int ld, int kbeg,
                                        int kend, d4 (&acc)[WM][WM], char* smem)
{
    typedef Geo<WM> G;
    constexpr int NQ = WM / 2;                            // column pairs per thread and operand: 64 rows of the tile each
    const int t = opaque_tid();
    const int lane = t & 63, wave = t >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int skp = t & 7, sip = t >> 3;
    int wa[NQ][2], wb[NQ][2];                             // LDS byte offsets of my entries
#pragma unroll
    for (int q = 0; q < NQ; q++)
#pragma unroll
        for (int e = 0; e < 2; e++) {
            const int row = 2 * (sip + 32 * q) + e;
            wa[q][e] = skp * G::PLANE + row * 16;
            wb[q][e] = G::OPER + skp * G::PLANE + bpos<WM>(row) * 16;
        }
    const int fr = lane & 15, fk = lane >> 4;
    const int abase = (fk >> 1) * G::PLANE + (wr * 16 * WM + fr) * 16 + (fk & 1) * 8;
    const int bbase = G::OPER + (fk >> 1) * G::PLANE + (wc * 16 * WM + fr) * 16 + (fk & 1) * 8;

    const int nk = (kend - kbeg) / BK;
    if (nk <= 0) return;
    const size_t step = (size_t)BK * ld;
    const double* pa0 = Ag + (size_t)(kbeg + 2 * skp) * ld + 2 * sip;
    const double* pa1 = pa0 + ld;
    const double* pb0 = Bg + (size_t)(kbeg + 2 * skp) * ld + 2 * sip;
    const double* pb1 = pb0 + ld;
    d2 ra[NQ][2], rb[NQ][2];

#define CUGP_TN_LOAD()                                                                             \
    do {                                                                                           \
        _Pragma("unroll") for (int q = 0; q < NQ; q++) {                                           \
            ra[q][0] = *(const d2*)(pa0 + 64 * q); ra[q][1] = *(const d2*)(pa1 + 64 * q);          \
            rb[q][0] = *(const d2*)(pb0 + 64 * q); rb[q][1] = *(const d2*)(pb1 + 64 * q);          \
        }                                                                                          \
        pa0 += step; pa1 += step; pb0 += step; pb1 += step;                                        \
    } while (0)
#define CUGP_TN_STORE(buf)                                                                         \
    do {                                                                                           \
        _Pragma("unroll") for (int q = 0; q < NQ; q++)                                             \
            _Pragma("unroll") for (int e = 0; e < 2; e++) {                                        \
                *(d2*)((buf) + wa[q][e]) = (d2){ra[q][0][e], ra[q][1][e]};                         \
                *(d2*)((buf) + wb[q][e]) = (d2){rb[q][0][e], rb[q][1][e]};                         \
            }                                                                                      \
    } while (0)
#define CUGP_TN_STAGE(HALF, MORE)                                                                  \
    do {                                                                                           \
        const char* cur_ = smem + (HALF) * G::STAGE;                                               \
        char* nxt_ = smem + (1 - (HALF)) * G::STAGE;                                               \
        const bool more_ = (MORE);                                                                 \
        if (more_) CUGP_TN_LOAD();                                                                 \
        tile_stage_mma<WM>(cur_, abase, bbase, acc);                                               \
        if (more_) CUGP_TN_STORE(nxt_);                                                            \
        __syncthreads();                                                                           \
    } while (0)

    CUGP_TN_LOAD();
    CUGP_TN_STORE(smem);
    __syncthreads();
    int kt = 0;
    for (; kt + 1 < nk; kt += 2) {
        CUGP_TN_STAGE(0, true);
        CUGP_TN_STAGE(1, kt + 2 < nk);
    }
    if (kt < nk) CUGP_TN_STAGE(0, false);
#undef CUGP_TN_STAGE
#undef CUGP_TN_STORE
#undef CUGP_TN_LOAD
}

// Gram product of one chunk of data rows: S_s(ti, tj) = sum_{k in split s} W[k][ti ..] W[k][tj ..] over the lower
// 128-tiles of mp x mp, W = k(X_c, Z) Lu^-T ([kend][ld], k_predict_gemm's output: exact zeros in its rows beyond the
// chunk and its columns beyond M).  Few output tiles (36 at M = 1024) and a long k: workgroup (tile, s) takes the k range
// [s kstep, min((s + 1) kstep, kend)) and writes its partial tile to scratch slot s (pstride doubles apart, ld = the
// matrix's); k_sparse_gram_finish adds the slots in index order: no atomics, the bits do not depend on which workgroup
// ends first.  Grid: lower tiles * split.
__global__ __launch_bounds__(256, 2) void k_sparse_gram(const double* __restrict__ W, int ld, int kend, int kstep,
                                                        int split, double* __restrict__ scr, size_t pstride)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tile = blockIdx.x / split, s = blockIdx.x % split;
    int ti, tj;
    tri_index(tile, ti, tj);
    const int k0 = s * kstep, k1 = k0 + kstep < kend ? k0 + kstep : kend;
    d4 acc[4][4];
    acc_zero(acc);
    tile_tn<4>(W + ti * TILE, W + tj * TILE, ld, k0, k1, acc, smem);
    tile_store(scr + (size_t)s * pstride + (size_t)ti * TILE * ld + tj * TILE, ld, acc, 1.0);
}

// ------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------
void launch_kbuild(const double* X, int n, int d, int npad, const CovFn& cf, double* K, bool full, hipStream_t s,
                   Batch bt, unsigned* tickets)
{
    const dim3 grid(tri_count(npad / KT), bt.count);
    hipLaunchKernelGGL(CUGP_COV_KERNEL(cf, k_build), grid, dim3(256), 0, s, X, n, d, npad, cf.h, cf.hd, K, full ? 1 : 0,
                       tickets, bt.tab, take_stamp());
}

void launch_sqdist(const double* X, int n, int d, int npad, double c, double* S, hipStream_t s)
{
    HyperScalars h{c, 0.0, 0.0};
    hipLaunchKernelGGL((k_build<false, KERNEL_SE>), dim3(tri_count(npad / KT)), dim3(256), 0, s, X, n, d, npad, h,
                       (const HyperScalars*)nullptr, S, 2, (unsigned*)nullptr, (const ExpertPtrs*)nullptr,
                       (unsigned long long*)nullptr);
}

void launch_kcross(const double* X, int n, int d, int npad, const double* Xt, int nt, int ntpad, const CovFn& cf,
                   double* Ks, hipStream_t s, Batch bt)
{
    const dim3 grid((ntpad / KT) * (npad / KT), bt.count);
    hipLaunchKernelGGL(CUGP_COV_KERNEL(cf, k_cross), grid, dim3(256), 0, s, X, n, d, npad, Xt, nt, ntpad, cf.h, Ks,
                       bt.tab, cf.hd);
}

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

void launch_predict_gemm(const double* Ks, const double* T, double* W, int ld, int ntt, int nt, hipStream_t s,
                         Batch bt)
{
    set_big_lds();
    // (ntt, nt in 128-row tiles; the kernel works on 64-row tiles in pairs)
    CUGP_LAUNCH(k_predict_gemm, dim3(2 * ntt * nt, bt.count), dim3(256), Geo<2>::LDS, s, Ks, T, W, ld, 2 * ntt, 2 * nt,
                take_stamp(), bt.tab);
}

CovShape predict_cov_shape(int ntpad, int n)
{
    CovShape c;
    const int aim = tune(TUNE_COV_SPLIT);                 // 64x64 workgroup slots to fill (four per CU); 0 = no split
    const int t128 = tri_count(ntpad / TILE);
    c.wm = (aim > 0 && 4 * t128 <= aim) ? 2 : 4;
    c.tiles = c.wm == 2 ? tri_count(ntpad / 64) : t128;
    c.kend = (n + BK - 1) / BK * BK;
    int split = aim / (c.wm == 2 ? 1 : 2) / c.tiles;      // (128x128 workgroups: two per CU)
    const int kmax = c.kend / 256;                        // chunks of at least 256 k
    if (split > kmax) split = kmax;
    if (split > 64) split = 64;
    const size_t pstride = (size_t)ntpad * ntpad;
    while (split > 1 && (size_t)(split - 1) * pstride * sizeof(double) > ((size_t)1 << 30)) split--;   // scratch <= 1 GiB
    if (split < 1) split = 1;
    c.kstep = ((c.kend + split - 1) / split + BK - 1) / BK * BK;
    c.split = c.kstep > 0 ? (c.kend + c.kstep - 1) / c.kstep : 1;
    if (c.split < 1) c.split = 1;
    return c;
}

void launch_predict_cov(const double* W, int ld, int ntpad, const CovShape& c, double* A, double* scr, hipStream_t s)
{
    set_big_lds();
    const size_t pstride = (size_t)ntpad * ntpad;
    if (c.wm == 2)
        CUGP_LAUNCH(k_predict_cov<2>, dim3(c.tiles * c.split), dim3(256), Geo<2>::LDS, s, W, ld, c.kend, c.kstep,
                    c.split, A, scr, pstride, ntpad, take_stamp());
    else
        CUGP_LAUNCH(k_predict_cov<4>, dim3(c.tiles * c.split), dim3(256), GEMM_LDS, s, W, ld, c.kend, c.kstep,
                    c.split, A, scr, pstride, ntpad, take_stamp());
}

void launch_predict_cov_finish(const double* Xt, int nt, int d, int ntpad, const CovFn& cf, bool with_noise,
                               double jitter, double* A, const double* scr, int nscr, unsigned* tickets, hipStream_t s)
{
    const dim3 grid(tri_count(ntpad / KT));
    hipLaunchKernelGGL(CUGP_COV_KERNEL(cf, k_predict_cov_finish), grid, dim3(256), 0, s, Xt, nt, d, ntpad, cf.h,
                       with_noise ? 1 : 0, jitter, A, scr, (size_t)ntpad * ntpad, nscr, tickets, cf.hd);
}

void launch_zero_upper_diag(double* A, int ld, int nt, hipStream_t s)
{
    hipLaunchKernelGGL(k_zero_upper_diag, dim3(nt), dim3(256), 0, s, A, ld);
}

void launch_sample_finish(const double* F, int ld, const double* mean, int nt, int ns, double* out, hipStream_t s)
{
    const size_t total = (size_t)nt * ns;
    hipLaunchKernelGGL(k_sample_finish, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, F, ld, mean, nt, ns, out);
}

void launch_predict_finish(const double* Ks, const double* W, const double* alpha, int n, int npad, int ntest,
                           HyperScalars h, double* mean, double* var, hipStream_t s, double* rows, size_t rstride,
                           int rhalf, int ntpad, Batch bt)
{
    hipLaunchKernelGGL(k_predict_finish, dim3((ntest + 3) / 4, bt.count), dim3(256), 0, s, Ks, W, alpha, n, npad,
                       ntest, h, mean, var, rows, rstride, rhalf, ntpad, bt.tab);
}

void launch_predict_grad(const double* X, int n, int d, int npad, const double* Xt, int nt, const CovFn& cf,
                         const double* Ks, const double* V, const double* alpha, double* part, size_t pstride,
                         hipStream_t s)
{
    const dim3 grid(((nt + KT - 1) / KT) * predict_grad_tiles(n));
    CUGP_LAUNCH(CUGP_COV_KERNEL(cf, k_predict_grad), grid, dim3(256), 0, s, X, n, d, npad, Xt, nt, cf.h, Ks, V, alpha, part,
                pstride, cf.hd);
}

void launch_predict_grad_finish(const double* part, size_t pstride, int n, int nt, int d, const CovFn& cf, double* dmean,
                                double* dvar, hipStream_t s)
{
    const size_t total = (size_t)nt * d;
    const double* wts = is_ard(cf) ? (const double*)(cf.hd + 1) : nullptr;   // (the weights behind the hyper-scalars)
    hipLaunchKernelGGL(k_predict_grad_finish, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, part, pstride,
                       predict_grad_tiles(n), nt, d, cf.h.ell_sq, wts, dmean, dvar);
}

// ---- the batched launches of cugp_group_predict_grad_enqueue (blockIdx.y = expert) ----
void launch_predict_finish_mv(const double* Ks, const double* W, int npad, int ntest, HyperScalars h, double* mean,
                              double* var, size_t row_stride, int ntpad, hipStream_t s, Batch bt)
{
    hipLaunchKernelGGL(k_predict_finish_mv, dim3((ntest + 3) / 4, bt.count), dim3(256), 0, s, Ks, W, npad, ntest, h, mean,
                       var, row_stride, ntpad, bt.tab);
}

void launch_targets_alpha_batched(const double* Z, double* A, int npad, int m, hipStream_t s, Batch bt)
{
    const int m64 = (m + 63) / 64, n64 = npad / 64;
    hipLaunchKernelGGL(k_targets_alpha_batched, dim3(m64 * (n64 / 2), bt.count), dim3(256), Geo<2>::LDS, s, Z, A, npad, m64,
                       n64, bt.tab);
}

void launch_predict_grad_batched(int d, int npad, const double* Xt, int nt, const CovFn& cf, const double* Ks,
                                 const double* V, size_t kslice, double* part, size_t pstride, int tiles_max,
                                 hipStream_t s, Batch bt)
{
    const dim3 grid(((nt + KT - 1) / KT) * tiles_max, bt.count);
    hipLaunchKernelGGL(CUGP_COV_KERNEL(cf, k_predict_grad_batched), grid, dim3(256), 0, s, d, npad, Xt, nt, cf.h, Ks, V,
                       kslice, part, pstride, (size_t)tiles_max * 2 * pstride, cf.hd, bt.tab);
}

void launch_predict_grad_finish_batched(const double* part, size_t pstride, int tiles_max, int nt, int d, const CovFn& cf,
                                        double* dmean, double* dvar, size_t row_stride, hipStream_t s, Batch bt)
{
    const size_t total = (size_t)nt * d;
    const double* wts = is_ard(cf) ? (const double*)(cf.hd + 1) : nullptr;   // (the weights behind the hyper-scalars)
    hipLaunchKernelGGL(k_predict_grad_finish_batched, dim3((unsigned)((total + 255) / 256), bt.count), dim3(256), 0, s, part,
                       pstride, (size_t)tiles_max * 2 * pstride, nt, d, cf.h.ell_sq, wts, dmean, dvar, row_stride, bt.tab);
}

void launch_poe_reduce_grad(const double* g, size_t rstride, int world, int K, int nt, int d, int mode, double sf2,
                            double sn2, int with_noise, int want_dvar, double* out, hipStream_t s)
{
    const size_t total = (size_t)nt * d;
    hipLaunchKernelGGL(k_poe_reduce_grad, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, g, rstride, world, K, nt,
                       d, mode, sf2, sn2, with_noise, want_dvar, out);
}

void launch_poe_reduce(const double* g, size_t rstride, int world, int K, int nt, double* out, hipStream_t s)
{
    hipLaunchKernelGGL(k_poe_reduce, dim3((nt + 255) / 256), dim3(256), 0, s, g, rstride, world, K, nt, out);
}

void launch_poe_reduce_mode(const double* g, size_t rstride, int world, int K, int nt, int mode, double sf2, double sn2,
                            int with_noise, double* out, hipStream_t s)
{
    hipLaunchKernelGGL(k_poe_reduce_mode, dim3((nt + 255) / 256), dim3(256), 0, s, g, rstride, world, K, nt, mode, sf2,
                       sn2, with_noise, out);
}

void launch_trmv_lower(const double* T, int ld, int npad, const double* x, double* z, hipStream_t s, Batch bt)
{
    hipLaunchKernelGGL(k_trmv_lower, dim3(npad / 4, bt.count), dim3(256), 0, s, T, ld, npad, x, z, bt.tab);
}

void launch_trmv_upper(const double* U, int ld, int npad, const double* x, double* a, hipStream_t s, Batch bt)
{
    hipLaunchKernelGGL(k_trmv_upper, dim3(npad / 4, bt.count), dim3(256), 0, s, U, ld, npad, x, a, bt.tab);
}

void launch_copy_y_to_w(int npad, hipStream_t s, Batch bt)
{
    hipLaunchKernelGGL(k_copy_y_to_w, dim3((npad + 255) / 256, bt.count), dim3(256), 0, s, npad, bt.tab);
}

void launch_trsv_lower(const double* A, const double* T, int ld, int nt, const double* y, double* z, hipStream_t s,
                       Batch bt)
{
    // y is consumed as the running right-hand side w (caller passes a scratch copy)
    double* w = const_cast<double*>(y);
    const int npad = nt * TILE;
    for (int kb = 0; kb < nt; kb++) {
        hipLaunchKernelGGL(k_trsv_diag, dim3(1, bt.count), dim3(256), 0, s, T, ld, kb, w, z, bt.tab);
        const int rows = npad - (kb + 1) * TILE;
        if (rows > 0)
            hipLaunchKernelGGL(k_trsv_update, dim3(rows / 4, bt.count), dim3(256), 0, s, A, ld, kb, npad, z, w, bt.tab);
    }
}

int trace_num_blocks(int npad) { return tri_count(npad / KT); }

void launch_trace(const double* X, int n, int d, int npad, const CovFn& cf, const double* Kinv, const double* alpha,
                  double* part, hipStream_t s, Batch bt, const double* z, const double* logdet_part, double* out,
                  double* hout, unsigned* ticket)
{
    const int nblocks = tri_count(npad / KT);
    const bool ard = is_ard(cf);
    // the last block takes the final sums where the launch is small (its 256 threads against k_finalize's 1024: at 8192
    // rows -- 8256 blocks -- the separate launch is as fast and keeps the blocks' stores plain); TUNE_FINALIZE_FUSE_MAX.
    // ARD: always both launches -- there is no fused form of the ARD final sums
    const bool fuse = !ard && out != nullptr && nblocks <= tune(TUNE_FINALIZE_FUSE_MAX);
    const FinalizeArgs fin{z, logdet_part, npad / TILE, fuse ? out : nullptr, hout, ticket};
    hipLaunchKernelGGL(CUGP_COV_KERNEL(cf, k_trace), dim3(nblocks, bt.count), dim3(256), 0, s, X, n, d, npad, cf.h, cf.hd,
                       Kinv, alpha, part, bt.tab, fin);
    if (ard) {
        assert(hout && (out || bt.tab));
        hipLaunchKernelGGL(k_finalize_ard, dim3(1, bt.count), dim3(FIN_THREADS), 0, s, z, npad, n, d, logdet_part,
                           npad / TILE, part, nblocks, cf.hd, out, hout, (size_t)(ARD_ROW_GRAD + d + 2), bt.tab);
    } else if (out != nullptr && !fuse) {
        launch_finalize(z, npad, n, logdet_part, npad / TILE, part, nblocks, cf.h, out, hout, s, cf.hd, bt);
    }
}

void launch_finalize(const double* z, int npad, int n, const double* logdet_part, int nt, const double* part,
                     int nblocks, HyperScalars h, double* out, double* hout, hipStream_t s, const HyperScalars* hd,
                     Batch bt)
{
    hipLaunchKernelGGL(k_finalize, dim3(1, bt.count), dim3(FIN_THREADS), 0, s, z, npad, n, logdet_part, nt, part, nblocks, h,
                       hd, out, hout, bt.tab);
}

void launch_targets_alpha(const double* Z, const double* U, double* A, int npad, int m, hipStream_t s)
{
    const int m64 = (m + 63) / 64, n64 = npad / 64;
    hipLaunchKernelGGL(k_targets_alpha, dim3(m64 * (n64 / 2)), dim3(256), Geo<2>::LDS, s, Z, U, A, npad, m64, n64);
}

void launch_trace_targets(const double* X, int n, int d, int npad, const CovFn& cf, const double* Kinv, const double* A,
                          int m, double* part, hipStream_t s)
{
    const dim3 grid(tri_count(npad / KT));
    hipLaunchKernelGGL(CUGP_COV_KERNEL(cf, k_trace_targets), grid, dim3(256), 0, s, X, n, d, npad, cf.h, Kinv, A, m, part,
                       cf.hd);
}

void launch_finalize_targets(const double* Z, int npad, int n, int d, int m, double logdet, const double* part,
                             const CovFn& cf, double* out, double* hout, hipStream_t s)
{
    hipLaunchKernelGGL(k_finalize_targets, dim3(1), dim3(FIN_THREADS), 0, s, Z, npad, n, m, logdet, part,
                       tri_count(npad / KT), is_ard(cf) ? d : -1, cf.h, is_ard(cf) ? cf.hd : nullptr, out, hout);
}

int targets_mean_split(int npad) { return (npad + TARGETS_MEAN_KSTEP - 1) / TARGETS_MEAN_KSTEP; }

void launch_targets_mean(const double* A, const double* Ks, double* P, int npad, int m, int nt, int ntpad, double* mean,
                         hipStream_t s)
{
    const int m64 = (m + 63) / 64, nt64 = (nt + 63) / 64, split = targets_mean_split(npad);
    const size_t pstride = (size_t)m64 * 64 * ntpad;
    hipLaunchKernelGGL(k_targets_mean, dim3(m64 * nt64 * split), dim3(256), Geo<2>::LDS, s, A, Ks, P, npad, m64, nt64,
                       TARGETS_MEAN_KSTEP, pstride, ntpad);
    const size_t total = (size_t)m * nt;
    hipLaunchKernelGGL(k_targets_mean_finish, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, P, pstride, split,
                       ntpad, m, nt, mean);
}

void launch_append_border(const double* P, const double* V, const double* Cf, const double* Ci, const double* flog, int r0,
                          int k, int ld, double* A, double* T, double* U, double* Kinv, const double* y, double* z,
                          double* alpha, double* logdet, double* Qt, hipStream_t s)
{
    const int nq = (r0 + 63) / 64 * (64 / APB_COLS);
    hipLaunchKernelGGL(k_append_border, dim3(nq + 1), dim3(256), 0, s, P, V, Cf, Ci, flog, r0, k, ld, nq, A, T, U, Kinv, y,
                       z, alpha, logdet, Qt);
}

void launch_append_kinv(const double* Qt, int r0, int k, int ld, double* Kinv, const double* zb, double* alpha,
                        hipStream_t s)
{
    const int n64 = (r0 + 63) / 64, lower = tri_count(n64), tiles = lower + n64 / 2, k16 = (k + BK - 1) / BK * BK;
    hipLaunchKernelGGL(k_append_kinv, dim3(tiles + (r0 + 255) / 256), dim3(256), Geo<2>::LDS, s, Qt, k16, k, r0, ld, lower,
                       tiles, Kinv, zb, alpha);
}

// ---- leave-one-out cross-validation ----
void launch_loo_point(const double* Kinv, const double* alpha, const double* y, int n, int npad, double* pt, double* out,
                      double* hout, hipStream_t s)
{
    hipLaunchKernelGGL(k_loo_point, dim3(npad / 256 + (npad % 256 ? 1 : 0)), dim3(256), 0, s, Kinv, alpha, y, n, npad, pt);
    hipLaunchKernelGGL(k_loo_sum, dim3(1), dim3(256), 0, s, (const double*)pt, npad, out, hout);
}

void launch_loo_mirror_scale(const double* Kinv, const double* pt, int n, int npad, double* Bm, double* bpart, double* b,
                             hipStream_t s)
{
    const int nb = npad / KT;
    hipLaunchKernelGGL(k_loo_mirror_scale, dim3(nb * nb), dim3(256), 0, s, Kinv, pt, n, npad, Bm, bpart);
    hipLaunchKernelGGL(k_loo_bsum, dim3(npad / 256 + (npad % 256 ? 1 : 0)), dim3(256), 0, s, (const double*)bpart, npad, b);
}

int launch_loo_product(const double* Bm, double* P, int npad, hipStream_t s)
{
    set_big_lds();
    const int tiles = tri_count(npad / TILE);
    if (tiles <= tune(TUNE_LAUUM_WM2_MAX)) {
        CUGP_LAUNCH(k_loo_product<2>, dim3(tiles * 4), dim3(256), Geo<2>::LDS, s, Bm, P, npad, 0);
        return 2;
    }
    const int nfull = split_round(tiles, 1);                 // (uniform K: a short last round is worth splitting)
    CUGP_LAUNCH(k_loo_product<4>, dim3(nfull + 4 * (tiles - nfull)), dim3(256), GEMM_LDS, s, Bm, P, npad, nfull);
    return 4;
}

void launch_trace_loo(const double* X, int n, int d, int npad, const CovFn& cf, const double* P, const double* alpha,
                      const double* b, double* part, double* out, double* hout, hipStream_t s)
{
    const int nblocks = tri_count(npad / KT);
    hipLaunchKernelGGL(CUGP_COV_KERNEL(cf, k_trace_loo), dim3(nblocks), dim3(256), 0, s, X, n, d, npad, cf.h, cf.hd, P, alpha,
                       b, part);
    hipLaunchKernelGGL(k_loo_finalize, dim3(1), dim3(256), 0, s, (const double*)part, nblocks, is_ard(cf) ? d : 1,
                       cf.h.noise_var, out, hout);
}

// ---- sparse variational GP regression on inducing points ----
SparseShape sparse_shape(int n, int mpad, int chunk_rows, int pass)
{
    SparseShape c;
    const int rows = chunk_rows > 0 ? chunk_rows : SPARSE_CHUNK_DEFAULT;
    c.chunks = (int)(((long long)n + rows - 1) / rows);
    c.r0 = (int)((long long)pass * rows < n ? (long long)pass * rows : n);
    c.count = n - c.r0 < rows ? n - c.r0 : rows;
    c.cpad = (c.count + TILE - 1) / TILE * TILE;
    const int tiles = tri_count(mpad / TILE);
    int split = SPARSE_GRAM_SLOTS / tiles;                // (128x128 workgroups, two per CU)
    const int kmax = c.cpad / 256;                        // chunks of at least 256 k
    if (split > kmax) split = kmax;
    if (split > 64) split = 64;
    const size_t pstride = (size_t)mpad * mpad;
    while (split > 1 && (size_t)split * pstride * sizeof(double) > ((size_t)1 << 30)) split--;   // scratch <= 1 GiB
    if (split < 1) split = 1;
    c.kstep = ((c.cpad + split - 1) / split + BK - 1) / BK * BK;
    c.split = c.kstep > 0 ? (c.cpad + c.kstep - 1) / c.kstep : 1;
    if (c.split < 1) c.split = 1;
    return c;
}

void launch_sparse_gram(const double* W, int mpad, const SparseShape& c, double* P, double* scr, bool first, hipStream_t s)
{
    set_big_lds();
    const int tiles = tri_count(mpad / TILE);
    const size_t pstride = (size_t)mpad * mpad;
    CUGP_LAUNCH(k_sparse_gram, dim3(tiles * c.split), dim3(256), GEMM_LDS, s, W, mpad, c.cpad, c.kstep, c.split, scr,
                pstride);
    hipLaunchKernelGGL(k_sparse_gram_finish, dim3(tiles * 16), dim3(256), 0, s, P, mpad, (const double*)scr, pstride,
                       c.split, first ? 1 : 0);
}

void launch_sparse_form_b(const double* P, int mpad, double s2, double* Bm, hipStream_t s)
{
    hipLaunchKernelGGL(k_sparse_form_b, dim3(tri_count(mpad / TILE) * 16), dim3(256), 0, s, P, mpad, s2, Bm);
}

void launch_sparse_transpose(const double* src, double* dst, int mpad, double scale, hipStream_t s)
{
    const int nb = mpad / KT;
    hipLaunchKernelGGL(k_sparse_transpose, dim3(nb * nb), dim3(256), 0, s, src, dst, mpad, scale);
}

void launch_sparse_weights(const double* W, const double* R, double* G, int cpad, int mpad, hipStream_t s)
{
    launch_test_gemm_nt(W, R, G, cpad, mpad, mpad, s);       // k_test_gemm: the plain NT product on the tile
}

void launch_trace_cross(const double* Xr, int nr, int rows_pad, const double* Z, int m, int d, int mpad, const CovFn& cf,
                        const double* G, const double* yv, const double* bv, double* part, size_t pstride, size_t pofs,
                        hipStream_t s)
{
    const dim3 grid((rows_pad / KT) * (mpad / KT));
    hipLaunchKernelGGL(CUGP_COV_KERNEL(cf, k_trace_cross), grid, dim3(256), 0, s, Xr, nr, Z, m, d, mpad, cf.h, cf.hd, G, yv,
                       bv, part, pstride, pofs);
}

SparseZShape sparse_z_shape(int rows_pad, int mpad, int d)
{
    SparseZShape z;
    z.row_tiles = rows_pad / KT;
    const int nct = mpad / KT;
    int ranges = SPARSE_Z_SLOTS / nct;                    // (64-column workgroups, two per CU)
    if (ranges > rows_pad / 256) ranges = rows_pad / 256; // ranges of at least 256 rows, as the Gram product's splits
    if (ranges < 1) ranges = 1;
    while (ranges > 1 && (size_t)ranges * mpad * d * sizeof(double) > ((size_t)1 << 30)) ranges--;   // scratch <= 1 GiB
    z.per = (z.row_tiles + ranges - 1) / ranges;
    z.ranges = (z.row_tiles + z.per - 1) / z.per;         // (no empty range)
    return z;
}

void launch_trace_cross_z(const double* Xr, int nr, int rows_pad, const double* Z, int m, int d, int mpad, const CovFn& cf,
                          const double* G, const double* yv, const double* bv, double* part, double* acc, bool first,
                          bool last, double* out, double* hout, hipStream_t s)
{
    const SparseZShape z = sparse_z_shape(rows_pad, mpad, d);
    const size_t sstride = (size_t)m * d;
    hipLaunchKernelGGL(CUGP_COV_KERNEL(cf, k_trace_cross_z), dim3((mpad / KT) * z.ranges), dim3(256), 0, s, Xr, nr, Z, m, d,
                       mpad, cf.h, cf.hd, G, yv, bv, z.row_tiles, z.per, z.ranges, part, sstride);
    const double* wts = is_ard(cf) ? (const double*)(cf.hd + 1) : nullptr;   // (the weights behind the hyper-scalars)
    hipLaunchKernelGGL(k_trace_cross_z_finish, dim3((unsigned)((sstride + 255) / 256)), dim3(256), 0, s, (const double*)part,
                       sstride, z.ranges, m, d, first ? 1 : 0, last ? 1 : 0, cf.h.ell_sq, wts, acc, out, hout);
}

void launch_sparse_predict_finish(const double* Wt, const double* Vt, const double* cp, int mpad, int nt, double sf2,
                                  double s2, double noise, double* mean, double* var, hipStream_t s)
{
    hipLaunchKernelGGL(k_sparse_predict_finish, dim3((nt + 3) / 4), dim3(256), 0, s, Wt, Vt, cp, mpad, nt, sf2, s2, noise,
                       mean, var);
}

// ---- joint covariance and input gradients of the sparse prediction ----
void launch_sparse_predict_cov(const double* Wt, const double* Vt, int ld, int ntpad, const CovShape& c, double* A,
                               double* scr, hipStream_t s)
{
    set_big_lds();
    const size_t pstride = (size_t)ntpad * ntpad;
    if (c.wm == 2)
        CUGP_LAUNCH(k_sparse_predict_cov<2>, dim3(c.tiles * c.split), dim3(256), Geo<2>::LDS, s, Wt, Vt, ld, c.kend, c.kstep,
                    c.split, A, scr, pstride, ntpad, take_stamp());
    else
        CUGP_LAUNCH(k_sparse_predict_cov<4>, dim3(c.tiles * c.split), dim3(256), GEMM_LDS, s, Wt, Vt, ld, c.kend, c.kstep,
                    c.split, A, scr, pstride, ntpad, take_stamp());
}

void launch_sparse_predict_diff(const double* Wt, const double* T, double* D, int mpad, int rows, const double* bp, double s2,
                                int m, double* a, hipStream_t s)
{
    const size_t total = std::max<size_t>(D ? (size_t)rows * mpad : 0, (size_t)mpad);
    hipLaunchKernelGGL(k_sparse_predict_diff, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, Wt, T, D, mpad, rows, bp,
                       s2, m, a);
}

// ---- multi-target regression over one set of inducing points ----
void launch_sparse_wty_targets(const double* W, int mpad, int cpad, const double* Y, size_t ystride, int p, double* part,
                               double* Q, bool first, hipStream_t s)
{
    const int slabs = cpad / TILE, groups = (p + SPT_GROUP - 1) / SPT_GROUP;
    hipLaunchKernelGGL(k_sparse_wty_targets, dim3((unsigned)((mpad / KT) * slabs) * groups), dim3(256), 0, s, W, mpad, slabs, Y,
                       ystride, p, part);
    hipLaunchKernelGGL(k_sparse_wty_targets_finish, dim3((unsigned)p * ((mpad + 255) / 256)), dim3(256), 0, s,
                       (const double*)part, slabs, mpad, p, Q, first ? 1 : 0);
}

void launch_sparse_yy_targets(const double* Y, size_t ystride, int n, int p, double* out, hipStream_t s)
{
    hipLaunchKernelGGL(k_sparse_yy_targets, dim3(p), dim3(256), 0, s, Y, ystride, n, out);
}

void launch_sparse_h_targets(const double* Binv, const double* P, const double* Gm, const double* Bt, int p, int m, int mpad,
                             double s2, double* H, double* H2, double* Bs, hipStream_t s)
{
    const int nb = mpad / KT;
    hipLaunchKernelGGL(k_sparse_h_targets, dim3(nb * nb), dim3(256), 0, s, Binv, P, Gm, Bt, p, m, mpad, s2, H, H2, Bs);
}

void launch_sparse_weights_targets(double* G, int cpad, int mpad, const double* Y, size_t ystride, const double* Bs, int p,
                                   int nr, int m, hipStream_t s)
{
    hipLaunchKernelGGL(k_sparse_weights_targets, dim3((cpad / KT) * (mpad / KT)), dim3(256), 0, s, G, mpad, Y, ystride, Bs, p,
                       nr, m);
}

void launch_sparse_scale_targets(const double* Cm, int p, int rows, int m, int mpad, double s2, double* Cs, hipStream_t s)
{
    const size_t total = (size_t)rows * mpad;
    hipLaunchKernelGGL(k_sparse_scale_targets, dim3((unsigned)std::min<size_t>((total + 255) / 256, 4096)), dim3(256), 0, s, Cm,
                       p, rows, m, mpad, s2, Cs);
}

void launch_sparse_finalize_targets(const SparseFinalTargets& f, const double* part_uf, size_t nb_uf, const double* part_uu,
                                    size_t nb_uu, int nl, double* out, double* hout, hipStream_t s)
{
    hipLaunchKernelGGL(k_sparse_finalize_targets, dim3(1), dim3(256), 0, s, f, part_uf, nb_uf, part_uu, nb_uu, nl, out, hout);
}

void launch_test_gemm_nt(const double* A, const double* B, double* C, int m, int n, int k, hipStream_t s)
{
    set_big_lds();
    hipLaunchKernelGGL(k_test_gemm, dim3((m / TILE) * (n / TILE)), dim3(256), GEMM_LDS, s, A, B, C, n, k, m / TILE);
}

void launch_mfma_peak(double* sink, int blocks, int iters, hipStream_t s)
{
    hipLaunchKernelGGL(k_mfma_peak, dim3(blocks), dim3(256), 0, s, sink, iters);
}

}  // namespace cugp
