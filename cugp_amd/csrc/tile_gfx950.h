// tile_gfx950.h -- the fp64 MFMA tile product every dense stage runs through: the geometry and its LDS sizes (BK, Geo,
// GEMM_LDS), the NT product on four waves (tile_nt) and on eight (tile_nt8) with their epilogues, the TN product
// (tile_tn), the split-K planner of the launches with few output tiles (plan_ksplit), and the two kernels that are
// nothing but the product: k_test_gemm and k_mfma_peak, each with its launcher.
//
// Include-point contract.  Needs the device; also holds launchers.  Included by kernels.hip alone, INSIDE namespace cugp,
// after these are declared -- the file includes nothing and declares none of them:
//   kernels.h        TILE, the launcher prototypes
//   kernels.hip      d2, d4, set_big_lds; with -DCUGP_TILE_STAMPS the stamps' globals are defined here
// Every *_gfx950.h and append_device.h below it use what it declares.
#pragma once

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

// Split-K plan of a product with too few output tiles to fill the chip (predict_cov_shape, sparse_shape): the k range
// [0, kend) in `split` chunks of kstep for as many workgroups per tile.  split on entry: the workgroup slots to fill divided
// by the tiles; chunks of at least 256 k, at most 64 of them, and the partial tiles in scratch (slot_bytes each; all of them, or
// all but the first when chunk 0 lands in place) within 1 GiB.  kstep is whole stages of BK and split is what it leaves.
struct KSplit { int kstep, split; };
static KSplit plan_ksplit(int kend, int split, size_t slot_bytes, bool first_in_place)
{
    const int kmax = kend / 256;
    if (split > kmax) split = kmax;
    if (split > 64) split = 64;
    while (split > 1 && (size_t)(split - (first_in_place ? 1 : 0)) * slot_bytes > ((size_t)1 << 30)) split--;
    if (split < 1) split = 1;
    KSplit p;
    p.kstep = ((kend + split - 1) / split + BK - 1) / BK * BK;
    p.split = p.kstep > 0 ? (kend + p.kstep - 1) / p.kstep : 1;
    if (p.split < 1) p.split = 1;
    return p;
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

void launch_test_gemm_nt(const double* A, const double* B, double* C, int m, int n, int k, hipStream_t s)
{
    set_big_lds();
    hipLaunchKernelGGL(k_test_gemm, dim3((m / TILE) * (n / TILE)), dim3(256), GEMM_LDS, s, A, B, C, n, k, m / TILE);
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

void launch_mfma_peak(double* sink, int blocks, int iters, hipStream_t s)
{
    hipLaunchKernelGGL(k_mfma_peak, dim3(blocks), dim3(256), 0, s, sink, iters);
}
