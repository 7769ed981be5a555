// chol_gfx950.h -- the blocked right-looking Cholesky: the panel solve with the forward substitution that rides in it
// (k_trsm_inv64), the 128x128 diagonal block in LDS (potf2_body, k_potf2), the step launch that updates the near window
// and factors the next diagonal block (k_syrk_step), the wide far update (k_syrk_wide, k_syrk_wide8, k_syrk_wide_rest);
// each launcher directly behind its kernel, so the grid a launcher builds and the blockIdx decoding of its kernel are one
// screen apart.
//
// Include-point contract.  Needs the device; also holds launchers.  Included by kernels.hip alone, INSIDE namespace cugp,
// after these are declared -- the file includes nothing and declares none of them:
//   kernels.h        TILE, ExpertPtrs, Batch, SUBPANEL_MAX, tune and the TUNE_* keys, the launcher prototypes
//   kernels.hip      d2, d4, GP, WGT and the WGT_* kinds, LaunchStamp, CUGP_LAUNCH, take_stamp, tri_count, set_big_lds
//   cov_device.h     tri_index, wave_sum
//   tile_gfx950.h    Geo, GEMM_LDS, tile_nt, tile_nt8 and their epilogues
// Declares for inverse_gfx950.h: MT, TRTRI_LDS, mt_off, micro_mma_nn, micro_mma_acc_b, micro_store; for the other uniform-K
// launchers (inverse_gfx950.h, launch_loo_product in dense_features_gfx950.h): split_round.
#pragma once

// diagonal-block kernels work on 16x16 micro tiles (one MFMA tile)
constexpr int MT = 16;                             // micro tile (one MFMA tile)
constexpr int MTS = MT * (MT + 1);                 // doubles per LDS micro tile, rows padded to 17
constexpr int NMT = TILE / MT;                     // 8 micro tiles per edge
constexpr int NLT = NMT * (NMT + 1) / 2;           // 36 lower micro tiles
constexpr int POTF2_LDS = (NLT * MTS + TILE) * 8;  // tiles + 1/L_ii  = 79360 B
static_assert(POTF2_LDS == 79360, "dynamic LDS of the diagonal-block Cholesky");

// Tiles (ti >= tj) of the tile columns [0, wcol) of a lower triangle, row by row: row r holds min(r + 1, wcol)
// tiles.  idx -> (ti, tj), both relative to the region's first column.  wcol >= the triangle's size gives the
// whole triangle (tri_index).
__device__ __forceinline__ void trap_index(int idx, int wcol, int& ti, int& tj)
{
    const int head = wcol * (wcol + 1) / 2;
    if (idx < head) { tri_index(idx, ti, tj); return; }
    const int rem = idx - head;
    ti = wcol + rem / wcol;
    tj = rem % wcol;
}

// ------------------------------------------------------------------------------------------
// panel solve with the two 64x64 diagonal inverses (T00, T11) of the factor block: per 16-row strip
//   X0 = A0 T00^T ;  Z1 = A1 - X0 L10^T ;  X1 = Z1 T11^T
// One workgroup of EIGHT waves per strip.  Everything is kept transposed, so a result in C/D layout is the next
// product's B operand (k = (lane>>4) + 4*reg) and passes from wave to wave through LDS as it stands.
// Round 3: the three 64x64 matrices and the strip come into LDS with coalesced 16-byte loads (L10 and T11 wait in
// registers until the buffer is free) and the MFMA operands are read from there.  The strip used to load every
// operand from global memory in MFMA layout -- 16 rows x 32 bytes per instruction, 68 such loads per lane, 96 KB of
// inverses per strip: ~280 MB of L2 sector traffic for a 63-tile panel, which took the launch 17-20 us (round-3
// timeline) on the factorisation's serial path; and each of the three dependent MFMA chains (<= 16 long) ran on one
// wave per SIMD at 138 cycles per MFMA.  Now wave (w, h) takes the k sub-ranges r in {2h, 2h+1} of column tile w:
// chains of <= 8, the two waves of a SIMD (w, w+4) interleaving at the pipe's full rate; the two halves meet in LDS.
// ------------------------------------------------------------------------------------------
constexpr int TRSM_TS = 68;                          // row stride (doubles) of the 64x64 matrix in LDS: rows 4 doubles apart mod 32
constexpr int TRSM_SS = 132;                         // ... of the 16 x 128 strip
constexpr int TRSM_LDS = (64 * TRSM_TS + MT * TRSM_SS + 3 * 4 * 4 * 64) * 8;   // + half sums, X0^T, Z1^T: 76288 B
static_assert(TRSM_LDS == 76288, "dynamic LDS of the panel solve");

// ---- forward substitution L z = y folded into the factorisation's own launches (round 5; LL-only evaluations) ----
// z_kb = L_kk^-1 w_kb needs only block kb of the factor and the running right-hand side w; w_i -= L(i,kb) z_kb for the
// rows below needs only the solved column kb.  Both ride in launches the factorisation makes anyway: ONE extra
// workgroup of the panel solve of column kb computes z_kb from the block's two 64x64 inverses (zblock_solve: z0 = T00
// w0, z1 = T11 (w1 - L10 z0)), and nt - kb - 1 extra workgroups of the step launch of column kb apply it to w
// (vec_update: one wave per row, the per-row order of k_trsv_update).  What used to follow the factorisation as 2 nt
// small launches (0.56 ms of a 5.5 ms log-likelihood at 8192 rows, 0.10 of 0.54 ms at 1500) is one 1-workgroup launch
// for the last block.
__device__ __forceinline__ void zblock_solve(const double* __restrict__ A, const double* __restrict__ d64, int ld, int kb,
                                             const double* __restrict__ w, double* __restrict__ z, double* __restrict__ sm)
{
    // 512 threads: row r = t >> 3 of a 64-row half, column group cg = t & 7 (8 columns each), partial sums over the 8
    // lanes of a row in a fixed order
    const int t = threadIdx.x, r = t >> 3, cg = t & 7, k0 = kb * TILE;
    double* w0 = sm;                                     // w_kb: [0, 64) upper half, [64, 128) lower half
    double* z0 = sm + 128;
    double* tt = sm + 192;
    const double* T00 = d64 + (size_t)kb * 8192;
    const double* T11 = T00 + 4096;
    const double* L10 = A + (size_t)(k0 + 64) * ld + k0;
    // every operand this thread will touch is requested before the first wait: one memory latency for the three
    // dependent products (requested phase by phase the workgroup took ~12 us and held the panel-solve launch -- on the
    // factorisation's chain -- 5 us longer than its strips)
    const int cend = (r | 15) + 1;
    double a0[8], a1[8], a2[8];
    const double wmine = t < TILE ? w[k0 + t] : 0.0;
#pragma unroll
    for (int q = 0; q < 8; q += 2) {
        const int c = cg * 8 + q;
        const d2 v0 = *(const d2*)(T00 + r * 64 + c), v1 = *(const d2*)(L10 + (size_t)r * ld + c), v2 = *(const d2*)(T11 + r * 64 + c);
        // (the 64x64 inverses hold their lower 16x16 micro tiles only: what lies beyond the row's own micro tile is
        //  never written -- selected away, not multiplied by zero; inside a diagonal micro tile the entries above the
        //  diagonal are exact zeros)
        a0[q] = c < cend ? v0[0] : 0.0; a0[q + 1] = c + 1 < cend ? v0[1] : 0.0;
        a1[q] = v1[0]; a1[q + 1] = v1[1];
        a2[q] = c < cend ? v2[0] : 0.0; a2[q + 1] = c + 1 < cend ? v2[1] : 0.0;
    }
    if (t < TILE) w0[t] = wmine;
    __syncthreads();
    auto row_sum = [&](double s) {
        s += __shfl_xor(s, 1, 64);
        s += __shfl_xor(s, 2, 64);
        s += __shfl_xor(s, 4, 64);
        return s;
    };
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < 8; q++) s = __builtin_fma(a0[q], w0[cg * 8 + q], s);
    s = row_sum(s);
    if (cg == 0) z0[r] = s;
    __syncthreads();
    s = 0.0;
#pragma unroll
    for (int q = 0; q < 8; q++) s = __builtin_fma(a1[q], z0[cg * 8 + q], s);
    s = row_sum(s);
    if (cg == 0) tt[r] = w0[64 + r] - s;
    __syncthreads();
    s = 0.0;
#pragma unroll
    for (int q = 0; q < 8; q++) s = __builtin_fma(a2[q], tt[cg * 8 + q], s);
    s = row_sum(s);
    if (cg == 0) { z[k0 + r] = z0[r]; z[k0 + 64 + r] = s; }
}

// w[row] -= L[row][k0 .. k0 + 128) . z[k0 ..) for the 128 rows of tile row `ti` (one wave per row, 32 rows per wave of a
// 256-thread workgroup): k_trsv_update's arithmetic
__device__ __forceinline__ void vec_update(const double* __restrict__ A, int ld, int kb, int ti, const double* __restrict__ z,
                                           double* __restrict__ w)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, k0 = kb * TILE;
    const d2 xv = *(const d2*)(z + k0 + lane * 2);
    const double* a = A + (size_t)(ti * TILE + wave * 32) * ld + k0 + lane * 2;
    // all 32 rows of the wave requested before the first is reduced (row by row the loop was one memory latency per
    // row: ~45 us per workgroup, longer than the diagonal block the step launch hides)
    d2 v[32];
#pragma unroll
    for (int q = 0; q < 32; q++) v[q] = *(const d2*)(a + (size_t)q * ld);
    double mine = 0.0;                                   // lane q ends up with row q's sum
#pragma unroll
    for (int q = 0; q < 32; q++) {
        double sum = v[q][0] * xv[0] + v[q][1] * xv[1];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_down(sum, o, 64);
        const double tot = __shfl(sum, 0, 64);
        if (lane == q) mine = tot;
    }
    if (lane < 32) {
        double* wr = w + ti * TILE + wave * 32 + lane;
        *wr -= mine;
    }
}

// zv / wv (when given): the forward substitution rides along -- workgroup `nstrips` of the launch computes z_kb
__global__ __launch_bounds__(512) void k_trsm_inv64(double* __restrict__ A, const double* __restrict__ d64,
                                                    int ld, int kb, const ExpertPtrs* __restrict__ bt,
                                                    unsigned long long* stamp, int nstrips, double* __restrict__ zvec,
                                                    const double* __restrict__ wvec)
{
    LaunchStamp stamp_(stamp);
    if (bt) {
        A = GP(bt[blockIdx.y].A); d64 = GP(bt[blockIdx.y].d64);
        if (zvec) { zvec = GP(bt[blockIdx.y].z); wvec = GP(bt[blockIdx.y].w); }
    }
    extern __shared__ __attribute__((aligned(16))) double sm[];
    // (zvec given: workgroup 0 -- dispatched first -- is the vector workgroup, the strips follow)
    const int strip = zvec ? (int)blockIdx.x - 1 : (int)blockIdx.x;
    if (strip < 0) {
        zblock_solve(A, d64, ld, kb, wvec, zvec, sm);
        return;
    }
    double* Tm = sm;                                    // T00, then -L10, then T11
    double* Sb = Tm + 64 * TRSM_TS;                     // the strip: A in, X out (row-major)
    double* Sc = Sb + MT * TRSM_SS;                     // half sums of the waves h = 1: [w][r][lane]
    double* X0 = Sc + 4 * 4 * 64;                       // X0^T tiles as B operands: [kt][r][lane]
    double* Z1 = X0 + 4 * 4 * 64;
    WGT(wgt_, WGT_TRSM, kb);
    __builtin_amdgcn_s_setprio(3);                      // on the factorisation's serial chain (see k_syrk_step)
    const int t = threadIdx.x, lane = t & 63, wv = __builtin_amdgcn_readfirstlane(t >> 6);
    const int w = wv & 3, h = wv >> 2, c = lane & 15, g = lane >> 4;
    const int k0 = kb * TILE;
    double* Ag = A + (size_t)(k0 + TILE + strip * MT) * ld + k0;
    const double* T00 = d64 + (size_t)kb * 8192;
    const double* T11 = T00 + 4096;
    const double* L10 = A + (size_t)(k0 + 64) * ld + k0;
    // coalesced requests for everything the strip will read: 4 chunks of 16 B per thread and 64x64 matrix, 2 of the strip
    d2 rt[4], rl[4], r1[4], ra[2];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int q = t + 512 * i, row = q >> 5, cp = (q & 31) * 2;
        rt[i] = *(const d2*)(T00 + row * 64 + cp);
        rl[i] = *(const d2*)(L10 + (size_t)row * ld + cp);
        r1[i] = *(const d2*)(T11 + row * 64 + cp);
    }
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int q = t + 512 * i, row = q >> 6, cp = (q & 63) * 2;
        ra[i] = *(const d2*)(Ag + (size_t)row * ld + cp);
    }
    auto fill_tm = [&](const d2 (&r)[4], double sign) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int q = t + 512 * i, row = q >> 5, cp = (q & 31) * 2;
            *(d2*)(Tm + row * TRSM_TS + cp) = sign * r[i];
        }
    };
    fill_tm(rt, 1.0);
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int q = t + 512 * i, row = q >> 6, cp = (q & 63) * 2;
        *(d2*)(Sb + row * TRSM_SS + cp) = ra[i];
    }
    __syncthreads();
    const d4 zero4 = (d4){0.0, 0.0, 0.0, 0.0};
    const double* tm = Tm + (w * MT + c) * TRSM_TS + g + 8 * h;        // my row of the matrix, my k sub-range
    // acc += sum over the k tiles kt < nkt of M[w][kt] (from Tm) times the B tiles bop[kt][r][lane], r in {2h, 2h+1}
    auto chain = [&](d4 acc, const double* bop, int nkt) {
#pragma unroll
        for (int kt = 0; kt < 4; kt++)
            if (kt < nkt) {
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(tm[kt * MT], bop[(kt * 4 + 2 * h) * 64 + lane], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(tm[kt * MT + 4], bop[(kt * 4 + 2 * h + 1) * 64 + lane], acc, 0, 0, 0);
            }
        return acc;
    };
    // phase 1: X0^T[w] = sum_{kt <= w} T00[w][kt] A0^T[kt]   (B operand straight from the strip: A0[row c][k])
    d4 x = zero4;
#pragma unroll
    for (int kt = 0; kt < 4; kt++)
        if (kt <= w) {
            x = __builtin_amdgcn_mfma_f64_16x16x4f64(tm[kt * MT], Sb[c * TRSM_SS + kt * MT + g + 8 * h], x, 0, 0, 0);
            x = __builtin_amdgcn_mfma_f64_16x16x4f64(tm[kt * MT + 4], Sb[c * TRSM_SS + kt * MT + g + 8 * h + 4], x, 0, 0, 0);
        }
    if (h == 1) {
#pragma unroll
        for (int r = 0; r < 4; r++) Sc[(w * 4 + r) * 64 + lane] = x[r];
    }
    __syncthreads();                                    // T00 and A0 have been read; the half sums are in LDS
    d4 z = zero4;
    if (h == 0) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const double v = x[r] + Sc[(w * 4 + r) * 64 + lane];
            X0[(w * 4 + r) * 64 + lane] = v;
            Sb[c * TRSM_SS + w * MT + g + 4 * r] = v;                   // X0 is final: into the strip, over A0
            z[r] = Sb[c * TRSM_SS + 64 + w * MT + g + 4 * r];           // A1^T[w]
        }
    }
    fill_tm(rl, -1.0);
    __syncthreads();
    // phase 2: Z1^T[w] = A1^T[w] - sum_kt L10[w][kt] X0^T[kt]
    z = chain(z, X0, 4);
    if (h == 1) {
#pragma unroll
        for (int r = 0; r < 4; r++) Sc[(w * 4 + r) * 64 + lane] = z[r];
    }
    __syncthreads();
    if (h == 0) {
#pragma unroll
        for (int r = 0; r < 4; r++) Z1[(w * 4 + r) * 64 + lane] = z[r] + Sc[(w * 4 + r) * 64 + lane];
    }
    fill_tm(r1, 1.0);
    __syncthreads();
    // phase 3: X1^T[w] = sum_{kt <= w} T11[w][kt] Z1^T[kt]
    d4 x1 = chain(zero4, Z1, w + 1);
    if (h == 1) {
#pragma unroll
        for (int r = 0; r < 4; r++) Sc[(w * 4 + r) * 64 + lane] = x1[r];
    }
    __syncthreads();
    if (h == 0) {
#pragma unroll
        for (int r = 0; r < 4; r++) Sb[c * TRSM_SS + 64 + w * MT + g + 4 * r] = x1[r] + Sc[(w * 4 + r) * 64 + lane];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; i++) {                       // the solved strip back to global memory, whole rows
        const int q = t + 512 * i, row = q >> 6, cp = (q & 63) * 2;
        *(d2*)(Ag + (size_t)row * ld + cp) = *(const d2*)(Sb + row * TRSM_SS + cp);
    }
}

void launch_trsm_inv64(double* A, const double* d64, int ld, int kb, int nt, hipStream_t s, Batch bt, double* zv,
                       const double* wv)
{
    const int nstrips = (nt - kb - 1) * (TILE / MT);
    if (nstrips <= 0 && !zv) return;                      // (kb = nt - 1 with zv: the last block's z alone)
    set_big_lds();
    hipLaunchKernelGGL(k_trsm_inv64, dim3(nstrips + (zv ? 1 : 0), bt.count), dim3(512), TRSM_LDS, s, A, d64, ld, kb, bt.tab,
                       take_stamp(), nstrips, zv, wv);
}

// ------------------------------------------------------------------------------------------
// diagonal block: 128x128 Cholesky in LDS (one workgroup), 16-wide inner blocks
// ------------------------------------------------------------------------------------------
constexpr int TRTRI_LDS = NLT * MTS * 8;             // the 36 lower micro tiles
static_assert(TRTRI_LDS == 78336, "dynamic LDS of the diagonal-tile inverse");

// ---- helpers for the diagonal block ------------------------------------------------------

__device__ __forceinline__ int mt_off(int bi, int bj) { return (bi * (bi + 1) / 2 + bj) * MTS; }

// broadcast of one lane's double through SGPRs (v_readlane x2); `src` must be wave-uniform
__device__ __forceinline__ double readlane_f64(double v, int src)
{
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(u & 0xffffffffull), src);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(u >> 32), src);
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

// 1/sqrt(x): v_rsq_f64 seed + two Newton steps; x <= 0 or NaN gives NaN/Inf that flows on
__device__ __forceinline__ double rsqrt_nr(double x)
{
    double y = __builtin_amdgcn_rsq(x);
#pragma unroll
    for (int it = 0; it < 2; it++) {
        const double e = __builtin_fma(-x * y, y, 1.0);
        y = __builtin_fma(0.5 * y, e, y);
    }
    return y;
}

// workgroup barrier that orders LDS traffic only: global stores in flight are NOT waited for (a __syncthreads
// would be: ~2k cycles at every barrier once the factored diagonal tiles go straight to global memory)
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// ---- panel factor: Cholesky of one 16x16 micro tile held in LDS (rows padded to 17) together with everything that
// hangs on it, by up to three waves side by side.  Lane l < 16 of every wave owns row l of the diagonal tile in
// registers (each wave factors the tile for itself: no hand-over between waves inside the pivot loop), right-looking.
// Every instruction of the loop runs on all 64 lanes, so lanes 16..63 carry OTHER ROWS through the same elimination
// for free: rows of the column block below the diagonal tile (48 per wave) come out as x = a L_jj^-T, and 16 lanes
// that start from the rows of the IDENTITY come out as the columns of L_jj^-1.
// One wave issues an fp64 VALU instruction per ~5.5-6.5 cycles and a dependent one per ~8.3, so the loop -- the
// latency floor of the whole factorisation -- is written for a short dependent chain and few instructions (round 3;
// measured by tools/panel_bench.hip: 16 pivots in 2.8k cycles, 175 per pivot; the round-2 loop: 4.2k, 265 per pivot):
//   * the pivot recurrence is in LDL^T form: the rank-1 update is  r[j] -= (m_i / d) m_j  with the UNSCALED column m,
//     which is final when the pivot starts -- its trip through LDS (one ds_write, uniform 16-byte reads back by all
//     64 lanes) starts at once and hides behind the rsq chain (the Cholesky form scales the column by 1/sqrt(d)
//     first, so that trip started at the END of the chain and its update had to wait a pivot);
//   * 1/sqrt(d): v_rsq_f64 seed (2^-24) + ONE third-order step y0 (1 + e/2 + 3e^2/8), e = 1 - d y0^2 (error
//     5/16 e^3 ~ 3e-24: below rounding); the stored factor is x = m y as before, m / d = x y;
//   * the chain per pivot: rsq, 5 polish ops, x, x y, ONE fma on column c+1, ONE readlane pair for the next pivot
//     (m_(c+1), the other operand of that fma, came back from LDS a pivot ago);
//   * software-pipelined by hand (one wave issues in order): the next pivot's v_rsq goes out first, the bulk of the
//     previous pivot's update (columns >= c+1) fills its latency and the gaps between the polish ops;
//   * every lane parks its column entry with ONE unmasked ds_write per pivot: rows of the diagonal tile into the
//     wave's column buffer, passenger rows into dead slots of their own LDS row (element 0, rewritten at the end, and
//     the pad element 16: the +128-byte immediate that alternates the two column buffers stays inside the 17-double
//     row), identity rows into parking slots of their own.  Spare lanes repeat rows (same values to the same
//     addresses) instead of being masked off.
// Two calls with a workgroup barrier between them: panel_load (everybody reads the diagonal tile) and panel_factor
// (the owner's rows go straight to global memory, the inverse replaces the diagonal tile in LDS).
struct PanelLanes {
    double* myrow;      // LDS row this lane loads from (rows of the factor: also where it stores to)
    double* wslot;      // where the lane parks its column entry at every pivot
    double* icol;       // identity rows: column `idx` of the diagonal tile in LDS (row stride MT + 1), else unused
    int kind;           // 0 row of the diagonal tile, 1 row of the column block below, 2 identity row
};

// zz: 64 doubles of LDS: [0, 32) a delta vector (1.0 at index 15: identity row i reads its 16 entries from zz + 15 - i,
// no selects), [32, 64) the parking slots of the identity rows.
// ident: this wave carries the 16 identity rows in its first spare lanes (the caller picks the wave with >= 16 of them):
// row i comes out as column i of L_jj^-1 -- the 16x16 inverse the 64x64 inverses are built from -- for free, every
// instruction of the pivot loop runs on all 64 lanes anyway.  The remaining spare lanes repeat rows (block rows, or the
// identity rows when the wave holds no block rows): same values to the same addresses.
__device__ __forceinline__ void panel_load(double* __restrict__ sm, int jb, int nrows, int q0, bool ident,
                                            double* colbuf, double* zz, PanelLanes& pl, double (&r)[MT])
{
    const int lane = threadIdx.x & 63;
    int nv = nrows - q0;                                       // block rows this wave holds: 0, 16, 32 or 48
    nv = nv < 0 ? 0 : (nv > 48 ? 48 : nv);
    int l = lane - MT;                                         // lanes >= 16: position among the wave's 48 passenger rows
    double* diagtile = sm + mt_off(jb, jb);
    if (lane < MT) {
        pl.kind = 0;
        pl.myrow = diagtile + lane * (MT + 1);
        pl.wslot = colbuf + lane;
        pl.icol = diagtile;
    } else {
        bool isid = ident && l >= nv && l < nv + MT;
        if (!isid && l >= nv) {                                // spare lane: repeat a block row, or an identity row
            if (nv > 0) { l -= nv; if (l >= nv) l -= nv; if (l >= nv) l -= nv; }
            else isid = true;
        }
        if (isid) {
            const int idx = (l - nv) & (MT - 1);
            pl.kind = 2;
            pl.myrow = zz + (MT - 1) - idx;
            pl.wslot = zz + 2 * MT + idx;
            pl.icol = diagtile + idx;
        } else {
            const int q = q0 + l;
            pl.kind = 1;
            pl.myrow = sm + mt_off(jb + 1 + (q >> 4), jb) + (q & 15) * (MT + 1);
            pl.wslot = pl.myrow;
            pl.icol = diagtile;
        }
    }
#pragma unroll
    for (int c = 0; c < MT; c++) r[c] = pl.myrow[c];
}

// arrive / arrive_target (when arrive_target > 0: several waves factor this panel): every factoring wave counts itself
// in *arrive once its copy of the diagonal tile is in registers; the wave with the identity rows overwrites the tile
// in LDS with the inverse only after it has seen all of them (a bounded wait that is over long before it is reached:
// the store comes 16 pivots after the loads) -- no workgroup barrier between panel_load and panel_factor.
__device__ __forceinline__ void panel_factor(const PanelLanes& pl, double (&r)[MT], double* __restrict__ gdiag, int ld,
                                              double* __restrict__ rinv, const double* colbuf, unsigned* arrive,
                                              unsigned arrive_target)
{
    // (colbuf is written through pl.wslot: no __restrict__)
    // Software-pipelined by hand, one wave issues in order: the next pivot's v_rsq goes out FIRST, the bulk of the
    // previous pivot's rank-1 update (columns >= c+1, operands long since back from LDS) fills its latency, then the
    // polish and the one fma + readlane pair that give the next pivot; as soon as column c+1 is final its LDS trip
    // and the broadcast of m_(c+2) start.  sched_barriers keep the compiler from sinking the bulk in front of the rsq.
    const int lane = threadIdx.x & 63;
    double piv = readlane_f64(r[0], 0);
    if (arrive_target > 0) {
        // (r[15], the last value panel_load asked for, is in its register: LDS returns a wave's reads in order)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (lane == 0) __hip_atomic_fetch_add(arrive, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    double ys[MT];
    d2 mm[2][MT / 2];                                  // uniform column entries m_j of the pivot in flight / the one before
    double ltp = 0.0;                                  // -(m / d) of the previous pivot
    pl.wslot[0] = r[0];
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#pragma unroll
    for (int c2 = 0; c2 < MT; c2 += 2) mm[0][c2 / 2] = *(const d2*)(colbuf + c2);
#define CUGP_SB __builtin_amdgcn_sched_barrier(0)
    // k-th fma of the previous pivot's bulk update (columns c+1 .. 15, column c+1 first: the chain needs it)
#define CUGP_BULK(k)                                                                                       \
    do {                                                                                                   \
        if (c >= 1 && c + 1 + (k) < MT) {                                                                  \
            const int j_ = c + 1 + (k);                                                                    \
            r[j_] = __builtin_fma(ltp, mm[(c - 1) & 1][j_ / 2][j_ & 1], r[j_]);                            \
            CUGP_SB;                                                                                       \
        }                                                                                                  \
    } while (0)
#pragma unroll
    for (int c = 0; c < MT; c++) {
        const int nb = c >= 1 ? MT - 1 - c : 0;        // fmas of the previous pivot's bulk
        const int pre = nb > 7 ? nb - 7 : (nb < 3 ? nb : 3);   // in the shadow of the rsq; the rest one per chain op
        const double y0 = __builtin_amdgcn_rsq(piv);
        CUGP_SB;
#pragma unroll
        for (int k = 0; k < pre; k++) CUGP_BULK(k);
        const double t = -piv * y0;
        CUGP_SB;
        CUGP_BULK(pre + 0);
        const double e = __builtin_fma(t, y0, 1.0);
        CUGP_SB;
        CUGP_BULK(pre + 1);
        const double h = __builtin_fma(e, 0.375, 0.5);
        CUGP_SB;
        CUGP_BULK(pre + 2);
        const double qq = e * h;
        CUGP_SB;
        CUGP_BULK(pre + 3);
        const double y = __builtin_fma(y0, qq, y0);
        CUGP_SB;
        CUGP_BULK(pre + 4);
        const double x = r[c] * y;
        CUGP_SB;
        CUGP_BULK(pre + 5);
        const double lt = -x * y;                      // -(m / d)
        CUGP_SB;
        CUGP_BULK(pre + 6);
        ys[c] = y;
        if (c + 1 < MT) {
            r[c + 1] = __builtin_fma(lt, mm[c & 1][(c + 1) / 2][(c + 1) & 1], r[c + 1]);   // m_(c+1): back from LDS a pivot ago
            CUGP_SB;
            piv = readlane_f64(r[c + 1], c + 1);       // next pivot
            pl.wslot[((c + 1) & 1) * MT] = r[c + 1];   // column c+1 is final: on its way
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#pragma unroll
            for (int c2 = (c + 2) & ~1; c2 < MT; c2 += 2) mm[(c + 1) & 1][c2 / 2] = *(const d2*)(colbuf + ((c + 1) & 1) * MT + c2);
        }
        r[c] = x;
        ltp = lt;
        CUGP_SB;
    }
#undef CUGP_BULK
#undef CUGP_SB
    if (pl.kind == 1) {
#pragma unroll
        for (int c = 0; c < MT; c++) pl.myrow[c] = r[c];
    } else if (pl.kind == 2) {
        // my row is column idx of L_jj^-1: the inverse replaces the diagonal tile in LDS (the factor itself goes to
        // global memory from the owner's registers)
        // (unbounded: the waves counted are co-resident waves of this workgroup, each of which counts itself right
        //  after its loads -- a bounded wait that fell through would overwrite the tile under a wave still loading it
        //  and give a silently wrong factor)
        if (arrive_target > 0)
            while (__hip_atomic_load(arrive, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < arrive_target)
                __builtin_amdgcn_s_sleep(1);
#pragma unroll
        for (int c = 0; c < MT; c++) pl.icol[c * (MT + 1)] = r[c];
    } else if (pl.kind == 0 && gdiag) {                                  // the owner wave: the factor's diagonal tile is final
        double* g = gdiag + (size_t)lane * ld;
        // (entries above the diagonal of a diagonal micro tile are never read on the device, and cugp_get_cholesky
        //  zeroes the strict upper triangle on the host: no masking)
#pragma unroll
        for (int c = 0; c < MT; c += 2) *(d2*)(g + c) = (d2){r[c], r[c + 1]};
        if (lane == 0) {
#pragma unroll
            for (int c = 0; c < MT; c += 2) *(d2*)(rinv + c) = (d2){ys[c], ys[c + 1]};
        }
    }
}

// C(bi,bj) -= sum_{p in [p0, p1)} X(bi,p) X(bj,p)^T on LDS micro tiles, one wave, NT tiles (bi, bi+1, .. of one
// column) side by side: every finished panel the tiles still lack in ONE pass over them (4 MFMAs per tile and panel,
// two accumulation chains each; the next panel's operands are requested before the current one's MFMAs, whose issue
// time (~550 cycles per tile from one wave) covers the LDS latency).  A tile alone pays ~400 cycles of prologue and
// epilogue (operand latency, the wait for its last MFMA before the store); two side by side share them -- the first
// tile's sums and stores issue while the second's MFMAs are still in flight.
template <int NT, int NP>   // NP = p1 - p0 panels, unrolled (as a rolled loop the compiler carried the accumulators in
                            // VGPRs and copied all of them to the MFMA's AGPRs and back on every trip)
__device__ __forceinline__ void micro_update_np(double* __restrict__ sm, int bi, int bj, int p0)
{
    const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
    double* C[NT];
    const double* Xi[NT];
    const double* Xj = sm + mt_off(bj, p0) + c * (MT + 1) + g;          // tiles (b, p), (b, p+1) are MTS doubles apart
    d4 acc[NT], acc2[NT];
    double a[NP][NT][4], b[NP][4];
#pragma unroll
    for (int s = 0; s < 4; s++) b[0][s] = Xj[4 * s];
#pragma unroll
    for (int n = 0; n < NT; n++) {
        C[n] = sm + mt_off(bi + n, bj);
        Xi[n] = sm + mt_off(bi + n, p0) + c * (MT + 1) + g;
#pragma unroll
        for (int s = 0; s < 4; s++) a[0][n][s] = -Xi[n][4 * s];
#pragma unroll
        for (int r = 0; r < 4; r++) acc[n][r] = C[n][(g + 4 * r) * (MT + 1) + c];
        acc2[n] = (d4){0.0, 0.0, 0.0, 0.0};
    }
#pragma unroll
    for (int p = 0; p < NP; p++) {
        if (p + 1 < NP) {                                                // next panel's operands on their way
#pragma unroll
            for (int s = 0; s < 4; s++) b[p + 1][s] = Xj[(p + 1) * MTS + 4 * s];
#pragma unroll
            for (int n = 0; n < NT; n++)
#pragma unroll
                for (int s = 0; s < 4; s++) a[p + 1][n][s] = -Xi[n][(p + 1) * MTS + 4 * s];
        }
#pragma unroll
        for (int n = 0; n < NT; n++) {
            acc[n] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[p][n][0], b[p][0], acc[n], 0, 0, 0);
            acc2[n] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[p][n][1], b[p][1], acc2[n], 0, 0, 0);
        }
#pragma unroll
        for (int n = 0; n < NT; n++) {
            acc[n] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[p][n][2], b[p][2], acc[n], 0, 0, 0);
            acc2[n] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[p][n][3], b[p][3], acc2[n], 0, 0, 0);
        }
    }
#pragma unroll
    for (int n = 0; n < NT; n++)
#pragma unroll
        for (int r = 0; r < 4; r++) C[n][(g + 4 * r) * (MT + 1) + c] = acc[n][r] + acc2[n][r];
}

template <int NT>
__device__ __forceinline__ void micro_update_multi(double* __restrict__ sm, int bi, int bj, int p0, int p1)
{
    switch (p1 - p0) {
    case 1: micro_update_np<NT, 1>(sm, bi, bj, p0); break;
    case 2: micro_update_np<NT, 2>(sm, bi, bj, p0); break;
    case 3: micro_update_np<NT, 3>(sm, bi, bj, p0); break;
    case 4: micro_update_np<NT, 4>(sm, bi, bj, p0); break;
    case 5: micro_update_np<NT, 5>(sm, bi, bj, p0); break;
    case 6: micro_update_np<NT, 6>(sm, bi, bj, p0); break;
    default: break;
    }
}

// The same for NB tiles at once (tile n of the step = the n-th of (bj = jb+1.., bi = bj..7) in that order): all
// operands of the batch are requested before the first MFMA and the NB x 4 MFMAs are independent, so the LDS
// latency and the MFMA latency of one tile hide behind the others (one tile at a time took ~1100 cycles, 4 MFMAs
// of 64).  Tiles past the end of the step (n >= ntiles) are skipped wave-uniformly.
template <int NB>
__device__ __forceinline__ void micro_update_batch(double* __restrict__ sm, int jb, int n0, int stride, int nend)
{
    const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
    const int mm = NMT - 1 - jb;                       // tiles per edge of the trailing part
    double* C[NB];
    const double *Xi[NB], *Xj[NB];
    bool on[NB];
#pragma unroll
    for (int b = 0; b < NB; b++) {
        const int n = __builtin_amdgcn_readfirstlane(n0 + b * stride);
        on[b] = n < nend;
        // n -> (column cj, row ri) of the trailing lower triangle, column by column: column cj holds mm - cj tiles
        int cj = 0, rem = on[b] ? n : 0;
        while (rem >= mm - cj) { rem -= mm - cj; cj++; }
        const int bj = jb + 1 + cj, bi = bj + rem;
        C[b] = sm + mt_off(bi, bj);
        Xi[b] = sm + mt_off(bi, jb);
        Xj[b] = sm + mt_off(bj, jb);
    }
    d4 acc[NB], acc2[NB];
    double xa[NB][4], xb[NB][4];
#pragma unroll
    for (int b = 0; b < NB; b++) {
#pragma unroll
        for (int r = 0; r < 4; r++) acc[b][r] = C[b][(g + 4 * r) * (MT + 1) + c];
#pragma unroll
        for (int s = 0; s < 4; s++) {
            xa[b][s] = -Xi[b][c * (MT + 1) + 4 * s + g];
            xb[b][s] = Xj[b][c * (MT + 1) + 4 * s + g];
        }
        acc2[b] = (d4){0.0, 0.0, 0.0, 0.0};
    }
    // every operand of the batch is on its way before the first MFMA waits for one (left alone the scheduler
    // interleaves loads and MFMAs tile by tile with a full LDS wait in front of each)
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int s = 0; s < 4; s += 2)
#pragma unroll
        for (int b = 0; b < NB; b++) {
            acc[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[b][s], xb[b][s], acc[b], 0, 0, 0);
            acc2[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[b][s + 1], xb[b][s + 1], acc2[b], 0, 0, 0);
        }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int b = 0; b < NB; b++)
        if (on[b]) {
#pragma unroll
            for (int r = 0; r < 4; r++) C[b][(g + 4 * r) * (MT + 1) + c] = acc[b][r] + acc2[b][r];
        }
}

// tiles n = n0, n0 + stride, ... < nend of step jb's rank-16 update by the calling wave, four at a time
__device__ __forceinline__ void micro_update_run(double* __restrict__ sm, int jb, int n0, int stride, int nend)
{
    for (int n = n0; n < nend; n += 4 * stride) {
        if (n + 2 * stride < nend) micro_update_batch<4>(sm, jb, n, stride, nend);
        else if (n + stride < nend) micro_update_batch<2>(sm, jb, n, stride, nend);
        else micro_update_batch<1>(sm, jb, n, stride, nend);
    }
}

// ------------------------------------------------------------------------------------------
// diagonal block: 128x128 Cholesky by one workgroup.  The lower triangle lives in LDS as 36
// padded 16x16 micro tiles (78 KiB: fits beside one resident MFMA workgroup on the CU).
// Per 16-wide inner step: (A) micro_factor of the diagonal micro tile in registers (one wave),
// (B) the rows below by per-row forward substitution (L_jj broadcast from LDS), (C) rank-16
// update of the remaining micro tiles with MFMA -- wave 0 takes the next diagonal tile first and
// factors it while waves 1..3 finish the update (look-ahead inside the block).
// Outputs: L (lower) back into A, the 16x16 diagonal inverses (d16, used by the panel solve and
// the inverse), and this block's share of log|K|.
// ------------------------------------------------------------------------------------------
#ifdef CUGP_STAMPS   // diagnostic build only (tools/chain_bench.hip): cycle stamps of wave 0 into a side buffer
__device__ unsigned long long g_stamps[128];
#define WSTAMP(i)                                                                  \
    do {                                                                           \
        if ((threadIdx.x & 63) == 0) {                                             \
            unsigned long long t_;                                                 \
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory"); \
            g_stamps[i] = t_;                                                      \
        }                                                                          \
    } while (0)
#define STAMP(i)                                                                   \
    do {                                                                           \
        if (threadIdx.x == 0) {                                                    \
            unsigned long long t_;                                                 \
            asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory"); \
            g_stamps[i] = t_;                                                      \
        }                                                                          \
    } while (0)
#else
#define STAMP(i)
#define WSTAMP(i)
#endif

// one MFMA 16x16x16 product on LDS micro tiles, "NN": acc += A(tile a)[row][k] * B(tile b)[k][col]
__device__ __forceinline__ d4 micro_mma_nn(const double* __restrict__ a, const double* __restrict__ b, d4 acc)
{
    const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
#pragma unroll
    for (int s = 0; s < 4; s++)
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[c * (MT + 1) + 4 * s + g], b[(4 * s + g) * (MT + 1) + c], acc, 0,
                                                   0, 0);
    return acc;
}

// acc -= A(tile a)[row][k] * W[k][col] where W is a previous MFMA result held in registers (C/D layout):
// register r of lane (col, g) is W[g + 4r][col], i.e. already the B operand for k = g + 4r
__device__ __forceinline__ d4 micro_mma_acc_b(const double* __restrict__ a, d4 w, d4 acc)
{
    const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
#pragma unroll
    for (int r = 0; r < 4; r++)
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-a[c * (MT + 1) + g + 4 * r], w[r], acc, 0, 0, 0);
    return acc;
}

__device__ __forceinline__ void micro_store(double* __restrict__ tile, d4 v)
{
    const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
#pragma unroll
    for (int r = 0; r < 4; r++) tile[(g + 4 * r) * (MT + 1) + c] = v[r];
}

// Which finished panels the helper waves (the ones not factoring) bring into which micro tiles while panel q is being
// factored.  Column q+1 gets ALL panels older than q in one pass over its tiles, one phase before it is needed (panel q
// itself follows in U1, by every wave, as soon as it exists): 4q MFMAs per tile, at most 24 per helper wave -- the
// ~3.3k cycles one wave needs to issue them fit under the ~3.5k cycles of the 16 pivots, in every phase.  (The
// right-looking order this replaces gave the two helper waves of the first phases 21 and 15 tiles: 9k and 7k cycles.)
// Two range tasks per (phase, helper): rows [bi0, bi1] of column bj take panels [p0, p1); 15 bits each.
__device__ __forceinline__ unsigned helper_tasks(int q, int h)
{
#define CUGP_T(bi0, bi1, bj, p0, p1) ((unsigned)((bi0) | (bi1) << 3 | (bj) << 6 | (p0) << 9 | (p1) << 12))
    switch (q * 4 + h) {
    case 1 * 4 + 0: return CUGP_T(3, 7, 2, 0, 1);                                      // 20 MFMAs (the only helper; tile (2,2) rode in U1(0))
    case 2 * 4 + 0: return CUGP_T(3, 5, 3, 0, 2);                                      // 24
    case 2 * 4 + 1: return CUGP_T(6, 7, 3, 0, 2) | CUGP_T(7, 7, 5, 0, 2) << 16;        // 16 + 8 (ahead of phase 4)
    case 3 * 4 + 0: return CUGP_T(4, 5, 4, 0, 3);                                      // 24
    case 3 * 4 + 1: return CUGP_T(6, 7, 4, 0, 3);                                      // 24
    case 4 * 4 + 0: return CUGP_T(5, 5, 5, 0, 4) | CUGP_T(7, 7, 5, 2, 4) << 16;        // 16 + 8
    case 4 * 4 + 1: return CUGP_T(6, 6, 5, 0, 4);                                      // 16
    case 5 * 4 + 0: return CUGP_T(6, 6, 6, 0, 5);                                      // 20
    case 5 * 4 + 1: return CUGP_T(7, 7, 6, 0, 5);                                      // 20
    case 6 * 4 + 0: return CUGP_T(7, 7, 7, 0, 6);                                      // 24
    default: return 0u;
    }
#undef CUGP_T
}

template <bool HANDED = false>   // HANDED: the block was written by other workgroups of this launch (agent-scope loads)
__device__ __forceinline__ void potf2_body(double* __restrict__ Ab, int ld, double* __restrict__ d16blk,
                                           double* __restrict__ d64blk, double* __restrict__ logdet_out,
                                           double* __restrict__ sm, double* __restrict__ red)
{
    double* rinv = sm + NLT * MTS;                          // 1 / L_ii, 128 entries
    double* colbuf = red;                                   // pivot columns: 2 x 16 doubles for each of the 4 waves
    double* zz = red + TILE;                                // delta vector + parking slots of the identity rows (panel_load)
    unsigned* arrive = (unsigned*)(zz + 2 * MT - 1);        // factoring waves that hold their copy of the diagonal tile (panel_factor)
    unsigned arrived = 0;                                   // ... expected once every wave of the phases so far has counted itself
    (void)d16blk;                                           // (16x16 inverses live in LDS only)
    // (the wave index through readfirstlane: the compiler then knows that everything decided by it -- which tiles
    //  a wave updates, which rows it factors -- is wave-uniform and keeps that control flow on the scalar unit)
    const int t = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    __builtin_amdgcn_s_setprio(3);                          // this workgroup is the critical path of the step

    STAMP(0);
    {   // load the lower micro tiles; thread t = element (t>>4, t&15) of every tile.  All 36 loads in flight before
        // the first LDS store (fully unrolled; as a rolled loop they went out a few at a time: 3.9k cycles)
        const int r = t >> 4, c = t & 15;
        double v[NLT];
#pragma unroll
        for (int bi = 0; bi < NMT; bi++)
#pragma unroll
            for (int bj = 0; bj <= bi; bj++) {
                const double* src = Ab + (size_t)(bi * MT + r) * ld + bj * MT + c;
                v[bi * (bi + 1) / 2 + bj] = HANDED ? __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : *src;
            }
#pragma unroll
        for (int q = 0; q < NLT; q++) sm[q * MTS + r * (MT + 1) + c] = v[q];
        if (t < 2 * MT) zz[t] = t == MT - 1 ? 1.0 : 0.0;    // (zz[31], never read as a double, is the arrival counter: 0)
    }
    __syncthreads();
    STAMP(1);
    // Phase q = 0..7:  P(q) panel factor of micro-tile column q -- the diagonal tile, the rows below it (48 per wave)
    // and 16 identity rows that come out as the tile's 16x16 inverse (panel_load / panel_factor) -- by waves 0..iw,
    // iw = rows / 48: the last of them is the one with >= 16 spare lanes (or holds the identity rows alone).  Beside
    // it the other waves run H(q): the older panels into column q+1 (helper_tasks).  Then U1(q), every wave: panel q
    // into column q+1, and on to P(q+1).
    // (barriers in this loop order LDS traffic only -- lds_barrier: the diagonal tiles' global stores drain behind them)
    PanelLanes pl;
    double pr[MT];
    double* gblk = Ab;                                       // global home of the 128x128 block (row stride ld)
    const d4 zero4 = (d4){0.0, 0.0, 0.0, 0.0};
    d4 hw0 = zero4, hw1 = zero4;                            // products a helper wave carries across a barrier
    // one off-diagonal micro tile of the factor back to global memory, by one wave (its LDS home is about to be
    // overwritten by a piece of an inverse, or the wave has nothing else to do)
    auto store_tile = [&](int bi, int bj) {
        const int lane = t & 63, r = lane >> 3, c = (lane & 7) * 2;             // two adjacent entries per lane: 16-byte stores
        const double* src = sm + mt_off(bi, bj) + r * (MT + 1) + c;
        double* dst = Ab + (size_t)(bi * MT + r) * ld + bj * MT + c;
#pragma unroll
        for (int k = 0; k < 2; k++)
            *(d2*)(dst + (size_t)(8 * k) * ld) = (d2){src[8 * k * (MT + 1)], src[8 * k * (MT + 1) + 1]};
    };
    // 16 -> 32: T21 = -T_B (L21 T_A) for the pair of diagonal micro tiles a = 2p, b = 2p + 1, in place of tile (b,a)
    auto pair_double = [&](int p2) {
        const int a = 2 * p2, b = 2 * p2 + 1;
        store_tile(b, a);
        const d4 w = micro_mma_nn(sm + mt_off(b, a), sm + mt_off(a, a), zero4);
        const d4 t21 = micro_mma_acc_b(sm + mt_off(b, b), w, zero4);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        micro_store(sm + mt_off(b, a), t21);
    };
    // 32 -> 64 of 64-block h, column bj of its lower-left 2x2 micro tiles, first half:
    // W(kb', bj) = sum_{jb' >= bj} C(kb', jb') T_A(jb', bj)  (reads only)
    auto block_w = [&](int h, int bj, d4& w0, d4& w1) {
        const int a0 = 4 * h, b0 = 4 * h + 2;
        w0 = zero4; w1 = zero4;
        for (int jp = bj; jp < 2; jp++) {
            w0 = micro_mma_nn(sm + mt_off(b0, a0 + jp), sm + mt_off(a0 + jp, a0 + bj), w0);
            w1 = micro_mma_nn(sm + mt_off(b0 + 1, a0 + jp), sm + mt_off(a0 + jp, a0 + bj), w1);
        }
    };
    // ... second half: T(b0 + i, a0 + bj) = -sum_{k <= i} T_B(i, k) W(k, bj)  (t0, t1 still to be stored)
    auto block_t = [&](int h, const d4& w0, const d4& w1, d4& t0, d4& t1) {
        const int b0 = 4 * h + 2;
        t0 = micro_mma_acc_b(sm + mt_off(b0, b0), w0, zero4);
        t1 = micro_mma_acc_b(sm + mt_off(b0 + 1, b0), w0, zero4);
        t1 = micro_mma_acc_b(sm + mt_off(b0 + 1, b0 + 1), w1, t1);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    };
    auto block_store = [&](int h, int bj, const d4& t0, const d4& t1) {
        micro_store(sm + mt_off(4 * h + 2, 4 * h + bj), t0);
        micro_store(sm + mt_off(4 * h + 3, 4 * h + bj), t1);
    };
    // one 64x64 inverse to global, row-major (micro tiles above the diagonal are never read), by nw waves from wave w0
    auto store_d64 = [&](int h, int w0, int nw) {
        const int u = t - w0 * 64, nth = nw * 64;
#pragma unroll 5
        for (int q = 0; q < 10; q++) {
            const int bi = q < 1 ? 0 : (q < 3 ? 1 : (q < 6 ? 2 : 3)), bj = q - bi * (bi + 1) / 2;
            for (int e = u; e < 128; e += nth) {                                // 128 pairs of adjacent entries per tile
                const int r = e >> 3, c = (e & 7) * 2;
                const double* src = sm + mt_off(4 * h + bi, 4 * h + bj) + r * (MT + 1) + c;
                *(d2*)(d64blk + (size_t)h * 4096 + (bi * MT + r) * 64 + bj * MT + c) = (d2){src[0], src[1]};
            }
        }
    };
    for (int q = 0; q < NMT; q++) {
        const int rows = (NMT - 1 - q) * MT, iw = rows / 48;
        if (wave <= iw) {
            panel_load(sm, q, rows, wave * 48, wave == iw, colbuf + wave * 2 * MT, zz, pl, pr);
            double* gd = wave == 0 ? gblk + (size_t)q * MT * ld + q * MT : nullptr;
            panel_factor(pl, pr, gd, ld, rinv + q * MT, colbuf + wave * 2 * MT, arrive, iw > 0 ? arrived + iw + 1 : 0u);
        } else {
            const int h = wave - iw - 1;
            unsigned code = helper_tasks(q, h);
            for (; code & 0x7fffu; code >>= 16) {
                const int bi1 = code >> 3 & 7, bj = code >> 6 & 7, p0 = code >> 9 & 7, p1 = code >> 12 & 7;
                int bi = code & 7;
                for (; bi + 1 <= bi1; bi += 2) micro_update_multi<2>(sm, bi, bj, p0, p1);
                if (bi <= bi1) micro_update_multi<1>(sm, bi, bj, p0, p1);
            }
            // The spare time of the helpers in the last phases goes to what used to follow the factorisation: the
            // finished columns of the factor back to global memory, and the doubling of the 16x16 inverses
            // (16 -> 32 -> 64) as far as the finished diagonal tiles allow.  A tile is stored before a piece of an
            // inverse takes its place in LDS; every such piece is read only from the next phase on (barriers between).
            if (q == 4 && h == 1) pair_double(0);
            if (q == 5) {                                           // columns 0..3 of the factor are final
                if (h == 2) {
#pragma nounroll
                    for (int bj = 0; bj < 2; bj++)
#pragma unroll 3
                        for (int bi = 2; bi < NMT; bi++) store_tile(bi, bj);    // ((1,0) went out with its pair in phase 4)
                    pair_double(1);                                 // (stores (3,2) itself)
                } else {
                    const int bj = 2 + h;                           // h = 0: column 2 below (3,2); h = 1: column 3
#pragma unroll 4
                    for (int bi = 4; bi < NMT; bi++) store_tile(bi, bj);
                }
            }
            if (q == 6 && h >= 1) {                                 // 64-block 0: column bj = h - 1
                block_w(0, h - 1, hw0, hw1);
                d4 t0, t1;
                block_t(0, hw0, hw1, t0, t1);
                // column 0 at once (wave h = 2 reads only column 1 of these tiles); column 1 after the barrier
                // (wave h = 1 reads it)
                if (h == 1) block_store(0, 0, t0, t1);
                else { hw0 = t0; hw1 = t1; }
            }
            if (q == 7) {
                if (h == 0) { pair_double(2); block_w(1, 0, hw0, hw1); }      // (4,5), then W(., 0) of 64-block 1
                if (h == 1) { block_w(1, 1, hw0, hw1); store_d64(0, 2, 1); }
                if (h == 2) {
                    store_tile(6, 4); store_tile(7, 4); store_tile(6, 5); store_tile(7, 5); store_tile(7, 6);
                    hw0 = micro_mma_nn(sm + mt_off(7, 6), sm + mt_off(6, 6), zero4);   // first half of the pair (6,7)
                    // log-determinant share of the first seven diagonal tiles: sum_i log(1/L_ii), i < 112, fixed order
                    const int lane = t & 63;
                    double v = log(rinv[lane]) + (lane < 48 ? log(rinv[lane + 64]) : 0.0);
#pragma unroll
                    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
                    if (lane == 0) colbuf[3 * 2 * MT] = v;          // (this wave's column buffer is idle: it never factors)
                }
            }
        }
        if (iw > 0) arrived += iw + 1;
        WSTAMP(64 + q * 4 + wave);                         // (diagnostic build: when each wave reaches the barrier)
        lds_barrier();
        STAMP(2 + 2 * q);
        if (q == 6 && wave == 3) block_store(0, 1, hw0, hw1);
        if (q + 1 < NMT) {
            // U1: panel q into column q+1 = tiles 0 .. m-1 of its update (phase 0: and tile (2,2), for the one wave
            // that would otherwise hold a single tile)
            micro_update_run(sm, q, wave, 4, NMT - 1 - q + (q == 0 ? 1 : 0));
            lds_barrier();
        }
        STAMP(3 + 2 * q);
    }
    lds_barrier();                                          // the last tile's inverse is in LDS
    STAMP(30);
    // what is left of the inverses: second half of the pair (6,7), then of 64-block 1 (its W came from phase 7)
    if (wave == 3) {
        const d4 t21 = micro_mma_acc_b(sm + mt_off(7, 7), hw0, zero4);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        micro_store(sm + mt_off(7, 6), t21);
    }
    // log-determinant share of this block: sum_i log L_ii = -sum_i log(1/L_ii); the last tile's 16 terms join the
    // partial sum of phase 7 (fixed order)
    if (wave == 0) {
        const int lane = t & 63;
        double v = lane < MT ? log(rinv[TILE - MT + lane]) : 0.0;
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        if (lane == 0) *logdet_out = -(colbuf[3 * 2 * MT] + v);
    }
    lds_barrier();
    STAMP(31);
    if (wave == 1 || wave == 2) {
        d4 t0, t1;
        block_t(1, hw0, hw1, t0, t1);
        block_store(1, wave - 1, t0, t1);
    }
    lds_barrier();
    STAMP(32);
    store_d64(1, 0, 4);
    STAMP(33);
}

__global__ __launch_bounds__(256) void k_potf2(double* __restrict__ A, int ld, int kb, double* __restrict__ d16,
                                               double* __restrict__ d64, double* __restrict__ logdet_part,
                                               const ExpertPtrs* __restrict__ bt)
{
    if (bt) { A = GP(bt[blockIdx.y].A); d16 = GP(bt[blockIdx.y].d16); d64 = GP(bt[blockIdx.y].d64); logdet_part = GP(bt[blockIdx.y].logdet); }
    extern __shared__ __attribute__((aligned(16))) double sm[];
    __shared__ double red[TILE + 4 * MT];
    potf2_body(A + (size_t)kb * TILE * ld + kb * TILE, ld, d16 + (size_t)kb * NMT * (MT * MT),
               d64 + (size_t)kb * 8192, logdet_part + kb, sm, red);
}

void launch_potf2(double* A, int ld, int kb, double* d16, double* d64, double* logdet_part, hipStream_t s, Batch bt)
{
    set_big_lds();
    hipLaunchKernelGGL(k_potf2, dim3(1, bt.count), dim3(256), POTF2_LDS, s, A, ld, kb, d16, d64, logdet_part, bt.tab);
}

// one 16x16 micro tile of A(kb+1,kb+1) -= sum_{k in [ks, kb]} L(kb+1,k) L(kb+1,k)^T by ONE workgroup, operands straight
// from L2: the four waves take a quarter of the k range each (8 MFMAs per k tile in two chains; one wave issues an fp64
// MFMA per ~138 cycles, so the whole K = 128 on one wave was 32 x 138 = 4.4k cycles of the chain), partial sums through
// LDS, added in a fixed order by wave 0, which stores the tile write-through (the consumer is another workgroup).
// NK = kb + 1 - ks k tiles (sub-panelled near window, enqueue_potrf: the tile receives the whole sub-panel so far in
// this one pass); every operand of the wave is requested before its first MFMA.
template <int NK>
__device__ __forceinline__ void diag_update_tile_nk(double* __restrict__ A, int ld, int kb, int mtile, double* __restrict__ part)
{
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int bi, bj;
    tri_index(mtile, bi, bj);
    const int c = lane & 15, g = lane >> 4;
    const int k0 = (kb + 1 - NK) * TILE + 32 * NK * w, i0 = (kb + 1) * TILE;
    const double* Li = A + (size_t)(i0 + bi * MT + c) * ld + k0 + g;
    const double* Lj = A + (size_t)(i0 + bj * MT + c) * ld + k0 + g;
    double* C = A + (size_t)(i0 + bi * MT + g) * ld + i0 + bj * MT + c;
    double la[8 * NK], lb[8 * NK];                      // all operands in flight before the first MFMA
#pragma unroll
    for (int s = 0; s < 8 * NK; s++) { la[s] = -Li[4 * s]; lb[s] = Lj[4 * s]; }
    d4 acc = (d4){0.0, 0.0, 0.0, 0.0}, acc2 = acc;
    if (w == 0) {
#pragma unroll
        for (int r = 0; r < 4; r++) acc[r] = C[(size_t)(4 * r) * ld];
    }
#pragma unroll
    for (int s = 0; s < 8 * NK; s += 2) {
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(la[s], lb[s], acc, 0, 0, 0);
        acc2 = __builtin_amdgcn_mfma_f64_16x16x4f64(la[s + 1], lb[s + 1], acc2, 0, 0, 0);
    }
    acc += acc2;
    if (w > 0) {
#pragma unroll
        for (int r = 0; r < 4; r++) part[((w - 1) * 4 + r) * 64 + lane] = acc[r];
    }
    __syncthreads();
    if (w == 0) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const double v = ((acc[r] + part[r * 64 + lane]) + part[(4 + r) * 64 + lane]) + part[(8 + r) * 64 + lane];
            __hip_atomic_store(C + (size_t)(4 * r) * ld, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

__device__ __forceinline__ void diag_update_tile(double* __restrict__ A, int ld, int kb, int ks, int mtile, double* __restrict__ part)
{
    switch (kb + 1 - ks) {                              // (uniform over the launch)
    case 1: diag_update_tile_nk<1>(A, ld, kb, mtile, part); break;
    case 2: diag_update_tile_nk<2>(A, ld, kb, mtile, part); break;
    case 3: diag_update_tile_nk<3>(A, ld, kb, mtile, part); break;
    default: diag_update_tile_nk<4>(A, ld, kb, mtile, part); break;
    }
}

// ------------------------------------------------------------------------------------------
// One launch per factorisation step kb: the trailing update A22 -= L21 L21^T AND, inside it, the
// factorisation of the NEXT diagonal block.  Workgroups 0..35 (dispatched first) update one micro tile of
// tile (kb+1,kb+1) each, straight from L2; the last of them to finish (a ticket at agent scope, no spinning)
// goes on to factor that block (potf2_body) while the other workgroups of the launch run the MFMA tile
// products of the rest of the trailing matrix.  The latency-bound diagonal block therefore never waits for
// a free CU slot and needs no second stream.
// (Round 3 also ran the panel solve inside this launch -- strips first, the diagonal workgroups and the tile
//  products waiting on per-row counters: every tile workgroup then needs an agent-scope acquire (per-XCD L2s
//  are not coherent) and the hand-offs cost what the kernel boundary did: 41.7 vs 43.5 us per chain-bound
//  step, Cholesky 5.86 vs 5.52 ms at N=8192.  Not kept.)
// ------------------------------------------------------------------------------------------
constexpr int NDIAGWG = NLT;                          // 36 workgroups, one micro tile of the next diagonal block each
constexpr int STEP_LDS = POTF2_LDS;                   // >= GEMM_LDS (66048); two such workgroups still fit one CU
static_assert(STEP_LDS == 79360, "dynamic LDS of the step launch");
static_assert(POTF2_LDS >= GEMM_LDS, "the fused step kernel sizes its LDS for both roles");

// wcol (two-speed form, enqueue_potrf): the launch updates only the tile columns [kb+1, kb+1+wcol) -- the near
// window -- and the far columns are brought up to date once per panel by k_syrk_wide with K = P*128.
// wcol >= the trailing size: the classic full update.
// ks (sub-panelled near window): the launch subtracts the k tiles [ks, kb] in one pass, K = (kb + 1 - ks) * 128 --
// the columns it touches have not seen any of them yet (plan_step, cugp_capi.cpp).  ks = kb: one k tile per step.
__global__ __launch_bounds__(256, 2) void k_syrk_step(double* __restrict__ A, int ld, int kb,
                                                      double* __restrict__ d16, double* __restrict__ d64,
                                                      double* __restrict__ logdet_part,
                                                      unsigned* __restrict__ tickets, int nfull, int wcol,
                                                      int ks, const ExpertPtrs* __restrict__ bt,
                                                      unsigned long long* stamp, int vec0, const double* __restrict__ zv,
                                                      double* __restrict__ wv)
{
    LaunchStamp stamp_(stamp);
    // batched: the EXPERT is the fast grid index, so the diagonal-block workgroups of all experts are
    // dispatched before any tile product (the serial chain of every expert starts at launch)
    const int bid = bt ? blockIdx.y : blockIdx.x;
    if (bt) {
        const ExpertPtrs& e = bt[blockIdx.x];
        A = GP(e.A); d16 = GP(e.d16); d64 = GP(e.d64); logdet_part = GP(e.logdet); tickets = GP(e.tickets);
        if (zv) { zv = GP(e.z); wv = GP(e.w); }
    }
    // workgroups from vec0 on (only launched when zv is given): the forward substitution's update of the running
    // right-hand side with the column this step consumes, one workgroup per tile row below it
    if (zv && bid >= vec0) {
        vec_update(A, ld, kb, kb + 1 + (bid - vec0), zv, wv);
        return;
    }
    extern __shared__ __attribute__((aligned(16))) double sm[];
    __shared__ double red[TILE + 4 * MT];
    __shared__ unsigned s_ticket;
    if (bid < NDIAGWG) {
        // the factorisation's serial chain: win instruction issue over the product waves sharing the SIMD
        // (this launch's own tiles and the inverse blocks running on the other streams)
        __builtin_amdgcn_s_setprio(3);
        WGT(wgt_, WGT_DIAGUPD, kb);
        diag_update_tile(A, ld, kb, ks, bid, sm);
        // publish: wave 0 drains its (agent-scope, write-through) tile stores, then ONE of its lanes draws the
        // ticket (relaxed: the tile is in memory before the ticket, and the last arriver reads the tiles with
        // agent-scope loads that bypass its L1 -- the hand-off form of the CDNA guide's Guideline 16, R1)
        // This form leans on gfx950 behaviour the HIP memory model does not promise: vmcnt counts stores as well as
        // loads (no separate store counter) and sc1 stores / loads are coherent across the XCDs' L2s.  EVERY read of
        // the handed-over block must be one of the agent-scope loads of potf2_body<true>.  The library is built for
        // gfx950 only (cugp_amd/build.py); another target must not compile this silently:
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "k_syrk_step's fence-free ticket hand-off is validated on gfx950 only: use an acq_rel ticket + agent acquire fence elsewhere"
#endif
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (threadIdx.x == 0)
            s_ticket = __hip_atomic_fetch_add(&tickets[kb], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        if (s_ticket != NDIAGWG - 1) return;           // not the last arriver
        // (the last arriver reads the 36 micro tiles with agent-scope loads: potf2_body<true>, no acquire fence)
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const int kn = kb + 1;
        WGT(wgt2_, WGT_POTF2, kb);
        potf2_body<true>(A + (size_t)kn * TILE * ld + kn * TILE, ld, d16 + (size_t)kn * NMT * (MT * MT),
                   d64 + (size_t)kn * 8192, logdet_part + kn, sm, red);
        return;
    }
    // tile 0 = (kb+1,kb+1) is the diagonal one above.  Odd steps walk the tiles backwards so the tiles
    // written last by step kb (still in the 256 MiB Infinity Cache) are the first read by step kb+1.
    // Regular tiles: `nfull` of them as 128x128 workgroups; the rest (a partial last round that would
    // leave most of the chip idle for a whole tile time) as four 64x64 workgroups each.
    __builtin_amdgcn_s_setprio(1);                      // ahead of the inverse-block products (priority 0)
    WGT(wgt_, WGT_STEPTILE, kb);
    const int x = bid - NDIAGWG;
    if (x < nfull) {
        // Workgroups are dealt round-robin over the 8 XCDs (private L2 each): give every XCD one contiguous
        // run of the tile list, so neighbouring tiles (same panel rows) share an L2 (bijective for any count).
        // Odd steps walk backwards: the tiles written last by step kb are the first read by step kb+1.
        int ti, tj;
        const int xg = x & 7, xq = nfull >> 3, xr = nfull & 7;
        const int tlin = (xg < xr ? xg * (xq + 1) : xr * (xq + 1) + (xg - xr) * xq) + (x >> 3) + 1;
        trap_index((kb & 1) ? nfull + 1 - tlin : tlin, wcol, ti, tj);   // tile 0 = (kb+1,kb+1) is the diagonal one
        const int i0 = (kb + 1 + ti) * TILE, j0 = (kb + 1 + tj) * TILE;
        d4 acc[4][4];
        acc_zero(acc);
        tile_nt<false>(A + (size_t)i0 * ld, ld, A + (size_t)j0 * ld, ld, ks * TILE, (kb + 1) * TILE, acc, (char*)sm);
        tile_accum_store<-1>(A + (size_t)i0 * ld + j0, ld, acc);
    } else {
        int ti, tj;
        const int y = x - nfull;
        trap_index(nfull + 1 + (y >> 2), wcol, ti, tj);
        const int i0 = (kb + 1 + ti) * TILE + ((y >> 1) & 1) * 64, j0 = (kb + 1 + tj) * TILE + (y & 1) * 64;
        d4 acc[2][2];
        acc_zero(acc);
        tile_nt<false>(A + (size_t)i0 * ld, ld, A + (size_t)j0 * ld, ld, ks * TILE, (kb + 1) * TILE, acc, (char*)sm);
        tile_accum_store<-1>(A + (size_t)i0 * ld + j0, ld, acc);
    }
}

static inline int trap_count(int m, int wcol)          // tiles (ti >= tj) of the first wcol columns of an m-triangle
{
    return wcol >= m ? tri_count(m) : tri_count(wcol) + (m - wcol) * wcol;
}

void launch_syrk_step(double* A, int ld, int kb, int nt, double* d16, double* d64, double* logdet_part,
                      unsigned* tickets, hipStream_t s, Batch bt, int wcol, int ks, const double* zv, double* wv)
{
    const int m = nt - kb - 1;
    if (m <= 0) return;
    set_big_lds();
    if (wcol <= 0 || wcol > m) wcol = m;
    // tiles beyond the last full round of 512 workgroup slots run as 64x64 quarters when that round
    // would be less than three quarters full
    const int ntl = trap_count(m, wcol) - 1;
    int nfull = ntl;
    if (ntl >= 512 && (ntl % 512) <= tune(TUNE_SYRK_REM_MAX)) nfull = ntl - ntl % 512;
    // Few tiles (the chain-bound tail of the factorisation): a 128x128 workgroup alone on its CU issues one MFMA
    // per ~138 cycles (one wave per SIMD: half the pipe's rate) and takes ~40 us -- as long as the diagonal block
    // inside this launch.  As 64x64 quarters the same tiles take ~12 us per round of 512 workgroups.
    if ((long long)ntl * bt.count * 4 <= tune(TUNE_STEP_QUARTER_MAX)) nfull = 0;
    const int vec0 = NDIAGWG + nfull + 4 * (ntl - nfull);
    const unsigned nwg = vec0 + (zv ? m : 0);
    if (ks < 0 || ks > kb) ks = kb;
    if (kb + 1 - ks > SUBPANEL_MAX) return;               // (plan_step never asks for more)
    CUGP_LAUNCH(k_syrk_step, bt.tab ? dim3(bt.count, nwg) : dim3(nwg), dim3(256), STEP_LDS, s, A, ld, kb, d16,
                       d64, logdet_part, tickets, nfull, wcol, ks, bt.tab, take_stamp(), vec0, zv, wv);
}

// ------------------------------------------------------------------------------------------
// Wide trailing update (look-ahead Cholesky): A(ti,tj) -= sum_{k in [k0, k0+kw)} L(ti,k) L(tj,k)^T for the tile
// columns tj in [ca, cb), ti >= tj -- ONE pass over the C tiles with K = kw*128 (the tile product costs a fixed
// ~12 us per C tile + 30.5 us per 128 of K: 50 TF/s at K=128, 66 at K=512 when the tiles fill whole rounds of
// the 512 workgroup slots).  One workgroup per tile; a small last round runs as 64x64 quarters.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256, 2) void k_syrk_wide(double* __restrict__ A, int ld, int k0, int kw, int ca,
                                                      int cb, int ntiles, int nfull, int rev,
                                                      const ExpertPtrs* __restrict__ bt, unsigned long long* stamp)
{
    LaunchStamp stamp_(stamp);
    if (bt) A = GP(bt[blockIdx.y].A);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __builtin_amdgcn_s_setprio(1);
    WGT(wgt_, WGT_WIDE, k0);
    if ((int)blockIdx.x >= nfull) {
        // the last, partly empty round of the launch as 64x64 quarters (split_round)
        const int y = blockIdx.x - nfull;
        int ti, tj;
        trap_index(nfull + (y >> 2), cb - ca, ti, tj);
        const int i0 = (ca + ti) * TILE + ((y >> 1) & 1) * 64, j0 = (ca + tj) * TILE + (y & 1) * 64;
        d4 acc[2][2];
        acc_zero(acc);
        tile_nt<false>(A + (size_t)i0 * ld, ld, A + (size_t)j0 * ld, ld, k0 * TILE, (k0 + kw) * TILE, acc, smem);
        tile_accum_store<-1>(A + (size_t)i0 * ld + j0, ld, acc);
        return;
    }
    // every XCD (workgroups are dealt round-robin over the 8 of them) walks one contiguous run of the row-major
    // tile list: neighbours share panel rows in its L2
    const int xg = blockIdx.x & 7;
    const int xq = nfull >> 3, xr = nfull & 7;
    const int tlin = (xg < xr ? xg * (xq + 1) : xr * (xq + 1) + (xg - xr) * xq) + (blockIdx.x >> 3);
    int ti, tj;
    trap_index(rev ? nfull - 1 - tlin : tlin, cb - ca, ti, tj);
    const int i0 = (ca + ti) * TILE, j0 = (ca + tj) * TILE;
    d4 acc[4][4];
    acc_zero(acc);
    tile_nt<false>(A + (size_t)i0 * ld, ld, A + (size_t)j0 * ld, ld, k0 * TILE, (k0 + kw) * TILE, acc, smem);
    tile_accum_store<-1>(A + (size_t)i0 * ld + j0, ld, acc);
}

// k_syrk_wide's whole tiles [0, nfull = gridDim.x) on eight waves (tile_nt8), the same walk over the tile list
__global__ __launch_bounds__(512, 4) void k_syrk_wide8(double* __restrict__ A, int ld, int k0, int kw, int ca, int cb,
                                                       int rev, const ExpertPtrs* __restrict__ bt,
                                                       unsigned long long* stamp)
{
    LaunchStamp stamp_(stamp);
    if (bt) A = GP(bt[blockIdx.y].A);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __builtin_amdgcn_s_setprio(1);
    const int nfull = gridDim.x;
    const int xg = blockIdx.x & 7;
    const int xq = nfull >> 3, xr = nfull & 7;
    const int tlin = (xg < xr ? xg * (xq + 1) : xr * (xq + 1) + (xg - xr) * xq) + (blockIdx.x >> 3);
    int ti, tj;
    trap_index(rev ? nfull - 1 - tlin : tlin, cb - ca, ti, tj);
    const int i0 = (ca + ti) * TILE, j0 = (ca + tj) * TILE;
    d4 acc[2][4];
    acc_zero8(acc);
    tile_nt8<false>(A + (size_t)i0 * ld, ld, A + (size_t)j0 * ld, ld, k0 * TILE, (k0 + kw) * TILE, acc, smem);
    tile_out8<-1>(A + (size_t)i0 * ld + j0, ld, acc);
}

// ... and the tiles from x0 on as 64x64 quarters on four waves (the quarter branch of k_syrk_wide)
__global__ __launch_bounds__(256, 2) void k_syrk_wide_rest(double* __restrict__ A, int ld, int k0, int kw, int ca, int cb,
                                                           int x0, const ExpertPtrs* __restrict__ bt)
{
    if (bt) A = GP(bt[blockIdx.y].A);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __builtin_amdgcn_s_setprio(1);
    const int y = blockIdx.x;
    int ti, tj;
    trap_index(x0 + (y >> 2), cb - ca, ti, tj);
    const int i0 = (ca + ti) * TILE + ((y >> 1) & 1) * 64, j0 = (ca + tj) * TILE + (y & 1) * 64;
    d4 acc[2][2];
    acc_zero(acc);
    tile_nt<false>(A + (size_t)i0 * ld, ld, A + (size_t)j0 * ld, ld, k0 * TILE, (k0 + kw) * TILE, acc, smem);
    tile_accum_store<-1>(A + (size_t)i0 * ld + j0, ld, acc);
}

// A launch of `tiles` uniform-ish 128x128 tiles fills the 512 workgroup slots round by round; a last round that is
// mostly empty still costs a whole tile time (134 us at K = 512).  When the remainder is small its tiles run as
// four 64x64 workgroups each instead: -> number of tiles launched whole (the rest are split).
static int split_round(int tiles, int count)
{
    const int slots = 512 / (count > 0 ? count : 1) > 0 ? 512 / (count > 0 ? count : 1) : 1;
    const int rem = tiles % slots;
    if (tiles < slots || rem == 0 || rem > tune(TUNE_SPLIT_REM_MAX)) return tiles;
    return tiles - rem;
}

// tile columns [ca, cb) (rows >= column) -= L(., k0..k0+kw) L(., k0..k0+kw)^T; returns the number of tiles
int launch_syrk_wide(double* A, int ld, int nt, int k0, int kw, int ca, int cb, int rev, hipStream_t s, Batch bt)
{
    if (cb > nt) cb = nt;
    if (ca >= cb || kw <= 0) return 0;
    set_big_lds();
    const int ntiles = trap_count(nt - ca, cb - ca);
    const int nfull = split_round(ntiles, bt.count);
    if (tune(TUNE_WAVES8) != 0 && nfull > 0) {
        CUGP_LAUNCH(k_syrk_wide8, dim3(nfull, bt.count), dim3(512), GEMM_LDS, s, A, ld, k0, kw, ca, cb, rev, bt.tab,
                    take_stamp());
        if (ntiles > nfull)
            hipLaunchKernelGGL(k_syrk_wide_rest, dim3(4 * (ntiles - nfull), bt.count), dim3(256), Geo<2>::LDS, s, A, ld, k0,
                               kw, ca, cb, nfull, bt.tab);
        return ntiles;
    }
    CUGP_LAUNCH(k_syrk_wide, dim3(nfull + 4 * (ntiles - nfull), bt.count), dim3(256), GEMM_LDS, s, A, ld, k0, kw, ca,
                       cb, ntiles, nfull, rev, bt.tab, take_stamp());
    return ntiles;
}
