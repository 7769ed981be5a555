// inverse_gfx950.h -- L^-1 by recursive doubling and bordering (k_trtri_level, k_trtri_border and its 8-wave / rest
// siblings), the 128x128 diagonal-tile inverse (k_trtri_diag), a whole hand-over block in one launch (k_trtri_block), and
// K^-1 = L^-T L^-1 (k_lauum, k_lauum8, k_lauum_rest); each launcher directly behind its kernels.
//
// Include-point contract.  Needs the device; also holds launchers.  Included by kernels.hip alone, INSIDE namespace cugp,
// after these are declared -- the file includes nothing and declares none of them:
//   kernels.h        TILE, ExpertPtrs, Batch, TRTRI_BLOCK_MAXWG, tune and the TUNE_* keys, the launcher prototypes
//   kernels.hip      d2, d4, GP, WGT and the WGT_* kinds, LaunchStamp, CUGP_LAUNCH, take_stamp, tri_count, set_big_lds
//   cov_device.h     tri_index
//   tile_gfx950.h    Geo, GEMM_LDS, tile_nt, tile_nt8, tile_store_t and their epilogues
//   chol_gfx950.h    MT, TRTRI_LDS, mt_off, micro_mma_nn, micro_mma_acc_b, micro_store, split_round
#pragma once

// ---- triangular inverse.  [A 0; C B]^-1 = [TA 0; -TB C TA, TB] with A = tiles [.., b0), B = tiles [b0, ..):
// step 1: Wt(tj in A, ti in B) = sum_{k in A, k >= tj} U[tj][k] * L[ti][k]   -> scratch in T's upper tiles
//         (k tiles [kbeg, kend) of it; `accumulate` adds onto what earlier launches left there)
// step 2: T(ti in B, tj in A) = -sum_{k in B, k <= ti} T[ti][k] * Wt[tj][k]   and U(tj,ti) = transpose
template <int WM>
__device__ __forceinline__ void trtri_tile(const double* __restrict__ L, double* __restrict__ T,
                                           double* __restrict__ U, int ld, int tj, int ti, int step, int kbeg,
                                           int kend, bool accumulate, int sub, char* smem)
{
    constexpr int SUB = 4 / WM;                          // output sub-tiles per 128-tile edge (1 or 2)
    constexpr int BT = 32 * WM;
    const int si = (sub / SUB) * BT, sj = (sub % SUB) * BT;     // offsets of my sub-tile inside the 128-tile
    d4 acc[WM][WM];
    if (step == 1) {
        // Wt(tj, ti) rows in A's tile tj, columns in B's tile ti
        double* W = T + (size_t)(tj * TILE + si) * ld + ti * TILE + sj;
        acc_zero(acc);
        tile_nt<false>(U + (size_t)(tj * TILE + si) * ld, ld, L + (size_t)(ti * TILE + sj) * ld, ld, kbeg * TILE,
                       kend * TILE, acc, smem);
        if (accumulate) tile_accum_store<1>(W, ld, acc);
        else tile_store(W, ld, acc, 1.0);
    } else {
        acc_zero(acc);
        tile_nt<true>(T + (size_t)(ti * TILE + si) * ld, ld, T + (size_t)(tj * TILE + sj) * ld, ld, kbeg * TILE,
                      kend * TILE, acc, smem);
        tile_store(T + (size_t)(ti * TILE + si) * ld + tj * TILE + sj, ld, acc, 1.0);
        tile_store_t(U + (size_t)(tj * TILE + sj) * ld + ti * TILE + si, ld, acc, 1.0, smem);
    }
}

// one tile (blk) / sub-tile (sub) of one level of recursive doubling over nt tiles: all pairs of s-tile blocks
template <int WM>
__device__ __forceinline__ void level_item(const double* __restrict__ L, double* __restrict__ T, double* __restrict__ U,
                                           int ld, int nt, int s, int step, int blk, int sub, char* smem)
{
    const int npairs = (nt + 2 * s - 1) / (2 * s);      // last one may have a short (or empty) B
    int p = blk / (s * s);
    if (p > npairs - 1) p = npairs - 1;
    int rem = blk - p * s * s;
    const int a0 = 2 * p * s;                            // A = [a0, a0+s), B = [a0+s, min(a0+2s, nt))
    const int b0 = a0 + s;
    int sb = nt - b0;
    if (sb > s) sb = s;
    // tile in A (column block), tile in B (row block); longest k range first in both steps
    // (step 1: k from tj to the end of A -> ja ascending; step 2: k from b0 to ti -> ib descending)
    const int ja = (step == 1) ? rem / sb : rem % s;
    const int ib = (step == 1) ? rem % sb : sb - 1 - rem / s;
    const int tj = a0 + ja, ti = b0 + ib;
    trtri_tile<WM>(L, T, U, ld, tj, ti, step, step == 1 ? tj : b0, step == 1 ? b0 : ti + 1, false, sub, smem);
}

// tiles |A| x |B| of one level over nt tiles (pairs p = 0.. : A = [2ps, 2ps+s), B = [2ps+s, min(2ps+2s, nt)))
__host__ __device__ inline int level_tiles(int nt, int s)
{
    int tiles = 0;
    for (int a0 = 0; a0 + s < nt; a0 += 2 * s) {
        int sb = nt - (a0 + s);
        if (sb > s) sb = s;
        tiles += s * sb;
    }
    return tiles;
}

// one level of recursive doubling: all pairs of s-tile blocks at once
template <int WM>
__global__ __launch_bounds__(256, 2) void k_trtri_level(const double* __restrict__ L, double* __restrict__ T,
                                                        double* __restrict__ U, int ld, int nt, int s, int step,
                                                        size_t off, const ExpertPtrs* __restrict__ bt,
                                                        unsigned long long* stamp)
{
    LaunchStamp stamp_(stamp);
    // off: element offset of the diagonal sub-matrix the level works on (a block of inverse rows)
    if (bt) { L = GP(bt[blockIdx.y].A); T = GP(bt[blockIdx.y].T); U = GP(bt[blockIdx.y].U); }
    L += off; T += off; U += off;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    WGT(wgt_, WGT_LEVEL, s * 2 + step);
    constexpr int SUB = 4 / WM;
    level_item<WM>(L, T, U, ld, nt, s, step, blockIdx.x / (SUB * SUB), blockIdx.x % (SUB * SUB), smem);
}

int launch_trtri_level(const double* L, double* T, double* U, int ld, int nt, int s, int step, hipStream_t st,
                       Batch bt, size_t off)
{
    // pairs p = 0.. : A = [2ps, 2ps+s), B = [2ps+s, min(2ps+2s, nt)); count tiles |A| x |B|
    int tiles = 0;
    for (int a0 = 0; a0 + s < nt; a0 += 2 * s) {
        int sb = nt - (a0 + s);
        if (sb > s) sb = s;
        tiles += s * sb;
    }
    if (tiles <= 0) return 0;
    // few 128-tiles cannot fill 512 workgroup slots: use 64x64 output tiles (4x the parallelism) there
    set_big_lds();
    if (tiles * bt.count <= tune(TUNE_TRTRI_WM2_MAX)) {  // (a batched launch fills the chip with fewer tiles each)
        CUGP_LAUNCH(k_trtri_level<2>, dim3(tiles * 4, bt.count), dim3(256), Geo<2>::LDS, st, L, T, U, ld, nt, s,
                           step, off, bt.tab, take_stamp());
        return 2;
    }
    CUGP_LAUNCH(k_trtri_level<4>, dim3(tiles, bt.count), dim3(256), GEMM_LDS, st, L, T, U, ld, nt, s, step,
                       off, bt.tab, take_stamp());
    return 4;
}

// bordering: rows B = [a, a+w) of the inverse from the finished leading block A = [0, a) and B's own
// inverse (the same two steps with an unbalanced split; lets the inverse follow the factorisation
// block row by block row).  Step 1 comes in launches over k chunks [c0, c1) of A, ascending, each adding
// onto the last; the host issues chunk [c0, c1) for ALL rows below it as soon as those inverse rows are
// final (uniform K, and most of the work is done before the rows' own turn comes).
template <int WM>
__device__ __forceinline__ void border_tile(const double* __restrict__ L, double* __restrict__ T, double* __restrict__ U,
                                            int ld, int a, int w, int step, int c0, int c1, int blk, int sub, char* smem)
{
    if (step == 1) {
        const int tj = blk / w, ti = a + blk % w;                       // tj < c1
        trtri_tile<WM>(L, T, U, ld, tj, ti, 1, tj > c0 ? tj : c0, c1, tj < c0, sub, smem);
    } else {
        const int tj = blk % a, ti = a + w - 1 - blk / a;               // longest k range first
        trtri_tile<WM>(L, T, U, ld, tj, ti, 2, a, ti + 1, false, sub, smem);
    }
}

// nfull (WM = 4 only): tiles beyond it run as four 64x64 workgroups each (the last, partly empty round; split_round)
template <int WM>
__global__ __launch_bounds__(256, 2) void k_trtri_border(const double* __restrict__ L, double* __restrict__ T,
                                                         double* __restrict__ U, int ld, int a, int w, int step,
                                                         int c0, int c1, int nfull, const ExpertPtrs* __restrict__ bt,
                                                         unsigned long long* stamp)
{
    LaunchStamp stamp_(stamp);
    if (bt) { L = GP(bt[blockIdx.y].A); T = GP(bt[blockIdx.y].T); U = GP(bt[blockIdx.y].U); }
    extern __shared__ __attribute__((aligned(16))) char smem[];
    WGT(wgt_, WGT_BORDER, a * 4 + step);
    if (WM == 2) {
        border_tile<2>(L, T, U, ld, a, w, step, c0, c1, blockIdx.x >> 2, blockIdx.x & 3, smem);
    } else if ((int)blockIdx.x < nfull) {
        border_tile<4>(L, T, U, ld, a, w, step, c0, c1, blockIdx.x, 0, smem);
    } else {
        const int y = blockIdx.x - nfull;
        border_tile<2>(L, T, U, ld, a, w, step, c0, c1, nfull + (y >> 2), y & 3, smem);
    }
}

// step 1 of the bordering (border_tile, step 1): whole tiles [0, gridDim.x) on eight waves
__global__ __launch_bounds__(512, 4) void k_trtri_border8(const double* __restrict__ L, double* __restrict__ T,
                                                          const double* __restrict__ U, int ld, int a, int w, int c0,
                                                          int c1, const ExpertPtrs* __restrict__ bt,
                                                          unsigned long long* stamp)
{
    LaunchStamp stamp_(stamp);
    if (bt) { L = GP(bt[blockIdx.y].A); T = GP(bt[blockIdx.y].T); U = GP(bt[blockIdx.y].U); }
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tj = blockIdx.x / w, ti = a + blockIdx.x % w;             // tj < c1
    double* W = T + (size_t)(tj * TILE) * ld + ti * TILE;
    d4 acc[2][4];
    acc_zero8(acc);
    tile_nt8<false>(U + (size_t)(tj * TILE) * ld, ld, L + (size_t)(ti * TILE) * ld, ld, (tj > c0 ? tj : c0) * TILE,
                    c1 * TILE, acc, smem);
    if (tj < c0) tile_out8<1>(W, ld, acc);
    else tile_out8<0>(W, ld, acc);
}

__global__ __launch_bounds__(256, 2) void k_trtri_border_rest(const double* __restrict__ L, double* __restrict__ T,
                                                              double* __restrict__ U, int ld, int a, int w, int c0,
                                                              int c1, int x0, const ExpertPtrs* __restrict__ bt)
{
    if (bt) { L = GP(bt[blockIdx.y].A); T = GP(bt[blockIdx.y].T); U = GP(bt[blockIdx.y].U); }
    extern __shared__ __attribute__((aligned(16))) char smem[];
    border_tile<2>(L, T, U, ld, a, w, 1, c0, c1, x0 + (blockIdx.x >> 2), blockIdx.x & 3, smem);
}

// step 1 of the bordering, spread over time: add the k tiles [c0, c1) (a block of inverse rows that just
// became final) to Wt(tj < c1, ti in [ra, ra+rw)) for ALL rows below the block
int launch_trtri_border1(const double* L, double* T, double* U, int ld, int ra, int rw, int c0, int c1,
                         hipStream_t st, Batch bt)
{
    const int tiles = c1 * rw;
    if (tiles <= 0) return 0;
    set_big_lds();
    if (tiles * bt.count <= tune(TUNE_BORDER_WM2_MAX)) {
        CUGP_LAUNCH(k_trtri_border<2>, dim3(tiles * 4, bt.count), dim3(256), Geo<2>::LDS, st, L, T, U, ld, ra, rw,
                           1, c0, c1, 0, bt.tab, take_stamp());
        return 2;
    }
    const int nfull = split_round(tiles, bt.count);
    if (tune(TUNE_WAVES8) != 0 && nfull > 0) {
        CUGP_LAUNCH(k_trtri_border8, dim3(nfull, bt.count), dim3(512), GEMM_LDS, st, L, T, U, ld, ra, rw, c0, c1, bt.tab,
                    take_stamp());
        if (tiles > nfull)
            hipLaunchKernelGGL(k_trtri_border_rest, dim3(4 * (tiles - nfull), bt.count), dim3(256), Geo<2>::LDS, st, L, T,
                               U, ld, ra, rw, c0, c1, nfull, bt.tab);
        return 4;
    }
    CUGP_LAUNCH(k_trtri_border<4>, dim3(nfull + 4 * (tiles - nfull), bt.count), dim3(256), GEMM_LDS, st, L, T,
                       U, ld, ra, rw, 1, c0, c1, nfull, bt.tab, take_stamp());
    return 4;
}

// step 2: rows [a, a+w) of the inverse from their finished Wt and the block's own inverse
int launch_trtri_border2(const double* L, double* T, double* U, int ld, int a, int w, hipStream_t st, Batch bt)
{
    const int tiles = a * w;
    if (tiles <= 0) return 0;
    set_big_lds();
    if (tiles * bt.count <= tune(TUNE_TRTRI_WM2_MAX)) {
        CUGP_LAUNCH(k_trtri_border<2>, dim3(tiles * 4, bt.count), dim3(256), Geo<2>::LDS, st, L, T, U, ld, a, w, 2,
                           0, 0, 0, bt.tab, take_stamp());
        return 2;
    }
    const int nfull = split_round(tiles, bt.count);
    CUGP_LAUNCH(k_trtri_border<4>, dim3(nfull + 4 * (tiles - nfull), bt.count), dim3(256), GEMM_LDS, st, L, T,
                       U, ld, a, w, 2, 0, 0, nfull, bt.tab, take_stamp());
    return 4;
}

// inverse of a 128x128 diagonal factor block from the two 64x64 inverses potf2 left in d64 (one doubling
// step, T10 = -T11 (L10 T00), on 16x16 micro tiles: wave = micro-tile column of T10); writes T (lower, zeros
// above) and U = T^T (upper, zeros below).  blockIdx.x = block offset from kb.  ~6 us (the blocked
// substitution from the 16x16 inverses it replaces took 92 us -- 10 % of a 1500-row evaluation).
__device__ __forceinline__ void trtri_diag_body(const double* __restrict__ A, int ld, int b,
                                                const double* __restrict__ d64, double* __restrict__ T,
                                                double* __restrict__ U, double* __restrict__ sm)
{
    const int t = threadIdx.x, wave = t >> 6;
    const double* Ab = A + (size_t)b * TILE * ld + b * TILE;
    const double* T00 = d64 + (size_t)b * 8192;
    const double* T11 = T00 + 4096;
    {
        // all 36 loads in flight before the first LDS store (fully unrolled: which of the three sources a micro
        // tile comes from is then a compile-time choice; as a rolled loop with the branches inside it the loads
        // went out one at a time and the kernel took 25 us, nearly all of it this prologue)
        const int r = t >> 4, c = t & 15;
        double v[NLT];
#pragma unroll
        for (int bi = 0; bi < NMT; bi++)
#pragma unroll
            for (int bj = 0; bj <= bi; bj++) {
                const int q = bi * (bi + 1) / 2 + bj;
                if (bi < 4) v[q] = T00[(bi * MT + r) * 64 + bj * MT + c];
                else if (bj >= 4) v[q] = T11[((bi - 4) * MT + r) * 64 + (bj - 4) * MT + c];
                else v[q] = Ab[(size_t)(bi * MT + r) * ld + bj * MT + c];            // L10
            }
#pragma unroll
        for (int q = 0; q < NLT; q++) sm[q * MTS + r * (MT + 1) + c] = v[q];
    }
    __syncthreads();
    {
        const int bj = wave;                                 // my micro-tile column of T10
        const d4 zero4 = (d4){0.0, 0.0, 0.0, 0.0};
        d4 w[4];                                             // W(4 + q, bj) = sum_{jp >= bj} L10(4 + q, jp) T00(jp, bj)
#pragma unroll
        for (int q = 0; q < 4; q++) {
            w[q] = zero4;
            for (int jp = bj; jp < 4; jp++) w[q] = micro_mma_nn(sm + mt_off(4 + q, jp), sm + mt_off(jp, bj), w[q]);
        }
        __syncthreads();                                     // every wave has read its L10 tiles
#pragma unroll
        for (int q = 0; q < 4; q++) {                        // T10(4 + q, bj) = -sum_{k <= q} T11(4 + q, 4 + k) W(4 + k, bj)
            d4 x = zero4;
#pragma unroll
            for (int k = 0; k <= q; k++) x = micro_mma_acc_b(sm + mt_off(4 + q, 4 + k), w[k], x);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            micro_store(sm + mt_off(4 + q, bj), x);
        }
    }
    __syncthreads();
    double* Tb = T + (size_t)b * TILE * ld + b * TILE;
    double* Ub = U + (size_t)b * TILE * ld + b * TILE;
#pragma unroll 8
    for (int e = t; e < TILE * TILE; e += 256) {
        const int r = e >> 7, c = e & 127, br = r >> 4, bc = c >> 4;
        // T(r,c) lives in micro tile (br,bc) when bc <= br (diagonal micro tiles are zero above their diagonal)
        Tb[(size_t)r * ld + c] = bc <= br ? sm[mt_off(br, bc) + (r & 15) * (MT + 1) + (c & 15)] : 0.0;
        Ub[(size_t)r * ld + c] = br <= bc ? sm[mt_off(bc, br) + (c & 15) * (MT + 1) + (r & 15)] : 0.0;   // T(c,r)
    }
}

__global__ __launch_bounds__(256) void k_trtri_diag(const double* __restrict__ A, int ld, int kb,
                                                    const double* __restrict__ d64, double* __restrict__ T,
                                                    double* __restrict__ U, const ExpertPtrs* __restrict__ bt)
{
    if (bt) { A = GP(bt[blockIdx.y].A); d64 = GP(bt[blockIdx.y].d64); T = GP(bt[blockIdx.y].T); U = GP(bt[blockIdx.y].U); }
    extern __shared__ __attribute__((aligned(16))) double sm[];       // 36 lower micro tiles, as potf2_body
    WGT(wgt_, WGT_TRTRI_DIAG, kb);
    trtri_diag_body(A, ld, kb + blockIdx.x, d64, T, U, sm);
}

void launch_trtri_diag(const double* A, int ld, int kb, int nblocks, const double* d64, double* T, double* U,
                       hipStream_t s, Batch bt)
{
    set_big_lds();
    hipLaunchKernelGGL(k_trtri_diag, dim3(nblocks, bt.count), dim3(256), TRTRI_LDS, s, A, ld, kb, d64, T, U, bt.tab);
}

// ------------------------------------------------------------------------------------------
// The whole inverse of ONE hand-over block of rows [a, a + wb) -- the 128x128 inverses of its diagonal tiles and every
// level of the recursive doubling inside the block -- in ONE launch: what k_trtri_diag + 2 log2(wb) launches of
// k_trtri_level<2> did (at N = 8192, wb = 4: five launches of 2-16 workgroups, 15-45 us apiece while the big products of
// the other streams hold the chip; 80 of the evaluation's 260 launches).  A small persistent grid (<= 64 workgroups)
// walks the stages; between two stages every workgroup arrives at a monotonic agent-scope counter and waits for the
// others (release fence -> add ... poll -> acquire fence: the safe forms of the CDNA guide's barrier-counter row).
// The same tile code (trtri_diag_body, level_item<2>) in the same per-element order: bit-identical to the launches it
// replaces.  The grid is far below one workgroup per CU, the workgroups of a launch are dispatched in order, and what
// holds the other slots always ends without waiting for this launch -- so the waiting is deadlock-free; it is BOUNDED
// all the same (~seconds), and a wait that ran out poisons the block's log-determinant share (the evaluation comes
// back NaN instead of hanging the device).
// ------------------------------------------------------------------------------------------
constexpr int TRTRI_BLOCK_LDS = TRTRI_LDS > Geo<2>::LDS ? TRTRI_LDS : Geo<2>::LDS;
static_assert(TRTRI_BLOCK_LDS == 78336, "dynamic LDS of the one-launch block inverse: the larger of its two roles");

__device__ __forceinline__ bool stage_barrier(unsigned* __restrict__ ctr, unsigned target, unsigned spin_cap)
{
    __shared__ int s_ok;
    // every wave drains its own stores of the stage (the barrier's own wait is lgkmcnt only), THEN the workgroup
    // meets, then one lane writes this XCD's L2 back (all of the workgroup's stores are in it by now) and arrives
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // (the compiler may drop the wait behind the write-back)
        __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        int ok = 0;
        for (unsigned spin = 0; spin < spin_cap; spin++) {
            if (__hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= target) { ok = 1; break; }
            __builtin_amdgcn_s_sleep(8);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        s_ok = ok;
    }
    __syncthreads();
    return s_ok != 0;
}

__global__ __launch_bounds__(256, 2) void k_trtri_block(const double* __restrict__ L, const double* __restrict__ d64,
                                                        double* __restrict__ T, double* __restrict__ U, int ld, int a,
                                                        int wb, unsigned* __restrict__ ctr, double* __restrict__ poison,
                                                        int ctr_off, unsigned spin_cap, double* __restrict__ hstat,
                                                        const ExpertPtrs* __restrict__ bt, unsigned long long* stamp)
{
    LaunchStamp stamp_(stamp);
    if (bt) {
        const ExpertPtrs& e = bt[blockIdx.y];
        L = GP(e.A); d64 = GP(e.d64); T = GP(e.T); U = GP(e.U); ctr = GP(e.tickets) + ctr_off; poison = GP(e.logdet);
        if (hstat) hstat += (size_t)blockIdx.y * 8;
    }
    extern __shared__ __attribute__((aligned(16))) char smem[];
    WGT(wgt_, WGT_TRTRI_DIAG, a);
    const int G = gridDim.x, wg = blockIdx.x;
    for (int b = wg; b < wb; b += G) {
        if (b != wg) __syncthreads();                    // (the body's LDS image is reused)
        trtri_diag_body(L, ld, a + b, d64, T, U, (double*)smem);
    }
    const size_t off = (size_t)a * TILE * ld + (size_t)a * TILE;
    const double* Lb = L + off;
    double* Tb = T + off;
    double* Ub = U + off;
    unsigned stage = 0;
    bool ok = true;
    for (int s = 1; s < wb; s *= 2)
        for (int step = 1; step <= 2; step++) {
            ok = stage_barrier(ctr, (unsigned)G * ++stage, spin_cap) && ok;
            const int items = level_tiles(wb, s) * 4;
            for (int it = wg; it < items; it += G) {
                if (it != wg) __syncthreads();           // (the transposed store of the item before still reads its LDS image)
                level_item<2>(Lb, Tb, Ub, ld, wb, s, step, it >> 2, it & 3, smem);
            }
        }
    // a wait that ran out: this block's numbers are not to be trusted -- NaN into its log-determinant share (the
    // evaluation's values come back NaN) and the handle's pinned status word (its fetch returns CUGP_ERR_DEVICE)
    if (!ok && threadIdx.x == 0) {
        poison[a] = __builtin_nan("");
        if (hstat) hstat[6] = 1.0;
    }
}

int launch_trtri_block(const double* L, const double* d64, double* T, double* U, int ld, int a, int wb, unsigned* ctr,
                       double* poison, int ctr_off, hipStream_t s, Batch bt, int gcap, double* hstat)
{
    if (wb <= 0) return 0;
    set_big_lds();
    int G = wb;                                           // workgroups: the widest stage, one item each (<= 64)
    for (int sl = 1; sl < wb; sl *= 2) {
        const int items = level_tiles(wb, sl) * 4;
        if (items > G) G = items;
    }
    if (G > TRTRI_BLOCK_MAXWG) G = TRTRI_BLOCK_MAXWG;
    if (gcap >= 1 && G > gcap) G = gcap;                  // (every workgroup count gives the same bits: a stage's items are independent)
    CUGP_LAUNCH(k_trtri_block, dim3(G, bt.count), dim3(256), TRTRI_BLOCK_LDS, s, L, d64, T, U, ld, a, wb, ctr,
                       poison, ctr_off, (unsigned)tune(TUNE_BARRIER_SPIN), hstat, bt.tab, take_stamp());
    return G;
}

// ---- K^-1 (lower tiles, diagonal tiles complete) = U * U^T, U = L^-T upper, taken one block of
// inverse rows [a, a+w) at a time:  Kinv(ti,tj) (+)= sum_{k in [max(ti,a), a+w)} U[ti][k] U[tj][k]^T
// for tj <= ti < a+w.  a = 0, w = nt is the whole product in one launch.
template <int WM>
__device__ __forceinline__ void lauum_tile(const double* __restrict__ U, double* __restrict__ Kinv, int ld, int a, int w,
                                           int tile, int sub, char* smem)
{
    constexpr int SUB = 4 / WM, BT = 32 * WM;
    int ti, tj;
    tri_index(tile, ti, tj);                           // ascending ti = longest k ranges first
    const int si = (sub / SUB) * BT, sj = (sub % SUB) * BT;
    double* C = Kinv + (size_t)(ti * TILE + si) * ld + tj * TILE + sj;
    d4 acc[WM][WM];
    acc_zero(acc);
    tile_nt<false>(U + (size_t)(ti * TILE + si) * ld, ld, U + (size_t)(tj * TILE + sj) * ld, ld,
                   (ti < a ? a : ti) * TILE, (a + w) * TILE, acc, smem);
    if (ti < a) tile_accum_store<1>(C, ld, acc);       // rows of earlier blocks: add this block's share
    else tile_store(C, ld, acc, 1.0);
}

// nfull (WM = 4 only): the first nfull tiles as 128x128 workgroups, the rest -- a last, partly empty round of 512
// workgroup slots that would take a whole tile time -- as four 64x64 workgroups each (split_round below)
template <int WM>
__global__ __launch_bounds__(256, 2) void k_lauum(const double* __restrict__ U, double* __restrict__ Kinv, int ld,
                                                  int a, int w, int nfull, const ExpertPtrs* __restrict__ bt,
                                                  unsigned long long* stamp)
{
    LaunchStamp stamp_(stamp);
    if (bt) { U = GP(bt[blockIdx.y].U); Kinv = GP(bt[blockIdx.y].Kinv); }
    extern __shared__ __attribute__((aligned(16))) char smem[];
    WGT(wgt_, WGT_LAUUM, a);
    if (WM == 2) {
        lauum_tile<2>(U, Kinv, ld, a, w, blockIdx.x >> 2, blockIdx.x & 3, smem);
    } else if ((int)blockIdx.x < nfull) {
        lauum_tile<4>(U, Kinv, ld, a, w, blockIdx.x, 0, smem);
    } else {
        const int y = blockIdx.x - nfull;
        lauum_tile<2>(U, Kinv, ld, a, w, nfull + (y >> 2), y & 3, smem);
    }
}

// k_lauum<4>'s whole tiles [0, gridDim.x) on eight waves (lauum_tile<4>)
__global__ __launch_bounds__(512, 4) void k_lauum8(const double* __restrict__ U, double* __restrict__ Kinv, int ld, int a,
                                                   int w, const ExpertPtrs* __restrict__ bt, unsigned long long* stamp)
{
    LaunchStamp stamp_(stamp);
    if (bt) { U = GP(bt[blockIdx.y].U); Kinv = GP(bt[blockIdx.y].Kinv); }
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int ti, tj;
    tri_index(blockIdx.x, ti, tj);
    double* C = Kinv + (size_t)(ti * TILE) * ld + tj * TILE;
    d4 acc[2][4];
    acc_zero8(acc);
    tile_nt8<false>(U + (size_t)(ti * TILE) * ld, ld, U + (size_t)(tj * TILE) * ld, ld, (ti < a ? a : ti) * TILE,
                    (a + w) * TILE, acc, smem);
    if (ti < a) tile_out8<1>(C, ld, acc);
    else tile_out8<0>(C, ld, acc);
}

// ... and the tiles from x0 on as 64x64 quarters on four waves (the quarter branch of k_lauum<4>)
__global__ __launch_bounds__(256, 2) void k_lauum_rest(const double* __restrict__ U, double* __restrict__ Kinv, int ld,
                                                       int a, int w, int x0, const ExpertPtrs* __restrict__ bt)
{
    if (bt) { U = GP(bt[blockIdx.y].U); Kinv = GP(bt[blockIdx.y].Kinv); }
    extern __shared__ __attribute__((aligned(16))) char smem[];
    lauum_tile<2>(U, Kinv, ld, a, w, x0 + (blockIdx.x >> 2), blockIdx.x & 3, smem);
}

int launch_lauum(const double* U, double* Kinv, int ld, int a, int w, hipStream_t s, Batch bt)
{
    set_big_lds();
    const int tiles = tri_count(a + w);
    if (tiles * bt.count <= tune(TUNE_LAUUM_WM2_MAX)) {
        CUGP_LAUNCH(k_lauum<2>, dim3(tiles * 4, bt.count), dim3(256), Geo<2>::LDS, s, U, Kinv, ld, a, w, 0, bt.tab, take_stamp());
        return 2;
    } else {
        // (a whole-matrix product, a = 0, has k ranges from 1 to a+w tiles, longest first: its tail is short tiles
        //  already; the split is for the block-wise calls, whose tiles all take w k tiles)
        const int nfull = a > 0 ? split_round(tiles, bt.count) : tiles;
        if (tune(TUNE_WAVES8) != 0 && nfull > 0) {
            CUGP_LAUNCH(k_lauum8, dim3(nfull, bt.count), dim3(512), GEMM_LDS, s, U, Kinv, ld, a, w, bt.tab, take_stamp());
            if (tiles > nfull)
                hipLaunchKernelGGL(k_lauum_rest, dim3(4 * (tiles - nfull), bt.count), dim3(256), Geo<2>::LDS, s, U, Kinv, ld,
                                   a, w, nfull, bt.tab);
            return 4;
        }
        CUGP_LAUNCH(k_lauum<4>, dim3(nfull + 4 * (tiles - nfull), bt.count), dim3(256), GEMM_LDS, s, U, Kinv, ld,
                           a, w, nfull, bt.tab, take_stamp());
        return 4;
    }
}
