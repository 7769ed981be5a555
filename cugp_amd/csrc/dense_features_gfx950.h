// dense_features_gfx950.h -- the optional features of a dense model (dense_features.cpp): multi-target regression
// (k_targets_alpha and its batched form, k_targets_mean, k_trace_targets, k_finalize_targets), appending observations
// and leave-one-out cross-validation.  The kernels of the last two are emulable (append_device.h, loo_device.h) except the
// one product k_loo_product, which is here; a *_device.h header is compiled by the host checks and cannot hold a launcher,
// so their launchers are here as well.  Each launcher directly behind its kernel.
//
// Include-point contract.  Needs the device; also holds launchers.  Included by kernels.hip alone, INSIDE namespace cugp,
// after these are declared -- the file includes nothing and declares none of them:
//   kernels.h        TILE, HyperScalars, CovFn, ExpertPtrs, Batch, TARGETS_MEAN_KSTEP, APB_COLS, tune and
//                    TUNE_LAUUM_WM2_MAX, the launcher prototypes
//   kernels.hip      d4, GP, CUGP_LAUNCH, tri_count, is_ard, CUGP_COV_KERNEL, set_big_lds
//   tile_gfx950.h    BK, Geo, GEMM_LDS, tile_nt, acc_zero, tile_store
//   cov_device.h     tri_index, wave_sum, KT, trace_ard_body
//   eval_gfx950.h    FIN_THREADS, FinalizeArgs, trace_body
//   chol_gfx950.h    split_round
//   append_device.h  k_append_border, k_append_kinv
//   loo_device.h     k_loo_point, k_loo_sum, k_loo_mirror_scale, k_loo_bsum, k_trace_loo, k_loo_finalize
#pragma once

// Multi-target regression: m target vectors over the handle's one factorisation (cugp_set_targets).  Everything is
// target-major, [mpad][npad] with zeros beyond n and beyond m: Y the targets, Z = Y L^-T (k_predict_gemm as it stands),
// A = Z L^-1 (row t = alpha_t, k_targets_alpha), then ONE pass over K^-1 for the gradient of the summed objective
// (k_trace_targets), the final sums (k_finalize_targets) and the means A Ks^T (k_targets_mean).
// The kernels have bodies of their own: the single-target kernels above keep their instructions.

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

void launch_targets_alpha(const double* Z, const double* U, double* A, int npad, int m, hipStream_t s)
{
    const int m64 = (m + 63) / 64, n64 = npad / 64;
    hipLaunchKernelGGL(k_targets_alpha, dim3(m64 * (n64 / 2)), dim3(256), Geo<2>::LDS, s, Z, U, A, npad, m64, n64);
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

void launch_targets_alpha_batched(const double* Z, double* A, int npad, int m, hipStream_t s, Batch bt)
{
    const int m64 = (m + 63) / 64, n64 = npad / 64;
    hipLaunchKernelGGL(k_targets_alpha_batched, dim3(m64 * (n64 / 2), bt.count), dim3(256), Geo<2>::LDS, s, Z, A, npad, m64,
                       n64, bt.tab);
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

void launch_trace_targets(const double* X, int n, int d, int npad, const CovFn& cf, const double* Kinv, const double* A,
                          int m, double* part, hipStream_t s)
{
    const dim3 grid(tri_count(npad / KT));
    hipLaunchKernelGGL(CUGP_COV_KERNEL(cf, k_trace_targets), grid, dim3(256), 0, s, X, n, d, npad, cf.h, Kinv, A, m, part,
                       cf.hd);
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

// The same for a handle with ONE tied length scale over dlen length columns (nl: length and shape columns; nh = nl - dlen
// + 3): k_finalize_ard_tied's order for the columns (all waves, then the index-order sum by thread 0), this kernel's for everything else.  Lines repeated, not shared, so
// that k_finalize_targets keeps its instructions.
__global__ __launch_bounds__(FIN_THREADS) void k_finalize_targets_tied(const double* __restrict__ Z, int npad, int n, int m,
                                                                       double logdet, const double* __restrict__ part,
                                                                       int nblocks, int nl, int dlen,
                                                                       const HyperScalars* __restrict__ hd,
                                                                       double* __restrict__ out, double* __restrict__ hout)
{
#pragma clang fp contract(off)
    const HyperScalars h = *hd;
    const int o = nl - dlen + 1, nh = o + 2;
    __shared__ double red[FIN_THREADS];
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
    double g0 = 0.0, s2 = 0.0;                             // (thread 0's)
    for (int c0 = 0; c0 < nl + 2; c0 += FIN_THREADS) {     // k_finalize_ard_tied's order: every column on its wave, FIN_THREADS at a time
        const int cc = (nl + 2 - c0 < FIN_THREADS) ? (nl + 2 - c0) : FIN_THREADS;
        __syncthreads();
        for (int c = wave; c < cc; c += FIN_THREADS / 64) {
            const double* col = part + (size_t)(c0 + c) * nblocks;
            double s = 0.0;
            for (int i = lane; i < nblocks; i += 64) s += col[i];
            s = wave_sum(s);
            if (lane == 0) red[c] = s;
        }
        __syncthreads();
        if (t == 0)
            for (int c = c0; c < c0 + cc; c++) {
                const double s = red[c - c0];
                if (c < dlen) g0 = c == 0 ? s / 2.0 : g0 + s / 2.0;
                else if (c < nl) out[2 + (c - dlen)] = dead ? logdet : s / 2.0;
                else if (c == nl) s2 = s;
                else {
                    const double s3 = s;
                    out[1 + o] = dead ? logdet : (2.0 * s2 - 2.0 * h.noise_var * s3) / 2.0;
                    out[2 + o] = dead ? logdet : (2.0 * h.noise_var * s3) / 2.0;
                }
            }
    }
    if (t == 0) out[1] = dead ? logdet : g0;
    __syncthreads();
    double ll = 0.0;
    for (int t0 = 0; t0 < m; t0 += FIN_THREADS) {
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

void launch_finalize_targets(const double* Z, int npad, int n, int d, int m, double logdet, const double* part,
                             const CovFn& cf, double* out, double* hout, hipStream_t s)
{
    const int nl = d + shape_count(cf.kind);
    if (is_ard(cf) && cf.tied)
        hipLaunchKernelGGL(k_finalize_targets_tied, dim3(1), dim3(FIN_THREADS), 0, s, Z, npad, n, m, logdet, part,
                           tri_count(npad / KT), nl, d, cf.hd, out, hout);
    else
        hipLaunchKernelGGL(k_finalize_targets, dim3(1), dim3(FIN_THREADS), 0, s, Z, npad, n, m, logdet, part,
                           tri_count(npad / KT), is_ard(cf) ? nl : -1, cf.h, is_ard(cf) ? cf.hd : nullptr, out, hout);
}

// ---- appending observations: the launchers of append_device.h's kernels ----
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
    const int nl = is_ard(cf) ? d + shape_count(cf.kind) : 1;
    if (is_ard(cf) && cf.tied)
        hipLaunchKernelGGL(k_loo_finalize_tied, dim3(1), dim3(256), 0, s, (const double*)part, nblocks, nl, d,
                           cf.h.noise_var, out, hout);
    else
        hipLaunchKernelGGL(k_loo_finalize, dim3(1), dim3(256), 0, s, (const double*)part, nblocks, nl, cf.h.noise_var, out,
                           hout);
}
