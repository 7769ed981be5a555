// predict_gfx950.h -- prediction at test points: W = Ks L^-T on paired 64x64 tiles (k_predict_gemm), the joint predictive
// covariance (k_predict_cov, k_predict_cov_finish, k_zero_upper_diag) and the posterior draws (k_sample_finish), mean and
// variance (k_predict_finish, k_predict_finish_mv), the product of experts (k_poe_reduce, k_poe_reduce_mode); each
// launcher directly behind its kernel.  At the end the launchers of the emulable prediction kernels: a *_device.h header
// is compiled by the host checks and cannot hold a launcher, so k_predict_grad and k_predict_grad_finish (cov_device.h),
// k_predict_grad_batched, k_predict_grad_finish_batched and k_poe_reduce_grad (bcm_grad_device.h) are launched from here.
//
// Include-point contract.  Needs the device; also holds launchers.  Included by kernels.hip alone, INSIDE namespace cugp,
// after these are declared -- the file includes nothing and declares none of them:
//   kernels.h        TILE, HyperScalars, CovFn, CovShape, ExpertPtrs, Batch, ticket_count, predict_grad_tiles, tune and
//                    TUNE_COV_SPLIT, the launcher prototypes
//   kernels.hip      d2, d4, GP, LaunchStamp, CUGP_LAUNCH, take_stamp, tri_count, is_ard, ard_weights_ptr, CUGP_COV_KERNEL,
//                    set_big_lds
//   tile_gfx950.h    BK, Geo, GEMM_LDS, tile_nt, acc_zero, tile_store, plan_ksplit
//   cov_device.h     tri_index, wave_sum, KT, DC, col4, sqdist_4x4, DivBy, div_prepare, ard_weights, kernel_value,
//                    k_predict_grad, k_predict_grad_finish
//   bcm_grad_device.h  k_predict_grad_batched, k_predict_grad_finish_batched, k_poe_reduce_grad
// Declares for sparse.cpp's covariance too: predict_cov_shape and k_predict_cov_finish serve k_sparse_predict_cov as they are.
#pragma once

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

void launch_predict_gemm(const double* Ks, const double* T, double* W, int ld, int ntt, int nt, hipStream_t s,
                         Batch bt)
{
    set_big_lds();
    // (ntt, nt in 128-row tiles; the kernel works on 64-row tiles in pairs)
    CUGP_LAUNCH(k_predict_gemm, dim3(2 * ntt * nt, bt.count), dim3(256), Geo<2>::LDS, s, Ks, T, W, ld, 2 * ntt, 2 * nt,
                take_stamp(), bt.tab);
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

CovShape predict_cov_shape(int ntpad, int n)
{
    CovShape c;
    const int aim = tune(TUNE_COV_SPLIT);                 // 64x64 workgroup slots to fill (four per CU); 0 = no split
    const int t128 = tri_count(ntpad / TILE);
    c.wm = (aim > 0 && 4 * t128 <= aim) ? 2 : 4;
    c.tiles = c.wm == 2 ? tri_count(ntpad / 64) : t128;
    c.kend = (n + BK - 1) / BK * BK;
    // (128x128 workgroups: two per CU; chunk 0 is written in place, to the factor handle's A)
    const KSplit k = plan_ksplit(c.kend, aim / (c.wm == 2 ? 1 : 2) / c.tiles, (size_t)ntpad * ntpad * sizeof(double), true);
    c.kstep = k.kstep; c.split = k.split;
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
    const ShapeArgs sh = shape_args<KIND>(wts, d);
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
            double v = kernel_value<ARD, KIND>(d2v[a][b], dl, h.signal_var, sh);
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

void launch_predict_cov_finish(const double* Xt, int nt, int d, int ntpad, const CovFn& cf, bool with_noise,
                               double jitter, double* A, const double* scr, int nscr, unsigned* tickets, hipStream_t s)
{
    const dim3 grid(tri_count(ntpad / KT));
    hipLaunchKernelGGL(CUGP_COV_KERNEL(cf, k_predict_cov_finish), grid, dim3(256), 0, s, Xt, nt, d, ntpad, cf.h,
                       with_noise ? 1 : 0, jitter, A, scr, (size_t)ntpad * ntpad, nscr, tickets, cf.hd);
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

void launch_zero_upper_diag(double* A, int ld, int nt, hipStream_t s)
{
    hipLaunchKernelGGL(k_zero_upper_diag, dim3(nt), dim3(256), 0, s, A, ld);
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

void launch_sample_finish(const double* F, int ld, const double* mean, int nt, int ns, double* out, hipStream_t s)
{
    const size_t total = (size_t)nt * ns;
    hipLaunchKernelGGL(k_sample_finish, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, F, ld, mean, nt, ns, out);
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

void launch_predict_finish(const double* Ks, const double* W, const double* alpha, int n, int npad, int ntest,
                           HyperScalars h, double* mean, double* var, hipStream_t s, double* rows, size_t rstride,
                           int rhalf, int ntpad, Batch bt)
{
    hipLaunchKernelGGL(k_predict_finish, dim3((ntest + 3) / 4, bt.count), dim3(256), 0, s, Ks, W, alpha, n, npad,
                       ntest, h, mean, var, rows, rstride, rhalf, ntpad, bt.tab);
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

void launch_predict_finish_mv(const double* Ks, const double* W, int npad, int ntest, HyperScalars h, double* mean,
                              double* var, size_t row_stride, int ntpad, hipStream_t s, Batch bt)
{
    hipLaunchKernelGGL(k_predict_finish_mv, dim3((ntest + 3) / 4, bt.count), dim3(256), 0, s, Ks, W, npad, ntest, h, mean,
                       var, row_stride, ntpad, bt.tab);
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

void launch_poe_reduce(const double* g, size_t rstride, int world, int K, int nt, double* out, hipStream_t s)
{
    hipLaunchKernelGGL(k_poe_reduce, dim3((nt + 255) / 256), dim3(256), 0, s, g, rstride, world, K, nt, out);
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

void launch_poe_reduce_mode(const double* g, size_t rstride, int world, int K, int nt, int mode, double sf2, double sn2,
                            int with_noise, double* out, hipStream_t s)
{
    hipLaunchKernelGGL(k_poe_reduce_mode, dim3((nt + 255) / 256), dim3(256), 0, s, g, rstride, world, K, nt, mode, sf2,
                       sn2, with_noise, out);
}

// ---- launchers of the emulable prediction kernels (cov_device.h, bcm_grad_device.h) ----
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
    const double* wts = ard_weights_ptr(cf);
    hipLaunchKernelGGL(k_predict_grad_finish, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, part, pstride,
                       predict_grad_tiles(n), nt, d, cf.h.ell_sq, wts, dmean, dvar);
}

// ---- the batched launches of cugp_group_predict_grad_enqueue (blockIdx.y = expert) ----
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
    const double* wts = ard_weights_ptr(cf);
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
