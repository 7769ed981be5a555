// loo_device.h -- leave-one-out cross-validation from the factored model (cugp_loo, cugp_loo_predict):
// every pass of it except the one tile product (k_loo_product: dense_features_gfx950.h, with the launchers).  Plain fp64 arithmetic, __syncthreads and
// wave shuffles: no MFMA, no atomics, no inline assembly, no stamps, and no #ifdef around arithmetic -- the host check
// (tools/loo_host_check.cpp) runs this text behind tools/host_emul.h under -fsanitize=address,undefined.
//
// Include-point contract.  Included INSIDE namespace cugp, after these are declared -- the file declares none of them:
//   kernels.h                      TILE, HyperScalars, KERNEL_*
//   kernels.hip / host_emul.h      the d2 typedef and the device vocabulary (__device__, __global__, __shared__, threadIdx,
//                                  blockIdx, gridDim, __syncthreads, __shfl_xor, __shfl_down)
//   cov_device.h                   tri_index, wave_sum, KT, DC, col4, sqdist_4x4, DivBy, div_prepare, div_by, ard_weights,
//                                  matern_entry, ard_entry
//
// With kappa_i = [K^-1]_ii (GPML 5.10-5.13) and c = the fp64 value of the literal 1.83787 (the constant LL uses):
//   mu_i = y_i - alpha_i / kappa_i,   var_i = 1 / kappa_i,   l_i = 1/2 log kappa_i - alpha_i^2 / (2 kappa_i) - c / 2,
//   L_LOO = sum_i l_i
//   a_i = alpha_i / kappa_i,  c_i = (1 + alpha_i a_i) / kappa_i (> 0),  s_i = sqrt(c_i),  b = K^-1 a,
//   B = K^-1 diag(s),  P = B B^T = K^-1 diag(c) K^-1,  W_loo = P - b alpha^T - alpha b^T,
//   d(-L_LOO) / dtheta_j = 1/2 tr(W_loo dK_j): the marginal likelihood's gradient pass with W_loo in the place of W.
// Every sum below has a fixed order (no atomics, no arrival order): repeated launches give identical bits.
// All kernels: 256 threads, grid (blocks, 1).
#pragma once

// rows of the per-point buffer pt[LOO_ROWS][npad]; rows >= n of every one are zero
enum { LOO_MEAN = 0, LOO_VAR = 1, LOO_LOGP = 2, LOO_A = 3, LOO_S = 4, LOO_ROWS = 5 };

// grid npad / 256: one thread per row.  K^-1 is read on its diagonal alone.
__global__ __launch_bounds__(256) void k_loo_point(const double* __restrict__ Kinv, const double* __restrict__ alpha,
                                                   const double* __restrict__ y, int n, int npad,
                                                   double* __restrict__ pt)
{
#pragma clang fp contract(off)
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= npad) return;
    double mean = 0.0, var = 0.0, lp = 0.0, a = 0.0, s = 0.0;
    if (i < n) {                                       // (the padding of K^-1 is the identity: it contributes nothing)
        const double kap = Kinv[(size_t)i * npad + i], al = alpha[i];
        a = al / kap;
        mean = y[i] - a;
        var = 1.0 / kap;
        lp = (0.5 * log(kap) - (al * al) / (2.0 * kap)) - 0.5 * 1.83787;
        s = __builtin_sqrt((1.0 + al * a) / kap);
    }
    pt[(size_t)LOO_MEAN * npad + i] = mean;
    pt[(size_t)LOO_VAR * npad + i] = var;
    pt[(size_t)LOO_LOGP * npad + i] = lp;
    pt[(size_t)LOO_A * npad + i] = a;
    pt[(size_t)LOO_S * npad + i] = s;
}

// one workgroup: L_LOO = sum_i l_i -- thread t adds the rows t, t + 256, ... ascending, the lanes of a wave by wave_sum,
// the four waves as (w0 + w1) + (w2 + w3).  out: the device results row, hout: its pinned host copy; entry 0 of both.
__global__ __launch_bounds__(256) void k_loo_sum(const double* __restrict__ pt, int npad, double* __restrict__ out,
                                                 double* __restrict__ hout)
{
#pragma clang fp contract(off)
    __shared__ double red[4];
    const int t = threadIdx.x;
    const double* lp = pt + (size_t)LOO_LOGP * npad;
    double s = 0.0;
    for (int i = t; i < npad; i += 256) s = s + lp[i];
    s = wave_sum(s);
    if ((t & 63) == 0) red[t >> 6] = s;
    __syncthreads();
    if (t == 0) {
        const double v = (red[0] + red[1]) + (red[2] + red[3]);
        out[0] = v;
        hout[0] = v;
    }
}

// B[i][k] = K^-1(i, k) s_k for i, k < n and 0 elsewhere, a full row-major npad x npad operand, from the lower 64x64 tiles
// of K^-1: entry (i, k) is read at (max, min) -- inside the lower triangle of the diagonal tiles too, which is all the
// gradient traces and cugp_append rely on.  One 64x64 output tile (bi, bj) per workgroup, grid (npad / 64)^2; the source
// tile goes through LDS (rows padded to 65: the transposed reads of an upper tile hit 64 different banks).
// The same pass gives the tile's share of b = K^-1 a: bpart[bj][i] = sum_{k in tile bj} K^-1(i, k) a_k, four lanes per
// row with 16 consecutive k each, added in index order and then across the four lanes by a butterfly of fixed shape;
// k_loo_bsum adds the shares in tile order.
__global__ __launch_bounds__(256) void k_loo_mirror_scale(const double* __restrict__ Kinv, const double* __restrict__ pt,
                                                          int n, int npad, double* __restrict__ B,
                                                          double* __restrict__ bpart)
{
#pragma clang fp contract(off)
    __shared__ double tile[KT][KT + 1];
    __shared__ double ss[KT], sa[KT];
    const int nb = npad / KT;
    const int bi = blockIdx.x / nb, bj = blockIdx.x % nb;
    const int si = bi > bj ? bi : bj, sj = bi > bj ? bj : bi;
    const int t = threadIdx.x;
    for (int e = t; e < KT * KT; e += 256) {
        const int r = e >> 6, c = e & 63;
        tile[r][c] = Kinv[(size_t)(si * KT + r) * npad + sj * KT + c];
    }
    if (t < KT) {
        const int k = bj * KT + t;
        ss[t] = k < n ? pt[(size_t)LOO_S * npad + k] : 0.0;
        sa[t] = k < n ? pt[(size_t)LOO_A * npad + k] : 0.0;
    }
    __syncthreads();
    for (int e = t; e < KT * KT; e += 256) {
        const int r = e >> 6, c = e & 63;
        const int i = bi * KT + r, k = bj * KT + c;
        const bool direct = bi > bj || (bi == bj && c <= r);
        const double v = direct ? tile[r][c] : tile[c][r];
        B[(size_t)i * npad + k] = (i < n && k < n) ? v * ss[c] : 0.0;
    }
    const int r = t >> 2, q = t & 3, i = bi * KT + r;
    double acc = 0.0;
    for (int c = q * 16; c < q * 16 + 16; c++) {
        const bool direct = bi > bj || (bi == bj && c <= r);
        const double v = direct ? tile[r][c] : tile[c][r];
        if (i < n && bj * KT + c < n) acc = acc + v * sa[c];
    }
    acc = acc + __shfl_xor(acc, 1, 4);
    acc = acc + __shfl_xor(acc, 2, 4);
    if (q == 0) bpart[(size_t)bj * npad + i] = acc;
}

// b_i = bpart[0][i] + bpart[1][i] + ... in tile order; grid npad / 256
__global__ __launch_bounds__(256) void k_loo_bsum(const double* __restrict__ bpart, int npad, double* __restrict__ b)
{
#pragma clang fp contract(off)
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= npad) return;
    const int nb = npad / KT;
    double s = bpart[i];
    for (int j = 1; j < nb; j++) s = s + bpart[(size_t)j * npad + i];
    b[i] = s;
}

// The gradient pass over the lower 64x64 tiles of P (grid: their number, tri_index order), k_trace's tile, thread layout,
// entry formulas, doubling of the off-diagonal entries and diagonal handling, with
//   W_loo(i, j) = (P(i, j) - b_i alpha_j) - alpha_i b_j
// formed per 4x4 block in registers.  Isotropic: the three sums of k_trace (sum W o dK/dlog l, sum W o K, tr W); ARD:
// trace_ard_body's two sweeps (d per-dimension sums, then the same two).  Partial sums column-major for both:
// part[c * nblocks + block], c = 0 .. nl - 1 the length-scale columns (nl = 1, ARD d), nl: sum W o K, nl + 1: tr W; a
// family with a shape parameter (RQ) has its column sum W o dK/dtheta_shape between the length columns and sum W o K.
// h_arg: the hyper-scalars by value (isotropic); hd: the same in device memory followed by the d weights (ARD, mandatory).
template <bool ARD, int KIND>
__device__ __forceinline__ void trace_loo_body(const double* __restrict__ X, int n, int d, int npad, HyperScalars h_arg,
                                               const HyperScalars* __restrict__ hd, const double* __restrict__ P,
                                               const double* __restrict__ alpha, const double* __restrict__ bv,
                                               double* __restrict__ part)
{
#pragma clang fp contract(off)
    const HyperScalars h = ARD ? *hd : h_arg;
    const double* __restrict__ wts = ARD ? ard_weights(hd) : nullptr;
    __shared__ double xs[KT][DC + 1], ys[KT][DC + 1];
    __shared__ double ws[DC];
    __shared__ double red[DC][4];
    int ti, tj;
    tri_index(blockIdx.x, ti, tj);
    const int i0 = ti * KT, j0 = tj * KT;
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const size_t nblocks = gridDim.x;
    const int nl = ARD ? d : 1;
    double wk[4][4];
    sqdist_4x4<ARD>(X, X, n, n, d, i0, j0, xs, ys, wk, wts, ws);
    double aj[4], bj[4];
#pragma unroll
    for (int b = 0; b < 4; b++) { aj[b] = alpha[j0 + col4(tx, b)]; bj[b] = bv[j0 + col4(tx, b)]; }
    const DivBy dl = div_prepare(h.ell_sq);
    double s1 = 0.0, s2 = 0.0, s3 = 0.0;
    constexpr int NS = ARD ? shape_count(KIND) : 0;      // shape columns behind the length columns (RQ: one); their sum rides in s1
    const ShapeArgs sh = shape_args<KIND>(wts, d);
#pragma unroll
    for (int a = 0; a < 4; a++) {
        const int i = i0 + ty * 4 + a;
        const double ai = alpha[i], bi = bv[i];
        const double* pr = P + (size_t)i * npad + j0 + tx * 2;
        d2 p01 = *(const d2*)pr, p23 = *(const d2*)(pr + 32);
        const double pv[4] = {p01[0], p01[1], p23[0], p23[1]};
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const int j = j0 + col4(tx, b);
            double e = 0.0;
            if (i < n && j < n && (ti != tj || j <= i)) {
                const double w = (pv[b] - bi * aj[b]) - ai * bj[b];
                double kf, dk, hh;
                if constexpr (NS > 0) {
                    ard_entry<KIND>(wk[a][b], h.signal_var, sh, kf, hh, dk);   // dk: dK / dtheta_shape, zero on the diagonal
                } else if constexpr (ARD) {
                    ard_entry<KIND>(wk[a][b], h.signal_var, kf, hh);
                    dk = 0.0;
                } else if constexpr (KIND == KERNEL_SE) {
                    kf = h.signal_var * exp(div_by(-wk[a][b] * 0.5, dl));
                    dk = kf * div_by(wk[a][b], dl);
                    hh = 0.0;
                } else {
                    matern_entry<KIND>(div_by(wk[a][b], dl), h.signal_var, kf, dk, hh);
                }
                if (i == j) {
                    kf += h.noise_var;
                    s1 += w * dk;
                    s2 += w * kf;
                    s3 += w;
                } else {
                    e = 2.0 * (w * hh);
                    s1 += 2.0 * (w * dk);
                    s2 += 2.0 * (w * kf);
                }
            }
            wk[a][b] = e;
        }
    }
    s1 = wave_sum(s1); s2 = wave_sum(s2); s3 = wave_sum(s3);
    if ((t & 63) == 0) { red[0][t >> 6] = s1; red[1][t >> 6] = s2; red[2][t >> 6] = s3; }
    __syncthreads();
    // (t = 0: the isotropic length-scale column; the ARD ones follow below)
    if constexpr (NS > 0) {                              // [d length columns][shape column = s1][sum W o K][tr W]
        if (t < 3) part[(size_t)(t == 0 ? d : d + NS + t - 1) * nblocks + blockIdx.x] = (red[t][0] + red[t][1]) + (red[t][2] + red[t][3]);
    } else
    if (t < 3 && (t > 0 || !ARD))
        part[(size_t)(t == 0 ? 0 : nl + t - 1) * nblocks + blockIdx.x] = (red[t][0] + red[t][1]) + (red[t][2] + red[t][3]);
    if constexpr (ARD) {
        for (int c0 = 0; c0 < d; c0 += DC) {
            const int dc = (d - c0 < DC) ? (d - c0) : DC;
            __syncthreads();
            for (int e = t; e < KT * dc; e += 256) {
                int r = e / dc, c = e - r * dc;
                xs[r][c] = (i0 + r < n) ? X[(size_t)(i0 + r) * d + c0 + c] : 0.0;
                ys[r][c] = (j0 + r < n) ? X[(size_t)(j0 + r) * d + c0 + c] : 0.0;
            }
            if (t < dc) ws[t] = wts[c0 + t];
            __syncthreads();
            double gs[DC];
#pragma unroll
            for (int c = 0; c < DC; c++) {
                gs[c] = 0.0;
                if (c < dc) {
                    double xv[4], yv[4];
#pragma unroll
                    for (int a = 0; a < 4; a++) { xv[a] = xs[ty * 4 + a][c]; yv[a] = ys[col4(tx, a)][c]; }
                    const double wc = ws[c];
                    double acc = 0.0;
#pragma unroll
                    for (int a = 0; a < 4; a++)
#pragma unroll
                        for (int b = 0; b < 4; b++) {
                            const double df = (xv[a] - yv[b]) * wc;
                            acc = acc + wk[a][b] * (df * df);
                        }
                    gs[c] = wave_sum(acc);
                }
            }
            if ((t & 63) == 0) {
#pragma unroll
                for (int c = 0; c < DC; c++) red[c][t >> 6] = gs[c];
            }
            __syncthreads();
            if (t < dc) part[(size_t)(c0 + t) * nblocks + blockIdx.x] = (red[t][0] + red[t][1]) + (red[t][2] + red[t][3]);
        }
    }
}

template <bool ARD, int KIND>
__global__ __launch_bounds__(256) void k_trace_loo(const double* __restrict__ X, int n, int d, int npad,
                                                   HyperScalars h_arg, const HyperScalars* __restrict__ hd,
                                                   const double* __restrict__ P, const double* __restrict__ alpha,
                                                   const double* __restrict__ bv, double* __restrict__ part)
{
    trace_loo_body<ARD, KIND>(X, n, d, npad, h_arg, hd, P, alpha, bv, part);
}

// one workgroup: the final sums of the gradient pass and the nh = nl + 2 components of d(-L_LOO) / dtheta in the handle's
// order.  Wave w takes the columns w, w + 4, ...: lane l adds the blocks l, l + 64, ... ascending, the lanes by wave_sum.
//   g_c = S_c / 2 (c < nl),  g_f = (2 s2 - 2 sn2 s3) / 2,  g_n = (2 sn2 s3) / 2     (k_finalize's and k_finalize_ard's formulas)
// out / hout: the results row, entries 1 .. nh.
__global__ __launch_bounds__(256) void k_loo_finalize(const double* __restrict__ part, int nblocks, int nl, double sn2,
                                                      double* __restrict__ out, double* __restrict__ hout)
{
#pragma clang fp contract(off)
    __shared__ double tail[2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int c = wave; c < nl + 2; c += 4) {
        const double* col = part + (size_t)c * nblocks;
        double s = 0.0;
        for (int i = lane; i < nblocks; i += 64) s = s + col[i];
        s = wave_sum(s);
        if (lane == 0 && c < nl) { out[1 + c] = s / 2.0; hout[1 + c] = s / 2.0; }
        if (lane == 0 && c >= nl) tail[c - nl] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double s2 = tail[0], s3 = tail[1];
        const double gf = (2.0 * s2 - 2.0 * sn2 * s3) / 2.0, gn = (2.0 * sn2 * s3) / 2.0;
        out[1 + nl] = gf; out[2 + nl] = gn;
        hout[1 + nl] = gf; hout[2 + nl] = gn;
    }
}

// The same for a handle with ONE tied length scale over dlen length columns (nl counts a family's shape columns with the
// length columns; nh = nl - dlen + 3): every column summed on its wave as above, 256 at a time into LDS; thread 0 adds the
// dlen finished results S_c / 2 in index order into g_0, the other columns' results move up behind it (k_finalize_ard_tied's order).  Lines repeated, not
// shared, so that k_loo_finalize keeps its instructions.
__global__ __launch_bounds__(256) void k_loo_finalize_tied(const double* __restrict__ part, int nblocks, int nl, int dlen,
                                                           double sn2, double* __restrict__ out, double* __restrict__ hout)
{
#pragma clang fp contract(off)
    constexpr int COLS = 256;                              // columns summed per round: wave w takes w, w + 4, ...
    __shared__ double cols[COLS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int o = nl - dlen + 1;
    double g0 = 0.0, s2 = 0.0;                             // (thread 0's)
    for (int c0 = 0; c0 < nl + 2; c0 += COLS) {
        const int cc = (nl + 2 - c0 < COLS) ? (nl + 2 - c0) : COLS;
        __syncthreads();
        for (int c = wave; c < cc; c += 4) {
            const double* col = part + (size_t)(c0 + c) * nblocks;
            double s = 0.0;
            for (int i = lane; i < nblocks; i += 64) s = s + col[i];
            s = wave_sum(s);
            if (lane == 0) cols[c] = s;
        }
        __syncthreads();
        if (threadIdx.x == 0)
            for (int c = c0; c < c0 + cc; c++) {
                const double s = cols[c - c0];
                if (c < dlen) g0 = c == 0 ? s / 2.0 : g0 + s / 2.0;
                else if (c < nl) { out[2 + (c - dlen)] = s / 2.0; hout[2 + (c - dlen)] = s / 2.0; }
                else if (c == nl) s2 = s;
                else {
                    const double s3 = s;
                    const double gf = (2.0 * s2 - 2.0 * sn2 * s3) / 2.0, gn = (2.0 * sn2 * s3) / 2.0;
                    out[1 + o] = gf; out[2 + o] = gn;
                    hout[1 + o] = gf; hout[2 + o] = gn;
                }
            }
    }
    if (threadIdx.x == 0) { out[1] = g0; hout[1] = g0; }
}
