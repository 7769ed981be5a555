// sparse_device.h -- sparse variational GP regression on inducing points (cugp_sparse_*; Titsias 2009, DESIGN.md section
// 25): every pass of it except the products on the MFMA tile (k_sparse_gram: sparse_gfx950.h, with the launchers)
// and what reads the labels -- q, y'y, H and the final sums: sparse_targets_device.h, which the handle's own y runs with
// p = 1.  Plain fp64 arithmetic, __syncthreads and wave shuffles: no MFMA, no atomics, no inline assembly, no stamps, and no
// #ifdef around arithmetic -- the host check (tools/sparse_host_check.cpp) runs this text behind tools/host_emul.h under
// -fsanitize=address,undefined.
//
// Include-point contract.  Included INSIDE namespace cugp, after these are declared -- the file declares none of them:
//   kernels.h                      TILE, HyperScalars, KERNEL_*
//   kernels.hip / host_emul.h      the d2 typedef and the device vocabulary (__device__, __global__, __shared__, threadIdx,
//                                  blockIdx, gridDim, __syncthreads, __shfl_xor, __shfl_down)
//   cov_device.h                   tri_index, wave_sum, KT, DC, col4, sqdist_4x4, DivBy, div_prepare, div_by, ard_weights,
//                                  matern_entry, ard_entry
//
// With M inducing inputs Z (padded to mp = a multiple of 128), N data rows in chunks of C rows, s2 = sn2 = exp(2 theta_n):
//   Kuu = k(Z, Z) + eps I = Lu Lu^T,  W_c = k(X_c, Z) Lu^-T  ([C][mp], one row per data row),
//   P = sum_c W_c^T W_c,  q = sum_c W_c^T y_c,  B = I + P / s2 = LB LB^T,  c' = LB^-1 q (= s2 c),
//   F = -N/2 log 2 pi - 1/2 log|B| - N/2 log s2 - y'y / (2 s2) + c''c' / (2 s2^2) - N sf2 / (2 s2) + tr P / (2 s2)
//   gamma' = LB^-T c',  beta' = Lu^-T gamma',  H = I - B^-1 - gamma' gamma'^T / s2^2,  H2 = H - P / s2,
//   R = Lu^-T H / s2,  G_c^T = W_c R^T + y_c (beta' / s2^2)^T  ([C][mp]),  2 G_uu = Lu^-T H2 Lu^-1,
//   dF / dtheta_j = sum G_c^T o dk(X_c, Z) / dtheta_j + 1/2 sum (2 G_uu) o dk(Z, Z) / dtheta_j   (theta_f: - N sf2 / s2)
// Every sum below has a fixed order (no atomics, no arrival order): repeated launches give identical bits.
// All kernels: 256 threads, grid (blocks, 1).
#pragma once

// lower 128-tile `tile` (tri_index order) of an ld x ld matrix in 16 blocks of 8 rows: the element offset of the thread's
// four consecutive entries
__device__ __forceinline__ size_t sparse_tile_offset(int ld)
{
    int ti, tj;
    tri_index(blockIdx.x >> 4, ti, tj);
    const int r = (blockIdx.x & 15) * 8 + (threadIdx.x >> 5), c = (threadIdx.x & 31) * 4;
    return (size_t)(ti * TILE + r) * ld + tj * TILE + c;
}

// P (lower 128-tiles, diagonal tiles complete) = (first ? 0 : P) + S_0 + S_1 + ... + S_{nscr - 1}: the split-k partial
// products of k_sparse_gram, added in index order.  Grid: 16 * lower tiles.
__global__ __launch_bounds__(256) void k_sparse_gram_finish(double* __restrict__ P, int ld, const double* __restrict__ scr,
                                                            size_t pstride, int nscr, int first)
{
#pragma clang fp contract(off)
    const size_t off = sparse_tile_offset(ld);
    d2 a = *(const d2*)(scr + off), b = *(const d2*)(scr + off + 2);
    if (!first) {
        a = *(const d2*)(P + off) + a;
        b = *(const d2*)(P + off + 2) + b;
    }
    for (int s = 1; s < nscr; s++) {
        const double* q = scr + (size_t)s * pstride + off;
        a = a + *(const d2*)q;
        b = b + *(const d2*)(q + 2);
    }
    *(d2*)(P + off) = a;
    *(d2*)(P + off + 2) = b;
}

// Bm (lower 128-tiles, diagonal tiles complete) = I + P / s2: what the factorisation reads.  Grid: 16 * lower tiles.
__global__ __launch_bounds__(256) void k_sparse_form_b(const double* __restrict__ P, int ld, double s2, double* __restrict__ Bm)
{
#pragma clang fp contract(off)
    int ti, tj;
    tri_index(blockIdx.x >> 4, ti, tj);
    const int i = ti * TILE + (blockIdx.x & 15) * 8 + (threadIdx.x >> 5), j0 = tj * TILE + (threadIdx.x & 31) * 4;
    const size_t off = (size_t)i * ld + j0;
#pragma unroll
    for (int e = 0; e < 4; e++) Bm[off + e] = (i == j0 + e ? 1.0 : 0.0) + P[off + e] / s2;
}

// dst[i][k] = src[k][i] * scale, ld x ld; one 64x64 tile per workgroup through LDS (rows padded to 65), grid (ld / 64)^2
__global__ __launch_bounds__(256) void k_sparse_transpose(const double* __restrict__ src, double* __restrict__ dst, int ld,
                                                          double scale)
{
#pragma clang fp contract(off)
    __shared__ double tile[KT][KT + 1];
    const int nb = ld / KT, bi = blockIdx.x / nb, bj = blockIdx.x % nb, t = threadIdx.x;
    for (int e = t; e < KT * KT; e += 256) tile[e >> 6][e & 63] = src[(size_t)(bj * KT + (e >> 6)) * ld + bi * KT + (e & 63)];
    __syncthreads();
    for (int e = t; e < KT * KT; e += 256) dst[(size_t)(bi * KT + (e >> 6)) * ld + bj * KT + (e & 63)] = tile[e & 63][e >> 6] * scale;
}

// The rectangular gradient pass: over the 64x64 tiles of a weight matrix G ([rows >= 64 * row tiles][ld], row i = point
// x_i of Xr, column j = point z_j of Z) the sums  sum_ij w_ij dk(x_i, z_j) / dtheta  with
//   w_ij = G[i][j] + yv_i bv_j     (the rank-one part in registers; yv null: none)
// k_cross's orientation, squared distances and entry formulas (sqdist_4x4<ARD>(Xr, Z, ..), div_by, matern_entry,
// ard_entry): an entry here has the bits k_cross gives it.  Isotropic: sum w o dK/dlog l and sum w o K; ARD:
// trace_ard_body's two sweeps -- the d per-dimension sums of w H ((x_ic - z_jc) w_c)^2, then sum w o K.  No noise term,
// no doubling, no diagonal: the rectangle is summed as it stands (the Kuu term is the same pass on (Z, Z, 2 G_uu)).
// Entries beyond row nr or column m contribute exact zeros and their points are never read.
// Partials column-major: part[c * pstride + pofs + block], c = 0 .. nl - 1 the length-scale columns (nl = 1, ARD d),
// nl: sum w o K.  Grid: row tiles * (ld / 64).
template <bool ARD, int KIND>
__device__ __forceinline__ void trace_cross_body(const double* __restrict__ Xr, int nr, const double* __restrict__ Z, int m,
                                                 int d, int ld, HyperScalars h_arg, const HyperScalars* __restrict__ hd,
                                                 const double* __restrict__ G, const double* __restrict__ yv,
                                                 const double* __restrict__ bv, double* __restrict__ part, size_t pstride,
                                                 size_t pofs)
{
#pragma clang fp contract(off)
    const HyperScalars h = ARD ? *hd : h_arg;
    const double* __restrict__ wts = ARD ? ard_weights(hd) : nullptr;
    __shared__ double xs[KT][DC + 1], ys[KT][DC + 1];
    __shared__ double ws[DC];
    __shared__ double red[DC][4];
    const int nct = ld / KT;
    const int i0 = (blockIdx.x / nct) * KT, j0 = (blockIdx.x % nct) * KT;
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const int nl = ARD ? d : 1;
    double* __restrict__ out = part + pofs + blockIdx.x;
    double wk[4][4];
    sqdist_4x4<ARD>(Xr, Z, nr, m, d, i0, j0, xs, ys, wk, wts, ws);
    double bj[4];
#pragma unroll
    for (int b = 0; b < 4; b++) bj[b] = yv ? bv[j0 + col4(tx, b)] : 0.0;
    const DivBy dl = div_prepare(h.ell_sq);
    double s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int a = 0; a < 4; a++) {
        const int i = i0 + ty * 4 + a;
        const double yi = (yv && i < nr) ? yv[i] : 0.0;
        const double* gr = G + (size_t)i * ld + j0 + tx * 2;
        d2 g01 = *(const d2*)gr, g23 = *(const d2*)(gr + 32);
        const double gv[4] = {g01[0], g01[1], g23[0], g23[1]};
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const int j = j0 + col4(tx, b);
            double e = 0.0;
            if (i < nr && j < m) {
                const double w = gv[b] + yi * bj[b];
                double kf, dk, hh;
                if constexpr (ARD) {
                    ard_entry<KIND>(wk[a][b], h.signal_var, kf, hh);
                    dk = 0.0;
                } else if constexpr (KIND == KERNEL_SE) {
                    kf = h.signal_var * exp(div_by(-wk[a][b] * 0.5, dl));
                    dk = kf * div_by(wk[a][b], dl);
                    hh = 0.0;
                } else {
                    matern_entry<KIND>(div_by(wk[a][b], dl), h.signal_var, kf, dk, hh);
                }
                e = w * hh;
                s1 += w * dk;
                s2 += w * kf;
            }
            wk[a][b] = e;
        }
    }
    s1 = wave_sum(s1); s2 = wave_sum(s2);
    if ((t & 63) == 0) { red[0][t >> 6] = s1; red[1][t >> 6] = s2; }
    __syncthreads();
    // (t = 0: the isotropic length-scale column; the ARD ones follow below)
    if (t < 2 && (t > 0 || !ARD))
        out[(size_t)(t == 0 ? 0 : nl) * pstride] = (red[t][0] + red[t][1]) + (red[t][2] + red[t][3]);
    if constexpr (ARD) {
        for (int c0 = 0; c0 < d; c0 += DC) {
            const int dc = (d - c0 < DC) ? (d - c0) : DC;
            __syncthreads();
            for (int e = t; e < KT * dc; e += 256) {
                int r = e / dc, c = e - r * dc;
                xs[r][c] = (i0 + r < nr) ? Xr[(size_t)(i0 + r) * d + c0 + c] : 0.0;
                ys[r][c] = (j0 + r < m) ? Z[(size_t)(j0 + r) * d + c0 + c] : 0.0;
            }
            if (t < dc) ws[t] = wts[c0 + t];
            __syncthreads();
            double gs[DC];
#pragma unroll
            for (int c = 0; c < DC; c++) {
                gs[c] = 0.0;
                if (c < dc) {
                    double xv[4], yv4[4];
#pragma unroll
                    for (int a = 0; a < 4; a++) { xv[a] = xs[ty * 4 + a][c]; yv4[a] = ys[col4(tx, a)][c]; }
                    const double wc = ws[c];
                    double acc = 0.0;
#pragma unroll
                    for (int a = 0; a < 4; a++)
#pragma unroll
                        for (int b = 0; b < 4; b++) {
                            const double df = (xv[a] - yv4[b]) * wc;
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
            if (t < dc) out[(size_t)(c0 + t) * pstride] = (red[t][0] + red[t][1]) + (red[t][2] + red[t][3]);
        }
    }
}

template <bool ARD, int KIND>
__global__ __launch_bounds__(256) void k_trace_cross(const double* __restrict__ Xr, int nr, const double* __restrict__ Z,
                                                     int m, int d, int ld, HyperScalars h_arg,
                                                     const HyperScalars* __restrict__ hd, const double* __restrict__ G,
                                                     const double* __restrict__ yv, const double* __restrict__ bv,
                                                     double* __restrict__ part, size_t pstride, size_t pofs)
{
    trace_cross_body<ARD, KIND>(Xr, nr, Z, m, d, ld, h_arg, hd, G, yv, bv, part, pstride, pofs);
}

// Prediction at the test rows of one pass: Wt = k(Xt, Z) Lu^-T and Vt = Wt LB^-T ([>= nt][ld], zero beyond column m),
//   mean_t = (sum_i Vt[t][i] c'_i) / s2,   var_t = ((sf2 - sum_i Wt[t][i]^2) + sum_i Vt[t][i]^2) + noise
// One wave per test row: lane l adds the columns l, l + 64, ... ascending, the lanes by wave_sum.  Grid: (nt + 3) / 4.
__global__ __launch_bounds__(256) void k_sparse_predict_finish(const double* __restrict__ Wt, const double* __restrict__ Vt,
                                                               const double* __restrict__ cp, int ld, int nt, double sf2,
                                                               double s2, double noise, double* __restrict__ mean,
                                                               double* __restrict__ var)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int r = row < nt ? row : nt - 1;                 // (whole waves shuffle: the spare ones repeat the last row)
    const double* w = Wt + (size_t)r * ld;
    const double* v = Vt + (size_t)r * ld;
    double sm = 0.0, sw = 0.0, sv = 0.0;
    for (int i = lane; i < ld; i += 64) {
        sm = sm + v[i] * cp[i];
        sw = sw + w[i] * w[i];
        sv = sv + v[i] * v[i];
    }
    sm = wave_sum(sm); sw = wave_sum(sw); sv = wave_sum(sv);
    if (lane == 0 && row < nt) {
        mean[row] = sm / s2;
        var[row] = ((sf2 - sw) + sv) + noise;
    }
}
