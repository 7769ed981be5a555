// sparse_z_device.h -- the gradient of the sparse model's bound with respect to the inducing inputs Z
// (cugp_sparse_bound_grad_z): the rectangular pass that knows dk / dz and its fixed-order sums.
// Plain fp64 arithmetic, __syncthreads and wave shuffles: no MFMA, no atomics, no inline assembly, no stamps, and no
// #ifdef around arithmetic -- the host check (tools/sparse_z_host_check.cpp) runs this text behind tools/host_emul.h
// under -fsanitize=address,undefined.
//
// Include-point contract.  Included INSIDE namespace cugp, behind sparse_device.h, after these are declared:
//   kernels.h                      HyperScalars, KERNEL_*
//   kernels.hip / host_emul.h      the d2 typedef and the device vocabulary (__device__, __global__, __shared__, threadIdx,
//                                  blockIdx, __syncthreads, __shfl_xor)
//   cov_device.h                   KT, DC, col4, sqdist_4x4, DivBy, div_prepare, div_by, ard_weights, matern_entry, ard_entry
//
// With H the factor ard_entry / matern_entry return as hh (SE and SE-ARD: k itself) and s_c = 1 / l^2 (ARD: w_c^2),
//   dk(z_j, x) / dz_jc = -H(z_j, x) (z_jc - x_c) s_c,   and with the weights the hyper-parameter gradient already forms,
//   dF / dz_jc = s_c [ sum_i G_c[i][j] H(x_i, z_j) (x_ic - z_jc)  over every chunk  +  sum_b (2 G_uu)[b][j] H(z_b, z_j) (z_bc - z_jc) ]
// (row j AND column j of Kuu move with z_j: the symmetric 2 G_uu enters with weight 1, not the 1/2 of the hyper-parameter
// trace; the diagonal and the jitter have no derivative; H is finite at zero distance and the difference exactly zero
// there, so a z_j on a data row needs no special case).  The library returns the gradient of -F.
// Every sum has a fixed order (no atomics, no arrival order): equal inputs and equal chunk_rows give equal bits.
// Both kernels: 256 threads, grid (blocks, 1).
#pragma once

// One pass over a weight matrix G ([rows >= 64 * row_tiles][ld]; row i = point x_i of Xr, column j = z_j: k_cross's and
// k_trace_cross's orientation, squared distances and entry formulas, so an entry has the bits they give it), with the
// rank-one part in registers: w_ij = G[i][j] + yv_i bv_j (yv null: none).  Per column j and feature c
//   S[j][c] = sum_i (w_ij H_ij) (x_ic - z_jc)
// the difference first, then the product (k_predict_grad's rule: sum u x - z sum u cancels where |x| >> |x - z|).
// Workgroup (ct, rg) = (blockIdx.x / ranges, blockIdx.x % ranges) owns the 64 columns ct and the row tiles
// [rg per, min((rg + 1) per, row_tiles)), walks them ascending and keeps its sums in registers, DC features at a time
// (d > DC: the walk is repeated per feature chunk).  The reduction index is the row:
//   thread   its tiles ascending, in a tile its four rows in index order
//   wave     the four lanes that share a column (lane ^ 16, lane ^ 32) by a butterfly of that shape
//   tile     the four waves through LDS as (w0 + w1) + (w2 + w3)
// and the workgroup stores its partial block to its own slot: part[rg * sstride + j * d + c], j < m only.
// Entries beyond row nr or column m contribute exact zeros and their points are never read.
template <bool ARD, int KIND>
__global__ __launch_bounds__(256) void k_trace_cross_z(const double* __restrict__ Xr, int nr, const double* __restrict__ Z,
                                                       int m, int d, int ld, HyperScalars h_arg,
                                                       const HyperScalars* __restrict__ hd, const double* __restrict__ G,
                                                       const double* __restrict__ yv, const double* __restrict__ bv,
                                                       int row_tiles, int per, int ranges, double* __restrict__ part,
                                                       size_t sstride)
{
#pragma clang fp contract(off)
    const HyperScalars h = ARD ? *hd : h_arg;
    const double* __restrict__ wts = ARD ? ard_weights(hd) : nullptr;
    __shared__ double xs[KT][DC + 1], ys[KT][DC + 1];
    __shared__ double ws[DC];
    __shared__ double red[4][KT][DC + 1];
    const int ct = blockIdx.x / ranges, rg = blockIdx.x % ranges;
    const int j0 = ct * KT;
    const int t0 = rg * per, t1 = (t0 + per < row_tiles) ? t0 + per : row_tiles;
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    double* __restrict__ out = part + (size_t)rg * sstride;
    double bj[4];
#pragma unroll
    for (int b = 0; b < 4; b++) bj[b] = yv ? bv[j0 + col4(tx, b)] : 0.0;
    const DivBy dl = div_prepare(h.ell_sq);
    for (int c0 = 0; c0 < d; c0 += DC) {
        const int dc = (d - c0 < DC) ? (d - c0) : DC;
        double acc[4][DC];
#pragma unroll
        for (int b = 0; b < 4; b++)
#pragma unroll
            for (int c = 0; c < DC; c++) acc[b][c] = 0.0;
        for (int rt = t0; rt < t1; rt++) {
            const int i0 = rt * KT;
            double wk[4][4];
            sqdist_4x4<ARD>(Xr, Z, nr, m, d, i0, j0, xs, ys, wk, wts, ws);
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
                        double kf, hh;
                        if constexpr (ARD) {
                            ard_entry<KIND>(wk[a][b], h.signal_var, kf, hh);
                        } else if constexpr (KIND == KERNEL_SE) {
                            kf = h.signal_var * exp(div_by(-wk[a][b] * 0.5, dl));
                            hh = kf;
                        } else {
                            double dk;
                            matern_entry<KIND>(div_by(wk[a][b], dl), h.signal_var, kf, dk, hh);
                        }
                        e = w * hh;
                    }
                    wk[a][b] = e;
                }
            }
            // sqdist_4x4 leaves the LAST feature chunk staged (unscaled coordinates, zero beyond nr and m): any other
            // chunk is staged again, as trace_cross_body's second sweep does
            if (c0 + DC < d) {
                __syncthreads();
                for (int e = t; e < KT * dc; e += 256) {
                    int r = e / dc, c = e - r * dc;
                    xs[r][c] = (i0 + r < nr) ? Xr[(size_t)(i0 + r) * d + c0 + c] : 0.0;
                    ys[r][c] = (j0 + r < m) ? Z[(size_t)(j0 + r) * d + c0 + c] : 0.0;
                }
                __syncthreads();
            }
#pragma unroll
            for (int c = 0; c < DC; c++) {
                if (c < dc) {
                    double xv[4], zv[4];
#pragma unroll
                    for (int a = 0; a < 4; a++) { xv[a] = xs[ty * 4 + a][c]; zv[a] = ys[col4(tx, a)][c]; }
#pragma unroll
                    for (int b = 0; b < 4; b++)
#pragma unroll
                        for (int a = 0; a < 4; a++) acc[b][c] = acc[b][c] + wk[a][b] * (xv[a] - zv[b]);
                }
            }
        }
        // (an empty range never reaches here with anything but zeros; the launcher makes none)
#pragma unroll
        for (int c = 0; c < DC; c++) {
            if (c < dc) {
#pragma unroll
                for (int b = 0; b < 4; b++) {
                    double v = acc[b][c];
                    v = v + __shfl_xor(v, 16, 64);
                    v = v + __shfl_xor(v, 32, 64);
                    if ((t & 63) < 16) red[t >> 6][col4(tx, b)][c] = v;
                }
            }
        }
        __syncthreads();
        for (int e = t; e < KT * dc; e += 256) {
            const int jl = e / dc, c = e - jl * dc;
            if (j0 + jl < m)
                out[(size_t)(j0 + jl) * d + c0 + c] = (red[0][jl][c] + red[1][jl][c]) + (red[2][jl][c] + red[3][jl][c]);
        }
        __syncthreads();
    }
}

// acc[e] = (first ? 0 : acc[e]) + part_0[e] + part_1[e] + ... in slot order over the m d outputs e = j d + c: the passes
// come chunks ascending, the square (Z, Z, 2 G_uu) last.  The last pass applies s_c (1 / l^2; wts given: ARD's w_c^2) and
// the sign once per output: out[e] = hout[e] (pinned) = -(s_c acc[e]), the gradient of -F.  Grid: (m d + 255) / 256.
__global__ __launch_bounds__(256) void k_trace_cross_z_finish(const double* __restrict__ part, size_t sstride, int nslots,
                                                              int m, int d, int first, int last, double ell_sq,
                                                              const double* __restrict__ wts, double* __restrict__ acc,
                                                              double* __restrict__ out, double* __restrict__ hout)
{
#pragma clang fp contract(off)
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)m * d) return;
    double s = first ? 0.0 : acc[e];
    for (int k = 0; k < nslots; k++) s = s + part[(size_t)k * sstride + e];
    acc[e] = s;
    if (last) {
        const int c = (int)(e % d);
        const double sc = wts ? wts[c] * wts[c] : 1.0 / ell_sq;
        const double r = -(sc * s);
        out[e] = r;
        hout[e] = r;
    }
}
