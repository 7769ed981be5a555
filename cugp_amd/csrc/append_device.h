// append_device.h -- the kernels of cugp_append (k_append_border, k_append_kinv): bordering arithmetic, barriers and
// wave_sum, plus ONE call of the fp64 MFMA tile product.  kernels.hip includes it for gfx950; tools/append_host_check.cpp
// includes the same text behind the emulation shim tools/host_emul.h with plain-loop stand-ins for the tile product.
//
// Include-point contract.  Included INSIDE namespace cugp, after these are declared -- the file declares none of them:
//   kernels.h                      TILE
//   cov_device.h                   tri_index, wave_sum
//   kernels.hip / host_emul.h      the d4 typedef, the device vocabulary, and CUGP_DYN_LDS(name): the workgroup's dynamic
//                                  LDS (kernels.hip: the extern __shared__ declaration; the shim: a null pointer)
//   tile_gfx950.h / the check      the tile product: acc_zero, tile_nt, tile_accum_store
// The launchers (launch_append_border, launch_append_kinv) are in dense_features_gfx950.h.
#pragma once

// ------------------------------------------------------------------------------------------
// Appending observations (cugp_append): one bordering step of the factor, its inverse and K^-1 by k <= 128 new rows
// [r0, r0 + k) that lie in ONE tile row.  The existing launches have left P = B L^-T and V = P L^-1 ([128][ld], zero
// beyond row k and column r0), and the factor handle holds C = chol(S) (Cf, lower) and C^-1 (Ci, lower, exact zeros
// above the diagonal), both ld = 128 with identity beyond k, and sum log C_ii (flog).
//   Q = -C^-1 V,  zb = C^-1 (yb - P z):
//   L' = [L 0; P C]   T' = [T 0; Q C^-1]   U' = T'^T   K'^-1 = [K^-1 + Q'Q, . ; C^-T Q, C^-T C^-1]   z' = [z; zb]
// Every sum runs over its index in ascending order in one thread (the dot products P z: per lane, then the fixed shuffle
// tree of wave_sum): no atomics, the same bits on every call.
// ------------------------------------------------------------------------------------------
constexpr int APB_COLS = 32;                 // old columns per workgroup of k_append_border: 32 columns x 8 row groups
constexpr int APPEND_QT_LD = TILE;           // Qt[j][i] = Q[i][j], k-contiguous, zero beyond k: the operand of k_append_kinv

// blockIdx.x < nq: the old columns [32 b, 32 b + 32) -- new rows of A (P), of T (Q), new columns of U, bottom rows of
// K^-1 (C^-T Q) and the rows of Qt (zero for columns >= r0: nq covers whole 64-row tiles of Qt).  blockIdx.x == nq: the
// corner -- C, C^-1, C^-T C^-1, the tails of z and alpha, the tile's log-determinant share.
__global__ __launch_bounds__(256) void k_append_border(const double* __restrict__ P, const double* __restrict__ V,
                                                       const double* __restrict__ Cf, const double* __restrict__ Ci,
                                                       const double* __restrict__ flog, int r0, int k, int ld, int nq,
                                                       double* __restrict__ A, double* __restrict__ T,
                                                       double* __restrict__ U, double* __restrict__ Kinv,
                                                       const double* __restrict__ y, double* __restrict__ z,
                                                       double* __restrict__ alpha, double* __restrict__ logdet,
                                                       double* __restrict__ Qt)
{
#pragma clang fp contract(off)
    __shared__ double qs[TILE][APB_COLS + 1];
    const int t = threadIdx.x;
    if ((int)blockIdx.x < nq) {
        const int cc = t & (APB_COLS - 1), rg = t / APB_COLS, c = blockIdx.x * APB_COLS + cc;
        const bool old = c < r0;
        for (int i = rg; i < TILE; i += 256 / APB_COLS) {
            double q = 0.0;
            if (old && i < k) {
                const double* ci = Ci + (size_t)i * TILE;
                for (int m = 0; m <= i; m++) q -= ci[m] * V[(size_t)m * ld + c];
                T[(size_t)(r0 + i) * ld + c] = q;
                A[(size_t)(r0 + i) * ld + c] = P[(size_t)i * ld + c];
            }
            qs[i][cc] = q;
        }
        __syncthreads();
        if (old)
            for (int i = rg; i < k; i += 256 / APB_COLS) {
                double s = 0.0;
                for (int m = i; m < k; m++) s += Ci[(size_t)m * TILE + i] * qs[m][cc];
                Kinv[(size_t)(r0 + i) * ld + c] = s;
                if (c >= r0 / TILE * TILE) Kinv[(size_t)c * ld + r0 + i] = s;     // (diagonal 128-tiles are kept complete)
            }
        // the transposed copies, k-contiguous stores: thread = (new row i, every second column)
        const int i = t & (TILE - 1);
        for (int c2 = t >> 7; c2 < APB_COLS; c2 += 2) {
            const int col = blockIdx.x * APB_COLS + c2;
            const double q = qs[i][c2];
            Qt[(size_t)col * APPEND_QT_LD + i] = q;
            if (col < r0 && i < k) U[(size_t)col * ld + r0 + i] = q;
        }
        return;
    }
    // ---- corner ----
    double* res = &qs[0][0];                 // yb - P z, then kept
    double* zb = res + TILE;
    const int lane = t & 63, wave = t >> 6;
    for (int i = wave; i < k; i += 4) {
        const double* p = P + (size_t)i * ld;
        double s = 0.0;
        for (int j = lane; j < r0; j += 64) s += p[j] * z[j];
        s = wave_sum(s);
        if (lane == 0) res[i] = y[r0 + i] - s;
    }
    __syncthreads();
    if (t < k) {
        double s = 0.0;
        for (int m = 0; m <= t; m++) s += Ci[(size_t)t * TILE + m] * res[m];
        zb[t] = s;
        z[r0 + t] = s;
    }
    __syncthreads();
    if (t < k) {
        double s = 0.0;
        for (int m = t; m < k; m++) s += Ci[(size_t)m * TILE + t] * zb[m];
        alpha[r0 + t] = s;
    }
    for (int e = t; e < k * k; e += 256) {
        const int i = e / k, j = e - i * k;
        const size_t ij = (size_t)(r0 + i) * ld + r0 + j, ji = (size_t)(r0 + j) * ld + r0 + i;
        if (j <= i) {
            const double ci = Ci[(size_t)i * TILE + j];
            A[ij] = Cf[(size_t)i * TILE + j];
            T[ij] = ci;
            U[ji] = ci;
            double s = 0.0;
            for (int m = i; m < k; m++) s += Ci[(size_t)m * TILE + i] * Ci[(size_t)m * TILE + j];
            Kinv[ij] = s;
            Kinv[ji] = s;
        } else {
            T[ij] = 0.0;
            U[ji] = 0.0;
        }
    }
    if (t == 0) logdet[r0 / TILE] = logdet[r0 / TILE] + flog[0];
}

// K^-1[0, r0) += Q'Q on its lower 64x64 tiles, diagonal 128-tiles complete (k_lauum's layout), and alpha[0, r0) += Q' zb.
// Tile (ti, tj): the fp64 MFMA product of Qt's row tiles ti and tj over the k16 = k rounded up to 16 columns (zero beyond
// k), added onto the tile in the epilogue (tile_accum_store): every tile is read once and written once -- the launch is
// bound by that traffic.  Rows of Qt at and beyond r0 are zero: the tile that straddles r0 adds exact zeros to the new
// rows.  blockIdx.x < lower: the lower tiles ti >= tj; then `tiles - lower` upper-right quadrants (2 e, 2 e + 1) of the
// diagonal 128-tiles; blockIdx.x >= tiles: 256 rows of alpha each, the k terms in index order.
__global__ __launch_bounds__(256, 2) void k_append_kinv(const double* __restrict__ Qt, int k16, int k, int r0, int ld,
                                                        int lower, int tiles, double* __restrict__ Kinv,
                                                        const double* __restrict__ zb, double* __restrict__ alpha)
{
    CUGP_DYN_LDS(smem);
    if ((int)blockIdx.x >= tiles) {
#pragma clang fp contract(off)
        const int j = (blockIdx.x - tiles) * 256 + threadIdx.x;
        if (j >= r0) return;
        const double* q = Qt + (size_t)j * APPEND_QT_LD;
        double s = 0.0;
        for (int i = 0; i < k; i++) s += q[i] * zb[i];
        alpha[j] = alpha[j] + s;
        return;
    }
    int ti, tj;
    if ((int)blockIdx.x < lower) tri_index(blockIdx.x, ti, tj);
    else { ti = 2 * (blockIdx.x - lower); tj = ti + 1; }
    d4 acc[2][2];
    acc_zero(acc);
    tile_nt<false>(Qt + (size_t)ti * 64 * APPEND_QT_LD, APPEND_QT_LD, Qt + (size_t)tj * 64 * APPEND_QT_LD, APPEND_QT_LD, 0,
                   k16, acc, smem);
    tile_accum_store<1>(Kinv + (size_t)ti * 64 * ld + tj * 64, ld, acc);
}
