// sparse_gfx950.h -- sparse variational GP regression on inducing points (sparse.cpp): the two products that need the
// device, k_sparse_predict_cov (k_predict_cov's sibling) and k_sparse_gram (the TN product), each with its launcher and
// its launch plan; behind them the launchers of the emulable sparse kernels (sparse_device.h, sparse_z_device.h,
// sparse_targets_device.h, sparse_predict_device.h, sparse_shard_device.h): a *_device.h header is compiled by the host
// checks and cannot hold a launcher.
//
// Include-point contract.  Needs the device; also holds launchers.  Included by kernels.hip alone, INSIDE namespace cugp,
// after these are declared -- the file includes nothing and declares none of them:
//   kernels.h        TILE, CovFn, CovShape, SparseShape, SparseZShape, SparseFinalTargets, SPARSE_CHUNK_DEFAULT,
//                    SPARSE_GRAM_SLOTS, SPARSE_Z_SLOTS, SPT_GROUP, the launcher prototypes (launch_test_gemm_nt among them)
//   kernels.hip      d4, LaunchStamp, CUGP_LAUNCH, take_stamp, tri_count, ard_weights_ptr, CUGP_COV_KERNEL3, set_big_lds
//   tile_gfx950.h    BK, Geo, GEMM_LDS, tile_nt, tile_tn, acc_zero, tile_store, plan_ksplit
//   cov_device.h     tri_index, KT
//   sparse_device.h, sparse_z_device.h, sparse_targets_device.h, sparse_predict_device.h   the kernels launched below
#pragma once

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
    // (128x128 workgroups, two per CU; every chunk goes to scratch, k_sparse_gram_finish adds them)
    const KSplit k = plan_ksplit(c.cpad, SPARSE_GRAM_SLOTS / tiles, (size_t)mpad * mpad * sizeof(double), false);
    c.kstep = k.kstep; c.split = k.split;
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

// ---- launchers of the emulable sparse kernels ----
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
    hipLaunchKernelGGL(CUGP_COV_KERNEL3(cf, k_trace_cross), grid, dim3(256), 0, s, Xr, nr, Z, m, d, mpad, cf.h, cf.hd, G, yv,
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
    hipLaunchKernelGGL(CUGP_COV_KERNEL3(cf, k_trace_cross_z), dim3((mpad / KT) * z.ranges), dim3(256), 0, s, Xr, nr, Z, m, d,
                       mpad, cf.h, cf.hd, G, yv, bv, z.row_tiles, z.per, z.ranges, part, sstride);
    const double* wts = ard_weights_ptr(cf);
    hipLaunchKernelGGL(k_trace_cross_z_finish, dim3((unsigned)((sstride + 255) / 256)), dim3(256), 0, s, (const double*)part,
                       sstride, z.ranges, m, d, first ? 1 : 0, last ? 1 : 0, cf.h.ell_sq, wts, acc, out, hout);
}

void launch_sparse_predict_finish(const double* Wt, const double* Vt, const double* cp, int mpad, int nt, double sf2,
                                  double s2, double noise, double* mean, double* var, hipStream_t s)
{
    hipLaunchKernelGGL(k_sparse_predict_finish, dim3((nt + 3) / 4), dim3(256), 0, s, Wt, Vt, cp, mpad, nt, sf2, s2, noise,
                       mean, var);
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

// ---- the rows sharded over ranks (sparse_shard_device.h) ----
void launch_sparse_shard_reduce(const double* src, size_t rstride, size_t hdr, size_t slot, size_t off, size_t len, int world,
                                int nshards, double* out, hipStream_t s)
{
    if (len == 0) return;
    hipLaunchKernelGGL(k_sparse_shard_reduce, dim3((unsigned)std::min<size_t>((len + 255) / 256, 2048)), dim3(256), 0, s, src,
                       rstride, hdr, slot, off, len, world, nshards, out);
}

void launch_sparse_shard_sums(const double* part_uf, size_t nb_uf, int nl, double* out, hipStream_t s)
{
    hipLaunchKernelGGL(k_sparse_shard_sums, dim3(1), dim3(256), 0, s, part_uf, nb_uf, nl, out);
}

void launch_sparse_finalize_sharded(const SparseFinalSharded& f, const double* suf, const double* part_uu, size_t nb_uu, int nl,
                                    double* out, double* hout, hipStream_t s)
{
    hipLaunchKernelGGL(k_sparse_finalize_sharded, dim3(1), dim3(256), 0, s, f, suf, part_uu, nb_uu, nl, out, hout);
}
