// iter_gfx950.h -- the fused covariance-times-vectors product of the matrix-free exact GP (cugp_iter_*; DESIGN.md section
// 33), and the launchers of it and of iter_device.h's vector kernels.
//
// Include-point contract.  Included INSIDE namespace cugp by kernels.hip, after kernels.h (ITER_*, IterPlan, CovFn), the
// d2 / d4 typedefs, CUGP_COV_KERNEL, cov_device.h (DC, DivBy, div_prepare, ard_weights, ShapeArgs, shape_args,
// kernel_value) and iter_device.h (the vector kernels).
//
// k_cov_apply<ARD, KIND>:  out[i][c] = sum_j k(a_i, b_j) V[j][c]  (+ sn2 V[i][c], square form), K in registers only.
//   v_mfma_f64_16x16x4_f64 takes A from lane (fr = lane & 15, fk = lane >> 4) as A[row fr][k fk]: the lane computes the
//   ONE entry k(a_{i0 + fr}, b_{j + fk}) and hands it to the MFMA as it is.  B is V[j + fk][16 ct + fr] out of the LDS image
//   of the stage's V rows; the entry feeds NCT MFMAs (column tiles).  C/D: lane holds rows fk + 4 r, column fr.
//   Workgroup: 4 waves x 16 rows = ITER_ROWS output rows; the wave's 16 a rows sit in registers, DC features at a time (d <=
//   DC: loaded once).  It sweeps its stages of ITER_JT b rows in ascending j: per stage 8 squared distances per lane --
//   differences before squares, (x - x') w squared and added in feature order, no contraction, sqdist_4x4's arithmetic
//   -- then 8 kernel_value, then 8 NCT MFMAs.  The next stage's b rows (first feature chunk) and V rows are in flight in
//   registers meanwhile and go into the other LDS buffer behind the MFMAs: one barrier per stage.  Feature chunks beyond
//   the first are staged through a third buffer inside the stage (two barriers per chunk: d > 16 only).
//   Rows of b and V beyond nb are staged as zeros: k 0 = 0.  No two waves share an output: no atomics; a column's sums
//   run j ascending, 4 per MFMA, and do not depend on the other columns.
//   LDS: ys [2][32][16], yc [32][16], vs [2][32][TPL] doubles, TPL = 16 (one column tile) | 80 (four; 64 + 16: the row stride
//   is 128 B mod 256 B so that the two k rows of a half-wave's ds_read_b64 fall on different banks): 16 KiB | 52 KiB.
//   grid (row blocks, split): workgroup (., s) sums the stages [s per, (s + 1) per) and, split > 1, writes its partial block
//   part[s][na][tp]; k_cov_apply_finish adds the blocks in ascending s (first copied, then a = a + b) and applies the noise
//   term.  sn2 V[i][c] enters once, by one fma: one rounding.
#pragma once

template <bool ARD, int KIND, int NCT>
__device__ __forceinline__ void cov_apply_body(const double* __restrict__ A, int na, const double* __restrict__ B, int nb, int d,
                                               const HyperScalars* __restrict__ hd, const double* __restrict__ V,
                                               double* __restrict__ out, int per, int square)
{
#pragma clang fp contract(off)
    constexpr int TP = NCT * 16, TPL = (TP % 32 == 0) ? TP + 16 : TP, NK = ITER_JT / 4;
    static_assert(ITER_JT * DC == 2 * 256 && ITER_JT * TP == 2 * 256 * NCT, "one d2 of b and NCT d2 of V per thread and stage");
    __shared__ __attribute__((aligned(16))) double ys[2][ITER_JT][DC];
    __shared__ __attribute__((aligned(16))) double yc[ITER_JT][DC];
    __shared__ __attribute__((aligned(16))) double vs[2][ITER_JT][TPL];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fk = lane >> 4;
    const int row = blockIdx.x * ITER_ROWS + wave * 16 + fr;
    const HyperScalars h = *hd;
    const double* __restrict__ wts = ard_weights(hd);
    const DivBy dl = div_prepare(h.ell_sq);
    ShapeArgs sh = ShapeArgs{0.0, 0.0};
    if constexpr (KIND == KERNEL_RQ) sh = shape_args<KIND>(wts, d);
    const int nst = (nb + ITER_JT - 1) / ITER_JT, nch = (d + DC - 1) / DC;
    const int s0 = blockIdx.y * per, s1 = s0 + per < nst ? s0 + per : nst;

    d4 acc[NCT];
#pragma unroll
    for (int ct = 0; ct < NCT; ct++) acc[ct] = (d4){0.0, 0.0, 0.0, 0.0};
    double ar[DC];
    auto load_a = [&](int c0) {
#pragma unroll
        for (int c = 0; c < DC; c++) ar[c] = (row < na && c0 + c < d) ? A[(size_t)row * d + c0 + c] : 0.0;
    };
    // the thread's share of a stage: one feature pair of one b row, NCT column pairs of V rows
    const int br = tid >> 3, bc = (tid & 7) * 2;
    d2 rb, rv[NCT];
    auto fetch_b = [&](int j0, int c0) {
        const int j = j0 + br, c = c0 + bc;
        rb[0] = (j < nb && c < d) ? B[(size_t)j * d + c] : 0.0;
        rb[1] = (j < nb && c + 1 < d) ? B[(size_t)j * d + c + 1] : 0.0;
    };
    auto fetch = [&](int st) {
        const int j0 = st * ITER_JT;
        fetch_b(j0, 0);
#pragma unroll
        for (int q = 0; q < NCT; q++) {
            const int e = tid + 256 * q, j = j0 + e / (TP / 2);
            rv[q] = j < nb ? *(const d2*)(V + (size_t)j * TP + 2 * (e % (TP / 2))) : (d2){0.0, 0.0};
        }
    };
    auto put = [&](int buf) {
        *(d2*)&ys[buf][br][bc] = rb;
#pragma unroll
        for (int q = 0; q < NCT; q++) {
            const int e = tid + 256 * q;
            *(d2*)&vs[buf][e / (TP / 2)][2 * (e % (TP / 2))] = rv[q];
        }
    };
    double sq[NK];
    // sq[kk] += the chunk's terms of |(a_row - b_{4 kk + fk}) w|^2, features ascending (a feature beyond d: 0 - 0)
    auto accumulate = [&](double (*yb)[DC], int c0) {
#pragma unroll
        for (int cp = 0; cp < DC / 2; cp++) {
            const int c = 2 * cp;
            if (c0 + c < d) {
                const double w0 = ARD ? wts[c0 + c] : 1.0, w1 = (ARD && c0 + c + 1 < d) ? wts[c0 + c + 1] : 1.0;
#pragma unroll
                for (int kk = 0; kk < NK; kk++) {
                    const d2 yv = *(const d2*)&yb[kk * 4 + fk][c];
                    double df = ar[c] - yv[0];
                    if (ARD) df = df * w0;
                    sq[kk] = sq[kk] + df * df;
                    df = ar[c + 1] - yv[1];
                    if (ARD) df = df * w1;
                    sq[kk] = sq[kk] + df * df;
                }
            }
        }
    };

    load_a(0);
    fetch(s0);
    put(0);
    __syncthreads();
    for (int st = s0; st < s1; st++) {
        const int cur = (st - s0) & 1;
        const bool more = st + 1 < s1;
        if (more) fetch(st + 1);
#pragma unroll
        for (int kk = 0; kk < NK; kk++) sq[kk] = 0.0;
        accumulate(ys[cur], 0);
        for (int ch = 1; ch < nch; ch++) {
            const d2 keep = rb;
            fetch_b(st * ITER_JT, ch * DC);
            __syncthreads();
            *(d2*)&yc[br][bc] = rb;
            rb = keep;
            load_a(ch * DC);
            __syncthreads();
            accumulate(yc, ch * DC);
        }
        if (nch > 1) load_a(0);
#pragma unroll
        for (int kk = 0; kk < NK; kk++) {
            const double kv = kernel_value<ARD, KIND>(sq[kk], dl, h.signal_var, sh);
#pragma unroll
            for (int ct = 0; ct < NCT; ct++)
                acc[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(kv, vs[cur][kk * 4 + fk][ct * 16 + fr], acc[ct], 0, 0, 0);
        }
        if (more) put(cur ^ 1);
        __syncthreads();
    }
    const bool direct = gridDim.y == 1;
    double* __restrict__ o = out + (size_t)blockIdx.y * na * TP;
#pragma unroll
    for (int ct = 0; ct < NCT; ct++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int i = blockIdx.x * ITER_ROWS + wave * 16 + fk + 4 * r;
            if (i < na) {
                const size_t e = (size_t)i * TP + ct * 16 + fr;
                double v = acc[ct][r];
                if (square && direct) v = __builtin_fma(h.noise_var, V[e], v);
                o[e] = v;
            }
        }
}

// one column tile (t <= 16) and four (t <= 64): the two instantiations of the body per covariance family
template <bool ARD, int KIND>
__global__ __launch_bounds__(256) void k_cov_apply(const double* __restrict__ A, int na, const double* __restrict__ B, int nb,
                                                   int d, const HyperScalars* __restrict__ hd, const double* __restrict__ V,
                                                   double* __restrict__ out, int per, int square)
{
    cov_apply_body<ARD, KIND, 1>(A, na, B, nb, d, hd, V, out, per, square);
}
template <bool ARD, int KIND>
__global__ __launch_bounds__(256) void k_cov_apply4(const double* __restrict__ A, int na, const double* __restrict__ B, int nb,
                                                    int d, const HyperScalars* __restrict__ hd, const double* __restrict__ V,
                                                    double* __restrict__ out, int per, int square)
{
    cov_apply_body<ARD, KIND, 4>(A, na, B, nb, d, hd, V, out, per, square);
}

// out[e] = part[0][e] + part[1][e] + ... in range order (+ sn2 V[e] by one fma: square), e < cnt = na * tp
__global__ __launch_bounds__(256) void k_cov_apply_finish(const double* __restrict__ part, int split, size_t cnt,
                                                          const HyperScalars* __restrict__ hd, const double* __restrict__ V,
                                                          int square, double* __restrict__ out)
{
#pragma clang fp contract(off)
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= cnt) return;
    double s = part[e];
    for (int k = 1; k < split; k++) s = s + part[(size_t)k * cnt + e];
    out[e] = square ? __builtin_fma(hd->noise_var, V[e], s) : s;
}

IterPlan iter_apply_plan(int na, int nb, int force)
{
    IterPlan p;
    p.row_blocks = (int)(((size_t)na + ITER_ROWS - 1) / ITER_ROWS);
    p.stages = (int)(((size_t)nb + ITER_JT - 1) / ITER_JT);
    int want = force;
    if (want <= 0) {
        want = p.row_blocks >= ITER_SLOTS ? 1 : (ITER_SLOTS + p.row_blocks - 1) / p.row_blocks;
        want = std::min(want, std::min(ITER_MAX_SPLIT, p.stages / ITER_MIN_STAGES));
    }
    want = std::max(1, std::min(want, std::min(p.stages, 65535)));     // (gridDim.y; cugp.h CUGP_ITER_MAX_SPLIT)
    p.per = (p.stages + want - 1) / want;
    p.split = (p.stages + p.per - 1) / p.per;          // no empty range
    return p;
}

void launch_cov_apply(const double* A, int na, const double* B, int nb, int d, const CovFn& cf, const double* V, int tp,
                      double* out, double* part, const IterPlan& pl, bool square, hipStream_t s)
{
    assert(cf.hd && (tp == 16 || tp == IT_MAXT) && (pl.split == 1 || part));
    auto kern = tp == 16 ? CUGP_COV_KERNEL(cf, k_cov_apply) : CUGP_COV_KERNEL(cf, k_cov_apply4);
    hipLaunchKernelGGL(kern, dim3(pl.row_blocks, pl.split), dim3(256), 0, s, A, na, B, nb, d, cf.hd, V,
                       pl.split > 1 ? part : out, pl.per, square ? 1 : 0);
    if (pl.split > 1) {
        const size_t cnt = (size_t)na * tp;
        hipLaunchKernelGGL(k_cov_apply_finish, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, s, part, pl.split, cnt, cf.hd, V,
                           square ? 1 : 0, out);
    }
}

// ---- the bilinear forms of dKf / dtheta (cugp_iter_grad_forms, cugp_iter_loglik_grad) ----
//
// k_cov_grad<ARD, KIND>:  G_h = sum_ij W_ij dKf_ij / dtheta_h with W_ij = sum_c U[i][c] V[j][c], neither K nor W stored.
//   k_cov_apply's decomposition with the MFMA's roles swapped: there the lane computes an entry and the MFMA multiplies it
//   with V; here the MFMA forms the weights and the lane multiplies them with the entries' derivative factors.  The wave
//   computes the TRANSPOSED weight tile D[j][i] = sum_c V[j][c] U[i][c]: A[row fr][k fk] = V[j0 + fr][4 kk + fk] out of the LDS
//   image of the stage's V rows, B[k fk][col fr] = U[i0 + fr][4 kk + fk], fixed for the whole sweep and held in registers
//   (TP / 4 doubles per lane); c ascending, 4 per MFMA.  In the C/D layout the lane then holds j = j0 + fk + 4 r and the one
//   i = i0 + fr -- the 8 entries per stage (two 16-row j tiles; entry kk = 4 jt + r is b row 4 kk + fk) whose squared
//   distances k_cov_apply's lane computes against the a row it keeps in registers: the same lines, the same bits.  Per entry:
//   the family's factors once (cov_device.h: ard_entry, rq_entry, matern_entry; isotropic SE kernel_value and the quotient
//   k_trace takes), times the weight.  ARD route: e = w H is kept for the 8 entries and a second loop over the features of
//   the workgroup's chunk (blockIdx.z; read again from the stage's LDS image) adds e ((a_c - b_c) w_c)^2 into DC per-lane sums
//   that live across the sweep; every z recomputes the whole distance (d > DC is served, not tuned), z = 0 alone writes the
//   scalar columns.  The full square: W is not symmetric.
//   LDS: ys, yc as k_cov_apply's, yz [32][16] (the z-th chunk of a stage with d > DC), vs [2][32][TP + 2] (rows 144 B | 528 B
//   apart: the 32 lanes of a half-wave's ds_read_b64 -- fr x two fk -- fall on 32 different 8-byte bank pairs): 21 | 46 KiB.
//   Sums: a lane adds its entries in ascending j (kk ascending, stages ascending), wave_sum, the four waves (0 + 1) + (2 + 3):
//   one partial row part[(row block * split + s)][nc] per workgroup, nc = d + shape columns + 1 (sum W o Kf) on the ARD route,
//   2 (sum W o dKf/dlog l, sum W o Kf) else; k_cov_grad_finish adds the rows in ascending order (first copied, then a = a + b).
//   Rows beyond n enter as zeros with zero weight; padding columns of U and V add exact zeros.  No atomics.
template <bool ARD, int KIND, int NCT>
__device__ __forceinline__ void cov_grad_body(const double* __restrict__ X, int n, int d, const HyperScalars* __restrict__ hd,
                                              const double* __restrict__ U, const double* __restrict__ V,
                                              double* __restrict__ part, int per)
{
#pragma clang fp contract(off)
    constexpr int TP = NCT * 16, TPL = TP + 2, NK = ITER_JT / 4, NS = shape_count(KIND);
    static_assert(ITER_JT * DC == 2 * 256 && ITER_JT * TP == 2 * 256 * NCT, "one d2 of b and NCT d2 of V per thread and stage");
    static_assert(ITER_JT == 32 && ITER_ROWS == 64, "two 16-row j tiles per stage, four waves of 16 i rows");
    __shared__ __attribute__((aligned(16))) double ys[2][ITER_JT][DC];
    __shared__ __attribute__((aligned(16))) double yc[ITER_JT][DC];
    __shared__ __attribute__((aligned(16))) double yz[ARD ? ITER_JT : 1][DC];
    __shared__ __attribute__((aligned(16))) double vs[2][ITER_JT][TPL];
    __shared__ double red[DC + 2][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fk = lane >> 4;
    const int row = blockIdx.x * ITER_ROWS + wave * 16 + fr;
    const HyperScalars h = *hd;
    const double* __restrict__ wts = ard_weights(hd);
    [[maybe_unused]] const DivBy dl = div_prepare(h.ell_sq);   // isotropic route only
    const ShapeArgs sh = shape_args<KIND>(wts, d);
    const int nst = (n + ITER_JT - 1) / ITER_JT, nch = (d + DC - 1) / DC;
    const int s0 = blockIdx.y * per, s1 = s0 + per < nst ? s0 + per : nst;
    const int cz = ARD ? blockIdx.z : 0;               // the feature chunk of this workgroup's per-dimension sums

    double ub[TP / 4];                                 // the MFMA's B operand: U[row][4 kk + fk]
#pragma unroll
    for (int kk = 0; kk < TP / 4; kk++) ub[kk] = row < n ? U[(size_t)row * TP + kk * 4 + fk] : 0.0;
    double ar[DC];
    auto load_a = [&](int c0) {
#pragma unroll
        for (int c = 0; c < DC; c++) ar[c] = (row < n && c0 + c < d) ? X[(size_t)row * d + c0 + c] : 0.0;
    };
    // the thread's share of a stage: one feature pair of one b row, NCT column pairs of V rows
    const int br = tid >> 3, bc = (tid & 7) * 2;
    d2 rb, rv[NCT];
    auto fetch_b = [&](int j0, int c0) {
        const int j = j0 + br, c = c0 + bc;
        rb[0] = (j < n && c < d) ? X[(size_t)j * d + c] : 0.0;
        rb[1] = (j < n && c + 1 < d) ? X[(size_t)j * d + c + 1] : 0.0;
    };
    auto fetch = [&](int st) {
        const int j0 = st * ITER_JT;
        fetch_b(j0, 0);
#pragma unroll
        for (int q = 0; q < NCT; q++) {
            const int e = tid + 256 * q, j = j0 + e / (TP / 2);
            rv[q] = j < n ? *(const d2*)(V + (size_t)j * TP + 2 * (e % (TP / 2))) : (d2){0.0, 0.0};
        }
    };
    auto put = [&](int buf) {
        *(d2*)&ys[buf][br][bc] = rb;
#pragma unroll
        for (int q = 0; q < NCT; q++) {
            const int e = tid + 256 * q;
            *(d2*)&vs[buf][e / (TP / 2)][2 * (e % (TP / 2))] = rv[q];
        }
    };
    double sq[NK];
    // sq[kk] += the chunk's terms of |(a_row - b_{4 kk + fk}) w|^2, features ascending: k_cov_apply's lines
    auto accumulate = [&](double (*yb)[DC], int c0) {
#pragma unroll
        for (int cp = 0; cp < DC / 2; cp++) {
            const int c = 2 * cp;
            if (c0 + c < d) {
                const double w0 = ARD ? wts[c0 + c] : 1.0, w1 = (ARD && c0 + c + 1 < d) ? wts[c0 + c + 1] : 1.0;
#pragma unroll
                for (int kk = 0; kk < NK; kk++) {
                    const d2 yv = *(const d2*)&yb[kk * 4 + fk][c];
                    double df = ar[c] - yv[0];
                    if (ARD) df = df * w0;
                    sq[kk] = sq[kk] + df * df;
                    df = ar[c + 1] - yv[1];
                    if (ARD) df = df * w1;
                    sq[kk] = sq[kk] + df * df;
                }
            }
        }
    };
    double sk = 0.0;                                   // sum W o Kf
    [[maybe_unused]] double sl = 0.0;                  // isotropic route only: sum W o dk
    [[maybe_unused]] double sa = 0.0;                  // ARD route, RQ only: sum W o da
    [[maybe_unused]] double gs[ARD ? DC : 1];          // ARD route only: sum W o H o u_c^2 for the DC dimensions of chunk cz
#pragma unroll
    for (int c = 0; c < (ARD ? DC : 1); c++) gs[c] = 0.0;

    load_a(0);
    fetch(s0);
    put(0);
    __syncthreads();
    for (int st = s0; st < s1; st++) {
        const int cur = (st - s0) & 1;
        const bool more = st + 1 < s1;
        if (more) fetch(st + 1);
#pragma unroll
        for (int kk = 0; kk < NK; kk++) sq[kk] = 0.0;
        accumulate(ys[cur], 0);
        for (int ch = 1; ch < nch; ch++) {
            const d2 keep = rb;
            fetch_b(st * ITER_JT, ch * DC);
            __syncthreads();
            *(d2*)&yc[br][bc] = rb;
            if (ARD && ch == cz) *(d2*)&yz[br][bc] = rb;
            rb = keep;
            load_a(ch * DC);
            __syncthreads();
            accumulate(yc, ch * DC);
        }
        if (nch > 1) load_a(cz * DC);
        d4 wt[2];                                      // W[i0 + fr][j0 + 16 jt + fk + 4 r]
#pragma unroll
        for (int jt = 0; jt < 2; jt++) {
            wt[jt] = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int kk = 0; kk < TP / 4; kk++)
                wt[jt] = __builtin_amdgcn_mfma_f64_16x16x4f64(vs[cur][jt * 16 + fr][kk * 4 + fk], ub[kk], wt[jt], 0, 0, 0);
        }
        [[maybe_unused]] double e[ARD ? NK : 1];       // ARD route only: w H of the 8 entries, for the per-dimension sums
#pragma unroll
        for (int kk = 0; kk < NK; kk++) {
            const double w = wt[kk >> 2][kk & 3];
            if constexpr (ARD) {
                double kf, hh, da;
                ard_entry<KIND>(sq[kk], h.signal_var, sh, kf, hh, da);
                sk = sk + w * kf;
                if constexpr (NS > 0) sa = sa + w * da;
                e[kk] = w * hh;
            } else {
                double kf, dk;
                if constexpr (KIND == KERNEL_SE) {
                    kf = kernel_value<false, KERNEL_SE>(sq[kk], dl, h.signal_var);
                    dk = kf * div_by(sq[kk], dl);
                } else {
                    double hh;                         // matern_entry's third output: the ARD route's factor
                    matern_entry<KIND>(div_by(sq[kk], dl), h.signal_var, kf, dk, hh);
                }
                sk = sk + w * kf;
                sl = sl + w * dk;
            }
        }
        if constexpr (ARD) {
            double (*yb)[DC] = cz == 0 ? ys[cur] : yz;
#pragma unroll
            for (int cp = 0; cp < DC / 2; cp++) {
                const int c = 2 * cp, f = cz * DC + c;
                if (f < d) {
                    const double w0 = wts[f], w1 = f + 1 < d ? wts[f + 1] : 1.0;
#pragma unroll
                    for (int kk = 0; kk < NK; kk++) {
                        const d2 yv = *(const d2*)&yb[kk * 4 + fk][c];
                        double df = (ar[c] - yv[0]) * w0;
                        gs[c] = gs[c] + e[kk] * (df * df);
                        df = (ar[c + 1] - yv[1]) * w1;
                        gs[c + 1] = gs[c + 1] + e[kk] * (df * df);
                    }
                }
            }
            if (cz != 0) load_a(0);
        }
        if (more) put(cur ^ 1);
        __syncthreads();
    }
    // the workgroup's partial row: lanes by wave_sum, the four waves in a fixed order
    sk = wave_sum(sk);
    if constexpr (ARD) {
#pragma unroll
        for (int c = 0; c < DC; c++) gs[c] = wave_sum(gs[c]);
        if constexpr (NS > 0) sa = wave_sum(sa);
    } else {
        sl = wave_sum(sl);
    }
    if (lane == 0) {
        if constexpr (ARD) {
#pragma unroll
            for (int c = 0; c < DC; c++) red[c][wave] = gs[c];
            if constexpr (NS > 0) red[DC][wave] = sa;
            red[DC + NS][wave] = sk;
        } else {
            red[0][wave] = sl;
            red[1][wave] = sk;
        }
    }
    __syncthreads();
    const int nc = ARD ? d + NS + 1 : 2;
    double* __restrict__ o = part + ((size_t)blockIdx.x * gridDim.y + blockIdx.y) * nc;
    if (tid < (ARD ? DC + NS + 1 : 2)) {
        const double s = (red[tid][0] + red[tid][1]) + (red[tid][2] + red[tid][3]);
        if constexpr (ARD) {
            if (tid < DC) { if (cz * DC + tid < d) o[cz * DC + tid] = s; }
            else if (cz == 0) o[d + tid - DC] = s;
        } else {
            o[tid] = s;
        }
    }
}

// one column tile of U and V (t <= 16) and four (t <= 64), as k_cov_apply's two
template <bool ARD, int KIND>
__global__ __launch_bounds__(256) void k_cov_grad(const double* __restrict__ X, int n, int d, const HyperScalars* __restrict__ hd,
                                                  const double* __restrict__ U, const double* __restrict__ V,
                                                  double* __restrict__ part, int per)
{
    cov_grad_body<ARD, KIND, 1>(X, n, d, hd, U, V, part, per);
}
template <bool ARD, int KIND>
__global__ __launch_bounds__(256) void k_cov_grad4(const double* __restrict__ X, int n, int d, const HyperScalars* __restrict__ hd,
                                                   const double* __restrict__ U, const double* __restrict__ V,
                                                   double* __restrict__ part, int per)
{
    cov_grad_body<ARD, KIND, 4>(X, n, d, hd, U, V, part, per);
}

// out[c] = part[0][c] + part[1][c] + ... in row order, c < nc
__global__ __launch_bounds__(256) void k_cov_grad_finish(const double* __restrict__ part, size_t rows, int nc, double* __restrict__ out)
{
#pragma clang fp contract(off)
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= nc) return;
    double s = part[c];
    for (size_t k = 1; k < rows; k++) s = s + part[k * nc + c];
    out[c] = s;
}

void launch_cov_grad(const double* X, int n, int d, const CovFn& cf, const double* U, const double* V, int tp, double* part,
                     double* out, const IterPlan& pl, hipStream_t s)
{
    assert(cf.hd && (tp == 16 || tp == IT_MAXT));
    auto kern = tp == 16 ? CUGP_COV_KERNEL(cf, k_cov_grad) : CUGP_COV_KERNEL(cf, k_cov_grad4);
    const int nz = is_ard(cf) ? (d + DC - 1) / DC : 1, nc = cov_grad_columns(cf, d);
    assert(nz <= 65535);
    hipLaunchKernelGGL(kern, dim3(pl.row_blocks, pl.split, nz), dim3(256), 0, s, X, n, d, cf.hd, U, V, part, pl.per);
    hipLaunchKernelGGL(k_cov_grad_finish, dim3((nc + 255) / 256), dim3(256), 0, s, part, (size_t)pl.row_blocks * pl.split, nc, out);
}

// ---- the test-input gradients (iter_xgrad_device.h) ----
// k_cov_xgrad<ARD, KIND, VAR> under CUGP_COV_KERNEL's two-parameter table: the mean-only and the mean-and-variance forms
template <bool ARD, int KIND> constexpr auto k_cov_xgrad_mean = k_cov_xgrad<ARD, KIND, false>;
template <bool ARD, int KIND> constexpr auto k_cov_xgrad_var = k_cov_xgrad<ARD, KIND, true>;

void launch_cov_xgrad(const double* Xt, int nt, const double* X, int n, int d, const CovFn& cf, const double* wm, const double* Wv,
                      int tp, double* part, double* outm, double* outv, double fv, const IterPlan& pl, hipStream_t s)
{
    const bool var = Wv != nullptr;
    const int nz = (d + DC - 1) / DC, nq = var ? 2 : 1;
    assert(cf.hd && nz <= 65535 && (var ? pl.row_blocks == 1 && nt <= tp && (tp == 16 || tp == IT_MAXT) : wm && !outv));
    auto kern = var ? CUGP_COV_KERNEL(cf, k_cov_xgrad_var) : CUGP_COV_KERNEL(cf, k_cov_xgrad_mean);
    hipLaunchKernelGGL(kern, dim3(pl.row_blocks, pl.split, nz), dim3(256), 0, s, Xt, nt, X, n, d, cf.hd, wm, Wv, var ? tp : 16, part,
                       pl.per);
    const size_t cnt = (size_t)nt * d;
    hipLaunchKernelGGL(k_cov_xgrad_finish, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, s, part, pl.split, nq, cnt, d, cf.hd,
                       is_ard(cf) ? 1 : 0, fv, outm, outv);
}

void launch_iter_cross_rhs(const double* X, int n, int d, const double* Xt, int count, int tp, const CovFn& cf, double* R,
                           hipStream_t s)
{
    assert(cf.hd);
    const size_t cnt = (size_t)n * tp;
    hipLaunchKernelGGL(CUGP_COV_KERNEL(cf, k_iter_cross_rhs), dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, s, X, n, d, Xt,
                       count, tp, cf.hd, R);
}

void launch_iter_dot(const double* a, const double* b, int n, int tp, double* part, hipStream_t s)
{
    hipLaunchKernelGGL(k_iter_dot, dim3(iter_blocks(n)), dim3(256), 0, s, a, b, n, tp, part);
}
void launch_iter_sum(const double* part, int n, int tp, double* out, hipStream_t s)
{
    hipLaunchKernelGGL(k_iter_sum, dim3(1), dim3(256), 0, s, part, iter_blocks(n), tp, out);
}
void launch_iter_start(const double* b, double* x, double* r, double* p, int n, int tp, hipStream_t s)
{
    const size_t cnt = (size_t)n * tp;
    hipLaunchKernelGGL(k_iter_start, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, s, b, x, r, p, cnt);
}
void launch_iter_init(const double* part, int n, int tp, double tol, double* sc, hipStream_t s)
{
    hipLaunchKernelGGL(k_iter_init, dim3(1), dim3(256), 0, s, part, iter_blocks(n), tp, tol, sc);
}
void launch_iter_step_a(const double* part, int n, int tp, double* sc, hipStream_t s)
{
    hipLaunchKernelGGL(k_iter_step_a, dim3(1), dim3(256), 0, s, part, iter_blocks(n), tp, sc);
}
void launch_iter_update(double* x, double* r, const double* p, const double* q, int n, int tp, const double* sc, double* part,
                        hipStream_t s)
{
    hipLaunchKernelGGL(k_iter_update, dim3(iter_blocks(n)), dim3(256), 0, s, x, r, p, q, n, tp, sc, part);
}
void launch_iter_step_b(const double* part, int n, int tp, double* sc, hipStream_t s)
{
    hipLaunchKernelGGL(k_iter_step_b, dim3(1), dim3(256), 0, s, part, iter_blocks(n), tp, sc);
}
void launch_iter_dir(double* p, const double* r, int n, int tp, const double* sc, int restart_only, hipStream_t s)
{
    hipLaunchKernelGGL(k_iter_dir, dim3(iter_blocks(n)), dim3(256), 0, s, p, r, n, tp, sc, restart_only);
}
void launch_iter_resid(const double* b, const double* q, double* r, int n, int tp, const double* sc, int final, double* part,
                       hipStream_t s)
{
    hipLaunchKernelGGL(k_iter_resid, dim3(iter_blocks(n)), dim3(256), 0, s, b, q, r, n, tp, sc, final, part);
}
void launch_iter_step_v(const double* part, int n, int tp, int final, double* sc, hipStream_t s)
{
    hipLaunchKernelGGL(k_iter_step_v, dim3(1), dim3(256), 0, s, part, iter_blocks(n), tp, final, sc);
}
void launch_iter_poison(double* x, int n, int tp, const double* sc, hipStream_t s)
{
    hipLaunchKernelGGL(k_iter_poison, dim3(iter_blocks(n)), dim3(256), 0, s, x, n, tp, sc);
}

// ---- the preconditioner's products: M^-1 R = (R - Q (Q'R)) / sn2, Q [n][rp], rp a multiple of 64 ----
//
// k_pc_project<NCT>:  part[b] [rp][TP] = sum over the block's rows i of A[i][m] R[i][c], TP = 16 NCT.  The contraction runs
//   over the rows, so both MFMA operands are read as they lie in memory: A[row m = fr][k = fk] = A[i0 + fk][m0 + fr] and
//   B[k = fk][col fr] = R[i0 + fk][16 ct + fr] are 16 consecutive doubles per k -- 128-byte segments, no LDS.  The rp / 16 row
//   tiles of T are dealt to the four waves in turn (tile 4 q + wave, q < rp / 64 <= MQ); a wave holds MQ x NCT accumulators
//   (MQ = 1, 2, 4, 8: the smallest that holds rp; 128 registers at rp = 512, TP = 64, where one workgroup fits a CU) and
//   reads its R operands once per four rows for all its tiles.  Rows beyond
//   the block enter as zeros.  No two workgroups share an output: no atomics; k_pc_project_finish adds the blocks in
//   ascending order (first copied, then a = a + b).  With R = a 64-column group of A itself it is the Gram product L'L.
template <int NCT, int MQ>
__global__ __launch_bounds__(256) void k_pc_project(const double* __restrict__ A, int rp, const double* __restrict__ R, int ldr,
                                                    int n, int per, double* __restrict__ part)
{
    constexpr int TP = NCT * 16;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fk = lane >> 4;
    const int nq = rp / 64;
    const size_t r0 = (size_t)blockIdx.x * per, r1 = r0 + per < (size_t)n ? r0 + per : (size_t)n;
    d4 acc[MQ][NCT];
#pragma unroll
    for (int q = 0; q < MQ; q++)
#pragma unroll
        for (int ct = 0; ct < NCT; ct++) acc[q][ct] = (d4){0.0, 0.0, 0.0, 0.0};
    for (size_t i0 = r0; i0 < r1; i0 += 4) {
        const size_t i = i0 + fk;
        const bool in = i < r1;
        double b[NCT];
#pragma unroll
        for (int ct = 0; ct < NCT; ct++) b[ct] = in ? R[i * ldr + ct * 16 + fr] : 0.0;
        const double* __restrict__ ai = A + i * rp + wave * 16 + fr;
#pragma unroll
        for (int q = 0; q < MQ; q++)
            if (q < nq) {
                const double a = in ? ai[q * 64] : 0.0;
#pragma unroll
                for (int ct = 0; ct < NCT; ct++) acc[q][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b[ct], acc[q][ct], 0, 0, 0);
            }
    }
    double* __restrict__ o = part + (size_t)blockIdx.x * rp * TP;
#pragma unroll
    for (int q = 0; q < MQ; q++)
        if (q < nq)
#pragma unroll
            for (int ct = 0; ct < NCT; ct++)
#pragma unroll
                for (int r = 0; r < 4; r++) o[(size_t)(q * 64 + wave * 16 + fk + 4 * r) * TP + ct * 16 + fr] = acc[q][ct][r];
}

// out[e] = part[0][e] + part[1][e] + ... in block order, e < cnt = rp * tp
__global__ __launch_bounds__(256) void k_pc_project_finish(const double* __restrict__ part, int blocks, size_t cnt,
                                                           double* __restrict__ out)
{
#pragma clang fp contract(off)
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= cnt) return;
    double s = part[e];
    for (int k = 1; k < blocks; k++) s = s + part[(size_t)k * cnt + e];
    out[e] = s;
}

// the Gram product's finish: C[i][c0 + c] = the blocks' sum, + sn2 on the diagonal; i < rp, c < 64
__global__ __launch_bounds__(256) void k_pc_gram_finish(const double* __restrict__ part, int blocks, int rp,
                                                        const HyperScalars* __restrict__ hd, double* __restrict__ C, int ldc, int c0)
{
#pragma clang fp contract(off)
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x, cnt = (size_t)rp * 64;
    if (e >= cnt) return;
    const int i = (int)(e / 64), c = c0 + (int)(e % 64);
    double s = part[e];
    for (int k = 1; k < blocks; k++) s = s + part[(size_t)k * cnt + e];
    if (i == c) s = s + hd->noise_var;
    C[(size_t)i * ldc + c] = s;
}

// C = I over ld x ld: the padding of the r x r side's matrix
__global__ __launch_bounds__(256) void k_pc_eye(double* __restrict__ C, int ld)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e < (size_t)ld * ld) C[e] = e / ld == e % ld ? 1.0 : 0.0;
}

// k_pc_correct<NCT, FORM>:  out = (R - Q T) / sn2, or (FORM) out = Q T.  A workgroup owns 64 rows, a wave 16 of them and all
//   NCT column tiles.  Stage = PC_KC = 16 values of k: the 64 x 16 piece of Q (a thread reads one d4 of a row: the global reads
//   are row-contiguous) and the 16 x TP piece of T go through two LDS images each; the next stage's pieces are in flight in
//   registers behind the MFMAs and go into the other image: one barrier per stage.  qs rows are 18 doubles apart (144 B:
//   the 32 lanes of a ds_read_b64 fall on 32 different 8-byte bank pairs), ts rows TP + 16 at TP = 64 as k_cov_apply's vs.
//   A[row fr][k fk] = qs[16 wave + fr][4 kk + fk], B[k fk][col fr] = ts[4 kk + fk][16 ct + fr]; k runs ascending, 4 per MFMA;
//   the subtraction and the division (IEEE, one rounding each) happen once, in the epilogue.  FORM: T is the upper
//   triangular Lc^-T of the r x r side read at column c0 with its own row stride, entries below the diagonal taken as
//   zeros whatever the buffer holds there; out is the 64-column group at c0 of Q = L Lc^-T.
template <int NCT, bool FORM>
__global__ __launch_bounds__(256) void k_pc_correct(const double* __restrict__ Q, int rp, const double* __restrict__ T, int ldt,
                                                    int c0, const double* __restrict__ R, const HyperScalars* __restrict__ hd,
                                                    int n, double* __restrict__ out, int ldo)
{
#pragma clang fp contract(off)
    constexpr int TP = NCT * 16, TPL = (TP % 32 == 0) ? TP + 16 : TP, QL = PC_KC + 2, TV = PC_KC * TP / 4;
    __shared__ __attribute__((aligned(32))) double qs[2][64][QL];
    __shared__ __attribute__((aligned(32))) double ts[2][PC_KC][TPL];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fk = lane >> 4;
    const size_t i0 = (size_t)blockIdx.x * 64;
    const int nst = rp / PC_KC;
    const int qr = tid >> 2, qc = (tid & 3) * 4, tr = tid / (TP / 4), tc = (tid % (TP / 4)) * 4;
    d4 rq, rt;
    auto fetch = [&](int st) {
        rq = i0 + qr < (size_t)n ? *(const d4*)(Q + (i0 + qr) * rp + st * PC_KC + qc) : (d4){0.0, 0.0, 0.0, 0.0};
        if (tid < TV) {
            const int m = st * PC_KC + tr;
            rt = *(const d4*)(T + (size_t)m * ldt + c0 + tc);
            if constexpr (FORM) {
#pragma unroll
                for (int x = 0; x < 4; x++)
                    if (m > c0 + tc + x) rt[x] = 0.0;
            }
        }
    };
    auto put = [&](int buf) {
        qs[buf][qr][qc] = rq[0]; qs[buf][qr][qc + 1] = rq[1]; qs[buf][qr][qc + 2] = rq[2]; qs[buf][qr][qc + 3] = rq[3];
        if (tid < TV) *(d4*)&ts[buf][tr][tc] = rt;
    };
    d4 acc[NCT];
#pragma unroll
    for (int ct = 0; ct < NCT; ct++) acc[ct] = (d4){0.0, 0.0, 0.0, 0.0};
    fetch(0);
    put(0);
    __syncthreads();
    for (int st = 0; st < nst; st++) {
        const int cur = st & 1;
        const bool more = st + 1 < nst;
        if (more) fetch(st + 1);
#pragma unroll
        for (int kk = 0; kk < PC_KC / 4; kk++) {
            const double a = qs[cur][wave * 16 + fr][kk * 4 + fk];
#pragma unroll
            for (int ct = 0; ct < NCT; ct++)
                acc[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, ts[cur][kk * 4 + fk][ct * 16 + fr], acc[ct], 0, 0, 0);
        }
        if (more) put(cur ^ 1);
        __syncthreads();
    }
    double sn2 = 1.0;
    if constexpr (!FORM) sn2 = hd->noise_var;
#pragma unroll
    for (int ct = 0; ct < NCT; ct++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const size_t i = i0 + wave * 16 + fk + 4 * r;
            if (i < (size_t)n) {
                const int c = ct * 16 + fr;
                if constexpr (FORM) out[i * ldo + c0 + c] = acc[ct][r];
                else out[i * ldo + c] = (R[i * TP + c] - acc[ct][r]) / sn2;
            }
        }
}

// k_pc_sample<NCT>:  Z = L G1 + sn G2, the probes of the preconditioner's own distribution (rows of Z' ~ (0, M) for standard
//   G1, G2).  k_pc_correct's sibling: a workgroup owns ITER_ROWS = 64 rows, a wave 16 of them and all NCT
//   column tiles; a stage is PC_KC = 16 values of k, the 64 x 16 piece of L and the 16 x TP piece of G1 pass through two LDS
//   images each (the same pitches: 18 doubles, TP + 16 at TP = 64), the next stage's pieces in flight in registers behind the
//   MFMAs, one barrier per stage.  A[row fr][k fk] = ls[16 wave + fr][4 kk + fk], B[k fk][col fr] = gs[4 kk + fk][16 ct + fr].
//   Only the ceil(r / 16) stages that hold a row of G1 run; G1 has exactly r rows: a row m >= r of the last stage enters LDS
//   as zeros and is never read from memory (L's columns r .. rp - 1 are zeros of the build).  Order of the sum: k ascending, 4
//   per MFMA, into one fp64 accumulator from 0; then Z = acc + (sn G2), sn = sqrt(sn2) once per thread, the product and the
//   sum rounded once each.
template <int NCT>
__global__ __launch_bounds__(256) void k_pc_sample(const double* __restrict__ L, int rp, const double* __restrict__ G1, int r,
                                                   const double* __restrict__ G2, const HyperScalars* __restrict__ hd, int n,
                                                   double* __restrict__ Z)
{
#pragma clang fp contract(off)
    constexpr int TP = NCT * 16, TPL = (TP % 32 == 0) ? TP + 16 : TP, QL = PC_KC + 2, TV = PC_KC * TP / 4;
    __shared__ __attribute__((aligned(32))) double ls[2][ITER_ROWS][QL];
    __shared__ __attribute__((aligned(32))) double gs[2][PC_KC][TPL];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fk = lane >> 4;
    const size_t i0 = (size_t)blockIdx.x * ITER_ROWS;
    const int nst = (r + PC_KC - 1) / PC_KC;
    const int qr = tid >> 2, qc = (tid & 3) * 4, tr = tid / (TP / 4), tc = (tid % (TP / 4)) * 4;
    d4 rl, rg;
    auto fetch = [&](int st) {
        rl = i0 + qr < (size_t)n ? *(const d4*)(L + (i0 + qr) * rp + st * PC_KC + qc) : (d4){0.0, 0.0, 0.0, 0.0};
        if (tid < TV) {
            const int m = st * PC_KC + tr;
            rg = m < r ? *(const d4*)(G1 + (size_t)m * TP + tc) : (d4){0.0, 0.0, 0.0, 0.0};
        }
    };
    auto put = [&](int buf) {
        ls[buf][qr][qc] = rl[0]; ls[buf][qr][qc + 1] = rl[1]; ls[buf][qr][qc + 2] = rl[2]; ls[buf][qr][qc + 3] = rl[3];
        if (tid < TV) *(d4*)&gs[buf][tr][tc] = rg;
    };
    d4 acc[NCT];
#pragma unroll
    for (int ct = 0; ct < NCT; ct++) acc[ct] = (d4){0.0, 0.0, 0.0, 0.0};
    fetch(0);
    put(0);
    __syncthreads();
    for (int st = 0; st < nst; st++) {
        const int cur = st & 1;
        const bool more = st + 1 < nst;
        if (more) fetch(st + 1);
#pragma unroll
        for (int kk = 0; kk < PC_KC / 4; kk++) {
            const double a = ls[cur][wave * 16 + fr][kk * 4 + fk];
#pragma unroll
            for (int ct = 0; ct < NCT; ct++)
                acc[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, gs[cur][kk * 4 + fk][ct * 16 + fr], acc[ct], 0, 0, 0);
        }
        if (more) put(cur ^ 1);
        __syncthreads();
    }
    const double sn = __builtin_sqrt(hd->noise_var);
#pragma unroll
    for (int ct = 0; ct < NCT; ct++)
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const size_t i = i0 + wave * 16 + fk + 4 * q;
            if (i < (size_t)n) {
                const size_t e = i * TP + ct * 16 + fr;
                Z[e] = acc[ct][q] + sn * G2[e];
            }
        }
}

PcPlan pc_plan(int n, int rank)
{
    PcPlan p;
    p.rp = (rank + PC_RANK_PAD - 1) / PC_RANK_PAD * PC_RANK_PAD;
    const size_t want = std::min<size_t>(ITER_SLOTS, ((size_t)n + PC_MIN_ROWS - 1) / PC_MIN_ROWS);
    const size_t per = (((size_t)n + want - 1) / want + 15) / 16 * 16;
    p.per = (int)per;
    p.blocks = (int)(((size_t)n + per - 1) / per);      // no empty block
    return p;
}

void launch_pchol_init(const CovFn& cf, int d, int n, int rp, double* L, double* dres, int* piv, int* ctl, hipStream_t s)
{
    assert(cf.hd);
    const size_t cnt = (size_t)n * rp;
    hipLaunchKernelGGL(CUGP_COV_KERNEL(cf, k_pchol_init), dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, s, cf.hd, d, n, rp, L,
                       dres, piv, ctl);
}
void launch_pchol_step(const double* X, int n, int d, const CovFn& cf, double* L, int rp, double* dres, int* piv, int* ctl,
                       double* shv, int* shi, int k, int kmax, hipStream_t s)
{
    assert(cf.hd && kmax <= PCH_MAX_RANK && kmax <= rp);
    const int nwg = pchol_blocks(n), in = ((k + 1) & 1) * nwg, out = (k & 1) * nwg;
    hipLaunchKernelGGL(CUGP_COV_KERNEL(cf, k_pchol_step), dim3(nwg), dim3(PCH_ROWS), 0, s, X, n, d, cf.hd, L, rp, dres, piv, ctl,
                       shv + in, shi + in, shv + out, shi + out, nwg, k, kmax);
}
void launch_pc_project(const double* A, const double* R, int ldr, int tp, int n, const PcPlan& pl, double* part, hipStream_t s)
{
    assert((tp == 16 || tp == IT_MAXT) && pl.rp % 64 == 0 && pl.rp <= PCH_MAX_RANK);
    const int nq = pl.rp / 64, w = tp == 16 ? 0 : 1;
    auto kern = nq <= 1 ? (w ? k_pc_project<4, 1> : k_pc_project<1, 1>) : nq <= 2 ? (w ? k_pc_project<4, 2> : k_pc_project<1, 2>)
                : nq <= 4 ? (w ? k_pc_project<4, 4> : k_pc_project<1, 4>) : (w ? k_pc_project<4, 8> : k_pc_project<1, 8>);
    hipLaunchKernelGGL(kern, dim3(pl.blocks), dim3(256), 0, s, A, pl.rp, R, ldr, n, pl.per, part);
}
void launch_pc_project_finish(const double* part, int blocks, size_t cnt, double* out, hipStream_t s)
{
    hipLaunchKernelGGL(k_pc_project_finish, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, s, part, blocks, cnt, out);
}
void launch_pc_gram_finish(const double* part, int blocks, int rp, const HyperScalars* hd, double* C, int ldc, int c0, hipStream_t s)
{
    hipLaunchKernelGGL(k_pc_gram_finish, dim3((unsigned)(((size_t)rp * 64 + 255) / 256)), dim3(256), 0, s, part, blocks, rp, hd, C,
                       ldc, c0);
}
void launch_pc_eye(double* C, int ld, hipStream_t s)
{
    hipLaunchKernelGGL(k_pc_eye, dim3((unsigned)(((size_t)ld * ld + 255) / 256)), dim3(256), 0, s, C, ld);
}
void launch_pc_correct(const double* Q, int rp, const double* T, int ldt, int c0, const double* R, const HyperScalars* hd, int n,
                       int tp, double* out, int ldo, hipStream_t s)
{
    assert((tp == 16 || tp == IT_MAXT) && rp % 64 == 0 && (R || tp == IT_MAXT));
    const dim3 grid((unsigned)(((size_t)n + 63) / 64));
    if (!R) hipLaunchKernelGGL((k_pc_correct<4, true>), grid, dim3(256), 0, s, Q, rp, T, ldt, c0, R, hd, n, out, ldo);
    else if (tp == 16) hipLaunchKernelGGL((k_pc_correct<1, false>), grid, dim3(256), 0, s, Q, rp, T, ldt, c0, R, hd, n, out, ldo);
    else hipLaunchKernelGGL((k_pc_correct<4, false>), grid, dim3(256), 0, s, Q, rp, T, ldt, c0, R, hd, n, out, ldo);
}
void launch_iter_step_a_pc(const double* part, int n, int tp, double* sc, hipStream_t s)
{
    hipLaunchKernelGGL(k_iter_step_a_pc, dim3(1), dim3(256), 0, s, part, iter_blocks(n), tp, sc);
}
void launch_iter_step_z(const double* part, int n, int tp, int first, double* sc, hipStream_t s)
{
    hipLaunchKernelGGL(k_iter_step_z, dim3(1), dim3(256), 0, s, part, iter_blocks(n), tp, first, sc);
}
// the Lanczos quadrature's kernels (iter_device.h) and the probes' product
void launch_iter_record(const double* sc, int tp, int start, int wrow, int cap, double* rec, double* meta, hipStream_t s)
{
    hipLaunchKernelGGL(k_iter_record, dim3(1), dim3(256), 0, s, sc, tp, start, wrow, cap, rec, meta);
}
void launch_slq_quad(const double* rec, const double* meta, int cnt, int cap, double* work, double* quad, hipStream_t s)
{
    assert(cnt >= 1 && cnt <= IT_MAXT);
    hipLaunchKernelGGL(k_slq_quad, dim3(1), dim3(256), 0, s, rec, meta, cnt, cap, work, quad);
}
void launch_slq_finish(const double* part, int n, const double* quad, int t, const double* U, int ldu, int r, double* out,
                       hipStream_t s)
{
    hipLaunchKernelGGL(k_slq_finish, dim3(1), dim3(64), 0, s, part, iter_blocks(n), quad, t, U, ldu, r, out);
}
void launch_pc_sample(const double* L, int rp, const double* G1, int r, const double* G2, const HyperScalars* hd, int n, int tp,
                      double* Z, hipStream_t s)
{
    assert((tp == 16 || tp == IT_MAXT) && rp % 64 == 0 && r >= 1 && r <= rp);
    const dim3 grid((unsigned)(((size_t)n + ITER_ROWS - 1) / ITER_ROWS));
    if (tp == 16) hipLaunchKernelGGL(k_pc_sample<1>, grid, dim3(256), 0, s, L, rp, G1, r, G2, hd, n, Z);
    else hipLaunchKernelGGL(k_pc_sample<4>, grid, dim3(256), 0, s, L, rp, G1, r, G2, hd, n, Z);
}
// the mixed mode's cycle kernels (iter_device.h; the fp32 product and its launcher: iter32_gfx950.h)
void launch_iter_goal_init(int tp, double rho2, double* sc, hipStream_t s)
{
    hipLaunchKernelGGL(k_iter_goal_init, dim3(1), dim3(256), 0, s, tp, rho2, sc);
}
void launch_iter_step_b_mx(const double* part, int n, int tp, double* sc, hipStream_t s)
{
    hipLaunchKernelGGL(k_iter_step_b_mx, dim3(1), dim3(256), 0, s, part, iter_blocks(n), tp, sc);
}
void launch_iter_step_v_mx(const double* part, int n, int tp, int final, double rho2, double* sc, hipStream_t s)
{
    hipLaunchKernelGGL(k_iter_step_v_mx, dim3(1), dim3(256), 0, s, part, iter_blocks(n), tp, final, rho2, sc);
}
void launch_iter_again(const double* b, double* x, double* r, int n, int tp, double* sc, hipStream_t s)
{
    hipLaunchKernelGGL(k_iter_again, dim3(iter_blocks(n)), dim3(256), 0, s, b, x, r, n, tp, sc);
    hipLaunchKernelGGL(k_iter_again_sc, dim3(1), dim3(256), 0, s, tp, sc);
}
