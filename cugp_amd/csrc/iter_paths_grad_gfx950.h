// iter_paths_grad_gfx950.h -- the input gradients of the matrix-free GP's posterior sample paths (cugp_iter_paths_grad;
// DESIGN.md section 39): for s <= 64 paths at once, at nt points,
//     df_c / dx_a (x_i) = -amp sum_k sin(p_ik) omega~_ka W[k][c]  -  s_a sum_j G_ij (x_ia - x_ja) V[j][c],
// p_ik k_rff_apply's phase, omega~ its scaled frequency, G xgrad_factor (iter_xgrad_device.h), s_a = w_a^2 | 1 / l^2.
//
// Include-point contract.  Included INSIDE namespace cugp by kernels.hip, after iter_rff_gfx950.h (rff_apply_plan) and
// everything that header asks for: iter_gfx950.h (iter_apply_plan), iter_xgrad_device.h (xgrad_factor), cov_device.h.
//
// Both sums have one shape: an entry computed in registers (G_ij | sin(p_ik)) times a per-dimension factor ((x_ia - x_ja) |
// omega~_ka), summed against a tile of columns that ALL points share.  k_cov_xgrad has no matrix instruction because its
// weights are per point; with shared columns the MFMA fits and the difference is still formed first:
//   lane (fr = lane & 15, fk = lane >> 4) computes the ONE entry for (row i0 + fr, stage row 4 kk + fk) -- the squared distance in
//   k_cov_apply's arithmetic (differences before squares, feature order, no contraction) | the phase in k_rff_apply's (b_k first,
//   products added in feature order, the origin subtracted first) -- and for each dimension a of its chunk forms
//       e_a = fl(G_ij fl(x_ia - x_ja))     (the difference first, unweighted)     |     e_a = fl(sin(p_ik) omega~_ka)
//   which v_mfma_f64_16x16x4_f64 takes as A[row fr][k fk]; B is V[j][16 ct + fr] | W[k][16 ct + fr] out of the LDS image of the
//   stage's rows (k_cov_apply4's layout: TPL = 80 doubles a row at tp = 64).  One entry feeds PG_FC x NCT MFMAs, accumulators
//   acc[PG_FC][NCT] (C/D: rows fk + 4 r, column fr).
// Register budget.  d x NCT accumulators of 4 doubles do not fit (d = 10, NCT = 4: 320 registers): the dimensions are split
//   into chunks of PG_FC = 4 over blockIdx.z and every chunk recomputes the entry, as k_cov_xgrad and k_cov_grad do.
//   acc takes 8 PG_FC NCT = 128 registers at NCT = 4.  A chunk lies inside one DC = 16 chunk of the distance | phase: chunk
//   z reads its x_j | omega~ values from the stage's own LDS image (DC chunk 0) or from yz | oz, the copy the chunk loop leaves
//   of DC chunk (z PG_FC) / DC (d > 16: served, not tuned); the lane's PG_FC coordinates x_ia are loaded once for the sweep.
// Decomposition: k_cov_apply's.  Workgroup = 4 waves x 16 rows (ITER_ROWS), stage = ITER_JT = 32 training rows | features,
//   double-buffered through LDS, the next stage in registers behind the MFMAs, one barrier per stage; grid (row blocks,
//   split, dimension chunks), the split from iter_apply_plan | rff_apply_plan.  Every workgroup writes its partial block
//   part[split s][i][a][c] (c fastest: 128-byte runs); k_paths_grad_finish adds the ranges in ascending s, applies -s_a and
//   -amp once per output, adds the two terms by one addition (the feature term first) and writes out[c][i][a], the
//   caller's layout.  Rows beyond n | m are staged as zeros (G 0 = 0, sin(0) 0 = 0); dimensions beyond d are not multiplied.
//   No atomics; a column's sums do not depend on the other columns, a row's not on nt or on its neighbours.
// LDS: ys [2][32][16], yc, yz [32][16], vs [2][32][TPL]: 24 KiB | 56 KiB;  os, oc, oz, bs [2][32], ws: 24.5 KiB | 56.5 KiB.
#pragma once

constexpr int PG_FC = 4;             // dimensions of a workgroup (blockIdx.z): PG_FC x NCT accumulator tiles per lane
static_assert(DC % PG_FC == 0, "a dimension chunk lies inside one feature chunk of the distance");

template <bool ARD, int KIND, int NCT>
__device__ __forceinline__ void cov_xgrad_cols_body(const double* __restrict__ Xt, int nt, const double* __restrict__ X, int n, int d,
                                                    const HyperScalars* __restrict__ hd, const double* __restrict__ V,
                                                    double* __restrict__ part, int per)
{
#pragma clang fp contract(off)
    constexpr int TP = NCT * 16, TPL = (TP % 32 == 0) ? TP + 16 : TP, NK = ITER_JT / 4;
    static_assert(ITER_JT * DC == 2 * 256 && ITER_JT * TP == 2 * 256 * NCT, "one d2 of x and NCT d2 of V per thread and stage");
    __shared__ __attribute__((aligned(32))) double ys[2][ITER_JT][DC];
    __shared__ __attribute__((aligned(16))) double yc[ITER_JT][DC];
    __shared__ __attribute__((aligned(32))) double yz[ITER_JT][DC];
    __shared__ __attribute__((aligned(16))) double vs[2][ITER_JT][TPL];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fk = lane >> 4;
    const int row = blockIdx.x * ITER_ROWS + wave * 16 + fr;
    const HyperScalars h = *hd;
    const double* __restrict__ wts = ard_weights(hd);
    const DivBy dl = div_prepare(h.ell_sq);
    const ShapeArgs sh = shape_args<KIND>(wts, d);
    const int nst = (n + ITER_JT - 1) / ITER_JT, nch = (d + DC - 1) / DC;
    const int s0 = blockIdx.y * per, s1 = s0 + per < nst ? s0 + per : nst;
    const int a0 = blockIdx.z * PG_FC, cz = a0 / DC, az0 = a0 % DC;     // the chunk's dimensions [a0, a0 + PG_FC): in DC chunk cz
    const int na = d - a0 < PG_FC ? d - a0 : PG_FC;

    d4 acc[PG_FC][NCT];
#pragma unroll
    for (int a = 0; a < PG_FC; a++)
#pragma unroll
        for (int ct = 0; ct < NCT; ct++) acc[a][ct] = (d4){0.0, 0.0, 0.0, 0.0};
    double ar[DC], xa[PG_FC];
    auto load_a = [&](int c0) {
#pragma unroll
        for (int c = 0; c < DC; c++) ar[c] = (row < nt && c0 + c < d) ? Xt[(size_t)row * d + c0 + c] : 0.0;
    };
#pragma unroll
    for (int a = 0; a < PG_FC; a++) xa[a] = (row < nt && a < na) ? Xt[(size_t)row * d + a0 + a] : 0.0;
    // the thread's share of a stage: one feature pair of one x row, NCT column pairs of V rows
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
            if (ch == cz) *(d2*)&yz[br][bc] = rb;
            rb = keep;
            load_a(ch * DC);
            __syncthreads();
            accumulate(yc, ch * DC);
        }
        if (nch > 1) load_a(0);
        const double (*yb)[DC] = cz == 0 ? ys[cur] : yz;
#pragma unroll
        for (int kk = 0; kk < NK; kk++) {
            const double g = xgrad_factor<ARD, KIND>(sq[kk], dl, h.signal_var, sh);
            const d4 xj = *(const d4*)&yb[kk * 4 + fk][az0];
#pragma unroll
            for (int a = 0; a < PG_FC; a++)
                if (a < na) {
                    const double e = g * (xa[a] - xj[a]);
#pragma unroll
                    for (int ct = 0; ct < NCT; ct++)
                        acc[a][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(e, vs[cur][kk * 4 + fk][ct * 16 + fr], acc[a][ct], 0, 0, 0);
                }
        }
        if (more) put(cur ^ 1);
        __syncthreads();
    }
    double* __restrict__ o = part + (size_t)blockIdx.y * nt * d * TP;
#pragma unroll
    for (int a = 0; a < PG_FC; a++)
        if (a < na)
#pragma unroll
            for (int ct = 0; ct < NCT; ct++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int i = blockIdx.x * ITER_ROWS + wave * 16 + fk + 4 * r;
                    if (i < nt) o[((size_t)i * d + a0 + a) * TP + ct * 16 + fr] = acc[a][ct][r];
                }
}

// one column tile (s <= 16) and four (s <= 64) per covariance family, under CUGP_COV_KERNEL's two-parameter table
template <bool ARD, int KIND>
__global__ __launch_bounds__(256) void k_cov_xgrad_cols(const double* __restrict__ Xt, int nt, const double* __restrict__ X, int n,
                                                        int d, const HyperScalars* __restrict__ hd, const double* __restrict__ V,
                                                        double* __restrict__ part, int per)
{
    cov_xgrad_cols_body<ARD, KIND, 1>(Xt, nt, X, n, d, hd, V, part, per);
}
template <bool ARD, int KIND>
__global__ __launch_bounds__(256) void k_cov_xgrad_cols4(const double* __restrict__ Xt, int nt, const double* __restrict__ X, int n,
                                                         int d, const HyperScalars* __restrict__ hd, const double* __restrict__ V,
                                                         double* __restrict__ part, int per)
{
    cov_xgrad_cols_body<ARD, KIND, 4>(Xt, nt, X, n, d, hd, V, part, per);
}

// The feature term: k_rff_apply's staging and phase chain, line for line; where that kernel takes a cosine this one takes one
// sine (the device library's fp64 sin: its own argument reduction) and multiplies it with the PG_FC scaled frequencies of
// its dimension chunk, which already lie in the stage's LDS image.
template <bool ARD, int NCT>
__device__ __forceinline__ void rff_grad_body(const double* __restrict__ Xq, int nq, int d, const HyperScalars* __restrict__ hd,
                                              const double* __restrict__ Om, const double* __restrict__ ph, int m,
                                              const double* __restrict__ org, const double* __restrict__ W,
                                              double* __restrict__ part, int per)
{
#pragma clang fp contract(off)
    constexpr int TP = NCT * 16, TPL = (TP % 32 == 0) ? TP + 16 : TP, NK = ITER_JT / 4;
    static_assert(ITER_JT * DC == 2 * 256 && ITER_JT * TP == 2 * 256 * NCT, "one d2 of omega and NCT d2 of W per thread and stage");
    __shared__ __attribute__((aligned(32))) double os[2][ITER_JT][DC];
    __shared__ __attribute__((aligned(16))) double oc[ITER_JT][DC];
    __shared__ __attribute__((aligned(32))) double oz[ITER_JT][DC];
    __shared__ double bs[2][ITER_JT];
    __shared__ __attribute__((aligned(16))) double ws[2][ITER_JT][TPL];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fk = lane >> 4;
    const int row = blockIdx.x * ITER_ROWS + wave * 16 + fr;
    const double* __restrict__ wts = ard_weights(hd);
    const double il = ARD ? 1.0 : 1.0 / __builtin_sqrt(hd->ell_sq);
    const int nst = (m + ITER_JT - 1) / ITER_JT, nch = (d + DC - 1) / DC;
    const int s0 = blockIdx.y * per, s1 = s0 + per < nst ? s0 + per : nst;
    const int a0 = blockIdx.z * PG_FC, cz = a0 / DC, az0 = a0 % DC;
    const int na = d - a0 < PG_FC ? d - a0 : PG_FC;

    d4 acc[PG_FC][NCT];
#pragma unroll
    for (int a = 0; a < PG_FC; a++)
#pragma unroll
        for (int ct = 0; ct < NCT; ct++) acc[a][ct] = (d4){0.0, 0.0, 0.0, 0.0};
    double ar[DC];
    auto load_a = [&](int c0) {
#pragma unroll
        for (int c = 0; c < DC; c++) ar[c] = (row < nq && c0 + c < d) ? Xq[(size_t)row * d + c0 + c] - org[c0 + c] : 0.0;
    };
    // the thread's share of a stage: one scaled feature pair of one omega row, NCT column pairs of W rows; the first 32
    // threads: a phase each
    const int br = tid >> 3, bc = (tid & 7) * 2;
    d2 rb, rv[NCT];
    double rp = 0.0;
    auto fetch_o = [&](int k0, int c0) {
        const int k = k0 + br, c = c0 + bc;
        rb[0] = (k < m && c < d) ? Om[(size_t)k * d + c] * (ARD ? wts[c] : il) : 0.0;
        rb[1] = (k < m && c + 1 < d) ? Om[(size_t)k * d + c + 1] * (ARD ? wts[c + 1] : il) : 0.0;
    };
    auto fetch = [&](int st) {
        const int k0 = st * ITER_JT;
        fetch_o(k0, 0);
        if (tid < ITER_JT) rp = k0 + tid < m ? ph[k0 + tid] : 0.0;
#pragma unroll
        for (int q = 0; q < NCT; q++) {
            const int e = tid + 256 * q, k = k0 + e / (TP / 2);
            rv[q] = k < m ? *(const d2*)(W + (size_t)k * TP + 2 * (e % (TP / 2))) : (d2){0.0, 0.0};
        }
    };
    auto put = [&](int buf) {
        *(d2*)&os[buf][br][bc] = rb;
        if (tid < ITER_JT) bs[buf][tid] = rp;
#pragma unroll
        for (int q = 0; q < NCT; q++) {
            const int e = tid + 256 * q;
            *(d2*)&ws[buf][e / (TP / 2)][2 * (e % (TP / 2))] = rv[q];
        }
    };
    double pv[NK];
    // pv[kk] += the chunk's terms (x_row - c)_f omega~_{4 kk + fk, f}, features ascending: k_rff_apply's lines
    auto accumulate = [&](double (*ob)[DC], int c0) {
#pragma unroll
        for (int cp = 0; cp < DC / 2; cp++) {
            const int c = 2 * cp;
            if (c0 + c < d) {
#pragma unroll
                for (int kk = 0; kk < NK; kk++) {
                    const d2 ov = *(const d2*)&ob[kk * 4 + fk][c];
                    pv[kk] = pv[kk] + ar[c] * ov[0];
                    pv[kk] = pv[kk] + ar[c + 1] * ov[1];     // (a feature beyond d: + 0 0)
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
        for (int kk = 0; kk < NK; kk++) pv[kk] = bs[cur][kk * 4 + fk];
        accumulate(os[cur], 0);
        for (int ch = 1; ch < nch; ch++) {
            const d2 keep = rb;
            fetch_o(st * ITER_JT, ch * DC);
            __syncthreads();
            *(d2*)&oc[br][bc] = rb;
            if (ch == cz) *(d2*)&oz[br][bc] = rb;
            rb = keep;
            load_a(ch * DC);
            __syncthreads();
            accumulate(oc, ch * DC);
        }
        if (nch > 1) load_a(0);
        const double (*ob)[DC] = cz == 0 ? os[cur] : oz;
#pragma unroll
        for (int kk = 0; kk < NK; kk++) {
            const double sv = sin(pv[kk]);
            const d4 ok = *(const d4*)&ob[kk * 4 + fk][az0];
#pragma unroll
            for (int a = 0; a < PG_FC; a++)
                if (a < na) {
                    const double e = sv * ok[a];
#pragma unroll
                    for (int ct = 0; ct < NCT; ct++)
                        acc[a][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(e, ws[cur][kk * 4 + fk][ct * 16 + fr], acc[a][ct], 0, 0, 0);
                }
        }
        if (more) put(cur ^ 1);
        __syncthreads();
    }
    double* __restrict__ o = part + (size_t)blockIdx.y * nq * d * TP;
#pragma unroll
    for (int a = 0; a < PG_FC; a++)
        if (a < na)
#pragma unroll
            for (int ct = 0; ct < NCT; ct++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int i = blockIdx.x * ITER_ROWS + wave * 16 + fk + 4 * r;
                    if (i < nq) o[((size_t)i * d + a0 + a) * TP + ct * 16 + fr] = acc[a][ct][r];
                }
}

template <bool ARD>
__global__ __launch_bounds__(256) void k_rff_grad(const double* __restrict__ Xq, int nq, int d, const HyperScalars* __restrict__ hd,
                                                  const double* __restrict__ Om, const double* __restrict__ ph, int m,
                                                  const double* __restrict__ org, const double* __restrict__ W,
                                                  double* __restrict__ part, int per)
{
    rff_grad_body<ARD, 1>(Xq, nq, d, hd, Om, ph, m, org, W, part, per);
}
template <bool ARD>
__global__ __launch_bounds__(256) void k_rff_grad4(const double* __restrict__ Xq, int nq, int d, const HyperScalars* __restrict__ hd,
                                                   const double* __restrict__ Om, const double* __restrict__ ph, int m,
                                                   const double* __restrict__ org, const double* __restrict__ W,
                                                   double* __restrict__ part, int per)
{
    rff_grad_body<ARD, 4>(Xq, nq, d, hd, Om, ph, m, org, W, part, per);
}

// out[c][i][a] = -amp (F_0 + F_1 + ...) + -s_a (D_0 + D_1 + ...): the ranges' partial blocks pf [sf][nt][d][tp] and pd [sd][nt][d][tp]
// in ascending order (first copied, then a = a + b), each term scaled once, one addition, the feature term first; a null
// block: the other term alone.  s_a = w_a^2 on the ARD route (a tied rational quadratic handle: its equal weights), else 1 / l^2.
// One thread per (i, a, c) of the partial blocks' layout: the reads are contiguous.
__global__ __launch_bounds__(256) void k_paths_grad_finish(const double* __restrict__ pf, int sf, const double* __restrict__ pd, int sd,
                                                           int nt, int d, int tp, const HyperScalars* __restrict__ hd, int route,
                                                           double amp, double* __restrict__ out)
{
#pragma clang fp contract(off)
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x, cnt = (size_t)nt * d * tp;
    if (e >= cnt) return;
    const int c = (int)(e % tp), a = (int)(e / tp % d);
    const size_t i = e / tp / d;
    double f = 0.0, g = 0.0;
    if (pf) {
        double s = pf[e];
        for (int k = 1; k < sf; k++) s = s + pf[(size_t)k * cnt + e];
        f = -(amp * s);
    }
    if (pd) {
        const double* __restrict__ wts = ard_weights(hd);
        const double sc = route ? wts[a] * wts[a] : 1.0 / hd->ell_sq;
        double s = pd[e];
        for (int k = 1; k < sd; k++) s = s + pd[(size_t)k * cnt + e];
        g = -(sc * s);
    }
    out[((size_t)c * nt + i) * d + a] = pf && pd ? f + g : (pf ? f : g);
}

void launch_paths_grad(const double* Xt, int nt, int d, const CovFn& cf, const double* X, int n, const double* V, const IterPlan& pd,
                       double* partd, const double* Om, const double* ph, int m, const double* org, const double* W, double amp,
                       const IterPlan& pf, double* partf, int tp, double* out, hipStream_t s)
{
    const int nz = (d + PG_FC - 1) / PG_FC;
    assert(cf.hd && (tp == 16 || tp == IT_MAXT) && nz <= 65535 && (V || W) && (!V || partd) && (!W || (partf && org)));
    if (W) {
        auto kern = tp == 16 ? (is_ard(cf) ? k_rff_grad<true> : k_rff_grad<false>) : (is_ard(cf) ? k_rff_grad4<true> : k_rff_grad4<false>);
        hipLaunchKernelGGL(kern, dim3(pf.row_blocks, pf.split, nz), dim3(256), 0, s, Xt, nt, d, cf.hd, Om, ph, m, org, W, partf, pf.per);
    }
    if (V) {
        auto kern = tp == 16 ? CUGP_COV_KERNEL(cf, k_cov_xgrad_cols) : CUGP_COV_KERNEL(cf, k_cov_xgrad_cols4);
        hipLaunchKernelGGL(kern, dim3(pd.row_blocks, pd.split, nz), dim3(256), 0, s, Xt, nt, X, n, d, cf.hd, V, partd, pd.per);
    }
    const size_t cnt = (size_t)nt * d * tp;
    hipLaunchKernelGGL(k_paths_grad_finish, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, s, W ? partf : nullptr, pf.split,
                       V ? partd : nullptr, pd.split, nt, d, tp, cf.hd, is_ard(cf) ? 1 : 0, amp, out);
}
