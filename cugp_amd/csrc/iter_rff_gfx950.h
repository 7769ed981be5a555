// iter_rff_gfx950.h -- the random-feature product of the matrix-free GP's pathwise posterior draws (cugp_iter_features_apply,
// cugp_iter_paths_fit, cugp_iter_paths_eval), its plan and its launcher.
//
// Include-point contract.  Included INSIDE namespace cugp by kernels.hip, after iter_gfx950.h (k_cov_apply_finish, whose
// second launch adds the partial blocks of a split feature range) and everything that header asks for.
//
// k_rff_apply<ARD>:  out[i][c] = amp sum_k cos(phase(i, k)) W[k][c],  phase(i, k) = b_k + sum_f (x_if - c_f) (omega_kf s_f),
//   s_f = w_f (ARD: the handle's weights exp(-theta_f), an RQ handle's tied ones included) | 1 / sqrt(ell_sq) (isotropic).
//   Phi is never stored.  k_cov_apply's decomposition with the frequencies in the place of the b rows: lane (fr = lane & 15,
//   fk = lane >> 4) computes the ONE entry cos(phase(i0 + fr, k + fk)) and hands it to v_mfma_f64_16x16x4_f64 as A[row fr][k fk];
//   B is W[k + fk][16 ct + fr] out of the LDS image of the stage's W rows; the entry feeds NCT MFMAs.  C/D: rows fk + 4 r, column fr.
//   Workgroup: 4 waves x 16 rows = ITER_ROWS output rows; the lane's row x_i - c (the origin subtracted first, one rounding)
//   sits in registers, DC features at a time.  Stage = ITER_JT = 32 features: their omega rows (first feature chunk) SCALED as
//   they are staged -- one product per stage and (k, f), not one per entry --, their phases b_k and their W rows.  Per stage a
//   lane forms 8 phases: b_k first, then the products (x_if - c_f) omega~_kf added in feature order, no contraction: one
//   rounding sequence, whatever s, tp and the neighbours are.  Then 8 cos (the device library's fp64 cos: its own argument
//   reduction holds for every finite phase), then 8 NCT MFMAs.  The next stage travels in registers meanwhile and goes into
//   the other LDS buffer behind the MFMAs: one barrier per stage.  Feature chunks beyond the first go through a third buffer
//   inside the stage, the phase carried across chunks (two barriers per chunk: d > 16 only, served, not tuned).
//   Features beyond m are staged as zero omega, zero b and zero W rows: cos(0) 0 = 0.  W rows are padded as k_cov_apply4's V rows.
//   LDS: os [2][32][16], oc [32][16], bs [2][32], ws [2][32][TPL] doubles, TPL = 16 | 80: 20.5 KiB | 52.5 KiB.
//   grid (row blocks, split): workgroup (., s) sums the stages [s per, (s + 1) per), k ascending, 4 per MFMA; amp = sqrt(2 sf2 / m)
//   (formed on the host) multiplies the workgroup's sum once, in the epilogue.  split > 1: the workgroup writes its scaled
//   partial block part[s][nq][tp] and k_cov_apply_finish (square = 0) adds the blocks in ascending s.  No atomics; a column's
//   sums do not depend on the other columns: column c of a 17-column call carries the bits of its 1-column call.
#pragma once

constexpr int RFF_MIN_STAGES = 2;    // stages (64 features) per range at least: an entry costs a cos, and nq is often a few hundred

template <bool ARD, int NCT>
__device__ __forceinline__ void rff_apply_body(const double* __restrict__ Xq, int nq, int d, const HyperScalars* __restrict__ hd,
                                               const double* __restrict__ Om, const double* __restrict__ ph, int m,
                                               const double* __restrict__ org, const double* __restrict__ W, double amp,
                                               double* __restrict__ out, int per)
{
#pragma clang fp contract(off)
    constexpr int TP = NCT * 16, TPL = (TP % 32 == 0) ? TP + 16 : TP, NK = ITER_JT / 4;
    static_assert(ITER_JT * DC == 2 * 256 && ITER_JT * TP == 2 * 256 * NCT, "one d2 of omega and NCT d2 of W per thread and stage");
    __shared__ __attribute__((aligned(16))) double os[2][ITER_JT][DC];
    __shared__ __attribute__((aligned(16))) double oc[ITER_JT][DC];
    __shared__ double bs[2][ITER_JT];
    __shared__ __attribute__((aligned(16))) double ws[2][ITER_JT][TPL];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fk = lane >> 4;
    const int row = blockIdx.x * ITER_ROWS + wave * 16 + fr;
    const double* __restrict__ wts = ard_weights(hd);
    const double il = ARD ? 1.0 : 1.0 / __builtin_sqrt(hd->ell_sq);
    const int nst = (m + ITER_JT - 1) / ITER_JT, nch = (d + DC - 1) / DC;
    const int s0 = blockIdx.y * per, s1 = s0 + per < nst ? s0 + per : nst;

    d4 acc[NCT];
#pragma unroll
    for (int ct = 0; ct < NCT; ct++) acc[ct] = (d4){0.0, 0.0, 0.0, 0.0};
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
    // pv[kk] += the chunk's terms (x_row - c)_f omega~_{4 kk + fk, f}, features ascending
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
            rb = keep;
            load_a(ch * DC);
            __syncthreads();
            accumulate(oc, ch * DC);
        }
        if (nch > 1) load_a(0);
#pragma unroll
        for (int kk = 0; kk < NK; kk++) {
            const double cv = cos(pv[kk]);
#pragma unroll
            for (int ct = 0; ct < NCT; ct++)
                acc[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(cv, ws[cur][kk * 4 + fk][ct * 16 + fr], acc[ct], 0, 0, 0);
        }
        if (more) put(cur ^ 1);
        __syncthreads();
    }
    double* __restrict__ o = out + (size_t)blockIdx.y * nq * TP;
#pragma unroll
    for (int ct = 0; ct < NCT; ct++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int i = blockIdx.x * ITER_ROWS + wave * 16 + fk + 4 * r;
            if (i < nq) o[(size_t)i * TP + ct * 16 + fr] = amp * acc[ct][r];
        }
}

// one column tile (s <= 16) and four (s <= 64); the family enters through the caller's frequencies and the handle's scales
// alone: four instantiations
template <bool ARD>
__global__ __launch_bounds__(256) void k_rff_apply(const double* __restrict__ Xq, int nq, int d, const HyperScalars* __restrict__ hd,
                                                   const double* __restrict__ Om, const double* __restrict__ ph, int m,
                                                   const double* __restrict__ org, const double* __restrict__ W, double amp,
                                                   double* __restrict__ out, int per)
{
    rff_apply_body<ARD, 1>(Xq, nq, d, hd, Om, ph, m, org, W, amp, out, per);
}
template <bool ARD>
__global__ __launch_bounds__(256) void k_rff_apply4(const double* __restrict__ Xq, int nq, int d, const HyperScalars* __restrict__ hd,
                                                    const double* __restrict__ Om, const double* __restrict__ ph, int m,
                                                    const double* __restrict__ org, const double* __restrict__ W, double amp,
                                                    double* __restrict__ out, int per)
{
    rff_apply_body<ARD, 4>(Xq, nq, d, hd, Om, ph, m, org, W, amp, out, per);
}

// iter_apply_plan's rule over (na = nq rows, nb = m features) with RFF_MIN_STAGES in the place of ITER_MIN_STAGES
IterPlan rff_apply_plan(int nq, int m, int force)
{
    IterPlan p;
    p.row_blocks = (int)(((size_t)nq + ITER_ROWS - 1) / ITER_ROWS);
    p.stages = (int)(((size_t)m + ITER_JT - 1) / ITER_JT);
    int want = force;
    if (want <= 0) {
        want = p.row_blocks >= ITER_SLOTS ? 1 : (ITER_SLOTS + p.row_blocks - 1) / p.row_blocks;
        want = std::min(want, std::min(ITER_MAX_SPLIT, p.stages / RFF_MIN_STAGES));
    }
    want = std::max(1, std::min(want, std::min(p.stages, 65535)));
    p.per = (p.stages + want - 1) / want;
    p.split = (p.stages + p.per - 1) / p.per;          // no empty range
    return p;
}

void launch_rff_apply(const double* Xq, int nq, int d, const CovFn& cf, const double* Om, const double* ph, int m, const double* org,
                      const double* W, int tp, double amp, double* out, double* part, const IterPlan& pl, hipStream_t s)
{
    assert(cf.hd && org && (tp == 16 || tp == IT_MAXT) && (pl.split == 1 || part));
    auto kern = tp == 16 ? (is_ard(cf) ? k_rff_apply<true> : k_rff_apply<false>) : (is_ard(cf) ? k_rff_apply4<true> : k_rff_apply4<false>);
    hipLaunchKernelGGL(kern, dim3(pl.row_blocks, pl.split), dim3(256), 0, s, Xq, nq, d, cf.hd, Om, ph, m, org, W, amp,
                       pl.split > 1 ? part : out, pl.per);
    if (pl.split > 1) {
        const size_t cnt = (size_t)nq * tp;
        hipLaunchKernelGGL(k_cov_apply_finish, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, s, part, pl.split, cnt, cf.hd, W, 0,
                           out);
    }
}

void launch_iter_paths_rhs(const double* yb, const double* f, const double* E, double sn, int count, int n, int tp, double* r,
                           hipStream_t s)
{
    const size_t cnt = (size_t)n * tp;
    hipLaunchKernelGGL(k_iter_paths_rhs, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, s, yb, f, E, sn, count, tp, cnt, r);
}
void launch_iter_paths_add(const double* f, double* k, size_t cnt, hipStream_t s)
{
    hipLaunchKernelGGL(k_iter_paths_add, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, s, f, k, cnt);
}
