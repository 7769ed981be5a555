// iter32_gfx950.h -- the single-precision covariance-times-vectors product of the matrix-free exact GP's mixed mode
// (cugp_iter_set_precision, cugp_iter_apply32) and its launcher.
//
// Include-point contract.  Included INSIDE namespace cugp by kernels.hip, after iter_gfx950.h (k_cov_apply_finish, the d2
// typedef, CUGP_COV_KERNEL, cov_device.h's DC and ard_weights, kernels.h's ITER_*, IterPlan, CovFn).  The per-entry
// function kernel_value32 stands here and not beside kernel_value in cov_device.h: it is built on the hardware
// transcendentals (v_exp_f32, v_log_f32, v_sqrt_f32), which have no host counterpart, and cov_device.h is compiled for the
// host checks as it stands.
//
// k_cov_apply32<ARD, KIND>:  out[i][c] = sum_j fl32(k(a_i, b_j)) fl32(V[j][c])  (+ sn2 V[i][c] in fp64, square form).
//   Vectors in and out are k_cov_apply's fp64 blocks [n][tp]; X and theta are read where they lie and rounded to fp32 on the
//   way into registers (a rows, weights) and into LDS (b rows, V rows).
//   v_mfma_f32_16x16x4_f32, one block: A from lane (fr = lane & 15, fk = lane >> 4) is A[row fr][k fk], B is B[k fk][col fr]
//   -- as the f64 instruction -- but C/D register r of that lane is D[row 4 fk + r][col fr] (f64: row fk + 4 r).
//   The lane computes the entries k(a_{i0 + fr}, b_{j0 + 4 kk + fk}), kk < 8, of a stage of ITER_JT b rows and hands each to NCT
//   MFMAs whose B operand is V[j0 + 4 kk + fk][16 ct + fr] out of the stage's LDS image.
//   Entries in pairs.  The lane's 8 entries are 4 pairs (kk = 2 p, 2 p + 1), every quantity of a pair one float2 in two
//   consecutive registers, and the LDS image of the b rows is laid out for it: ys[(4 p + fk)][c] holds the float2
//   (b_{8 p + fk}[c], b_{8 p + 4 + fk}[c]), so one ds_read_b128 brings two features of a pair and the difference, the weight,
//   the square and the sum are one packed instruction each (v_pk_add_f32 with a negated operand, v_pk_mul_f32, v_pk_mul_f32,
//   v_pk_add_f32): differences before squares, features ascending, no contraction -- k32(i, j) == k32(j, i) in bits.
//   Accumulation.  The MFMA accumulates in fp32 over FOLD = 4 stages (128 consecutive j) at most; then the 4 NCT sums of
//   the lane are converted and added into fp64 carry registers, j ascending, and cleared.  The fold's position counts from
//   the range's first stage: neither t nor tp enters.  The split over j ranges, the partial blocks (fp64) and
//   k_cov_apply_finish are k_cov_apply's; the noise term enters once by one fp64 fma.
//   Rows of b and V beyond nb are staged as zeros.  No atomics.  d > 16: further feature chunks through a third buffer, as
//   k_cov_apply (served, not tuned).
//   LDS: ys [3][16][16] float2 (two stage images and the chunk buffer), vs [2][32][TPL] floats, TPL = 16 | 80: 10 KiB | 26 KiB.
#pragma once

typedef float f2 __attribute__((ext_vector_type(2)));
typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int ITER_FOLD = 4;         // stages an fp32 MFMA accumulator spans before it is folded into fp64: 128 terms

// One pair of entries from the pair's scaled squared distances s (isotropic: |x - x'|^2 / l^2; ARD route: the weighted
// sum), every line one fp32 rounding, the transcendentals the hardware's (1 ulp; no denormal results):
//   SE      kf = sf2 exp2(s (-log2(e) / 2))
//   Matern  a = c sqrt(s), e = exp2(-(a log2 e)), kf = sf2 (p e) with matern_entry's p; e == 0: kf = 0 (its guard)
//   RQ      u = s h2a, kf = sf2 exp2(-(alpha log2(1 + u)))
template <int KIND>
__device__ __forceinline__ f2 kernel_value32(f2 s, float sf2, float alpha, float h2a)
{
#pragma clang fp contract(off)
    constexpr float LOG2E = 1.44269504088896341f;
    f2 e;
    if constexpr (KIND == KERNEL_SE) {
        const f2 x = s * (-0.5f * LOG2E);
        e = (f2){__builtin_amdgcn_exp2f(x[0]), __builtin_amdgcn_exp2f(x[1])};
        return sf2 * e;
    } else if constexpr (KIND == KERNEL_RQ) {
        const f2 w = 1.0f + s * h2a;
        const f2 x = -(alpha * (f2){__builtin_amdgcn_logf(w[0]), __builtin_amdgcn_logf(w[1])});
        e = (f2){__builtin_amdgcn_exp2f(x[0]), __builtin_amdgcn_exp2f(x[1])};
        return sf2 * e;
    } else {
        static_assert(KIND == KERNEL_MATERN32 || KIND == KERNEL_MATERN52, "the four families");
        const float c = KIND == KERNEL_MATERN32 ? 1.7320508075688772f : 2.23606797749979f;
        const f2 a = c * (f2){__builtin_amdgcn_sqrtf(s[0]), __builtin_amdgcn_sqrtf(s[1])};
        const f2 x = -(a * LOG2E);
        e = (f2){__builtin_amdgcn_exp2f(x[0]), __builtin_amdgcn_exp2f(x[1])};
        f2 p = 1.0f + a;
        if constexpr (KIND == KERNEL_MATERN52) p = p + (a * a) * 0.333333333333333333f;
        f2 kf = sf2 * (p * e);
        if (e[0] == 0.0f) kf[0] = 0.0f;
        if (e[1] == 0.0f) kf[1] = 0.0f;
        return kf;
    }
}

template <bool ARD, int KIND, int NCT>
__device__ __forceinline__ void cov_apply32_body(const double* __restrict__ A, int na, const double* __restrict__ B, int nb, int d,
                                                 const HyperScalars* __restrict__ hd, const double* __restrict__ V,
                                                 double* __restrict__ out, int per, int square)
{
#pragma clang fp contract(off)
    constexpr int TP = NCT * 16, TPL = (TP % 32 == 0) ? TP + 16 : TP, NP = ITER_JT / 8;
    static_assert(ITER_JT == 32 && DC == 16, "4 pairs of entries per lane and stage; one feature pair of a b row per thread");
    __shared__ __attribute__((aligned(16))) f2 ys[3][ITER_JT / 2][DC];     // two stage images; [2]: the chunk buffer yc
    __shared__ __attribute__((aligned(16))) float vs[2][ITER_JT][TPL];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fk = lane >> 4;
    const int row = blockIdx.x * ITER_ROWS + wave * 16 + fr;
    const HyperScalars h = *hd;
    const double* __restrict__ wts = ard_weights(hd);
    const float sf2 = (float)h.signal_var, inv_l2 = ARD ? 1.0f : (float)(1.0 / h.ell_sq);
    float alpha = 0.0f, h2a = 0.0f;
    if constexpr (KIND == KERNEL_RQ) { alpha = (float)wts[d]; h2a = (float)wts[d + 1]; }
    const int nst = (nb + ITER_JT - 1) / ITER_JT, nch = (d + DC - 1) / DC;
    const int s0 = blockIdx.y * per, s1 = s0 + per < nst ? s0 + per : nst;

    f4 acc[NCT];                                       // the MFMA's: at most ITER_FOLD stages
    double carry[NCT][4];                              // the folds' sums
#pragma unroll
    for (int ct = 0; ct < NCT; ct++) {
        acc[ct] = (f4){0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int r = 0; r < 4; r++) carry[ct][r] = 0.0;
    }
    float ar[DC];
    [[maybe_unused]] float wr[ARD ? DC : 1];
    auto load_a = [&](int c0) {
#pragma unroll
        for (int c = 0; c < DC; c++) {
            ar[c] = (row < na && c0 + c < d) ? (float)A[(size_t)row * d + c0 + c] : 0.0f;
            if constexpr (ARD) wr[c] = c0 + c < d ? (float)wts[c0 + c] : 1.0f;
        }
    };
    // the thread's share of a stage: one feature pair of one b row, NCT column pairs of V rows; rounded as they arrive
    const int br = tid >> 3, bc = (tid & 7) * 2;
    float* const yslot = (float*)&ys[0][(br >> 3) * 4 + (br & 3)][bc] + ((br >> 2) & 1);   // b row 8 p + 4 half + fk
    f2 rb, rv[NCT];
    auto fetch_b = [&](int j0, int c0) {
        const int j = j0 + br, c = c0 + bc;
        rb[0] = (j < nb && c < d) ? (float)B[(size_t)j * d + c] : 0.0f;
        rb[1] = (j < nb && c + 1 < d) ? (float)B[(size_t)j * d + c + 1] : 0.0f;
    };
    auto fetch = [&](int st) {
        const int j0 = st * ITER_JT;
        fetch_b(j0, 0);
#pragma unroll
        for (int q = 0; q < NCT; q++) {
            const int e = tid + 256 * q, j = j0 + e / (TP / 2);
            const d2 v = j < nb ? *(const d2*)(V + (size_t)j * TP + 2 * (e % (TP / 2))) : (d2){0.0, 0.0};
            rv[q] = (f2){(float)v[0], (float)v[1]};
        }
    };
    auto put_b = [&](int buf) {                        // (the two features of the row: 8 bytes apart in the pair layout)
        yslot[buf * (ITER_JT / 2) * DC * 2] = rb[0];
        yslot[buf * (ITER_JT / 2) * DC * 2 + 2] = rb[1];
    };
    auto put = [&](int buf) {
        put_b(buf);
#pragma unroll
        for (int q = 0; q < NCT; q++) {
            const int e = tid + 256 * q;
            *(f2*)&vs[buf][e / (TP / 2)][2 * (e % (TP / 2))] = rv[q];
        }
    };
    f2 sq[NP];
    // sq[p] += the chunk's terms of |(a_row - b) w|^2 for the pair's two b rows, features ascending (beyond d: 0 - 0)
    auto accumulate = [&](const f2 (*yb)[DC], int c0) {
#pragma unroll
        for (int cp = 0; cp < DC / 2; cp++) {
            const int c = 2 * cp;
            if (c0 + c < d) {
#pragma unroll
                for (int p = 0; p < NP; p++) {
                    const f4 yv = *(const f4*)&yb[p * 4 + fk][c];
                    f2 df = ar[c] - (f2){yv[0], yv[1]};
                    if constexpr (ARD) df = df * wr[c];
                    sq[p] = sq[p] + df * df;
                    df = ar[c + 1] - (f2){yv[2], yv[3]};
                    if constexpr (ARD) df = df * wr[c + 1];
                    sq[p] = sq[p] + df * df;
                }
            }
        }
    };
    auto fold = [&]() {
#pragma unroll
        for (int ct = 0; ct < NCT; ct++) {
#pragma unroll
            for (int r = 0; r < 4; r++) carry[ct][r] = carry[ct][r] + (double)acc[ct][r];
            acc[ct] = (f4){0.0f, 0.0f, 0.0f, 0.0f};
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
        for (int p = 0; p < NP; p++) sq[p] = (f2){0.0f, 0.0f};
        accumulate(ys[cur], 0);
        for (int ch = 1; ch < nch; ch++) {
            const f2 keep = rb;
            fetch_b(st * ITER_JT, ch * DC);
            __syncthreads();
            put_b(2);
            rb = keep;
            load_a(ch * DC);
            __syncthreads();
            accumulate(ys[2], ch * DC);
        }
        if (nch > 1) load_a(0);
#pragma unroll
        for (int p = 0; p < NP; p++) {
            const f2 kv = kernel_value32<KIND>(ARD ? sq[p] : sq[p] * inv_l2, sf2, alpha, h2a);
#pragma unroll
            for (int hf = 0; hf < 2; hf++)
#pragma unroll
                for (int ct = 0; ct < NCT; ct++)
                    acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(kv[hf], vs[cur][(2 * p + hf) * 4 + fk][ct * 16 + fr], acc[ct], 0, 0, 0);
        }
        if (((st - s0) & (ITER_FOLD - 1)) == ITER_FOLD - 1) fold();
        if (more) put(cur ^ 1);
        __syncthreads();
    }
    fold();                                            // (an empty last fold adds +0.0: no bit changes)
    const bool direct = gridDim.y == 1;
    double* __restrict__ o = out + (size_t)blockIdx.y * na * TP;
#pragma unroll
    for (int ct = 0; ct < NCT; ct++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int i = blockIdx.x * ITER_ROWS + wave * 16 + 4 * fk + r;
            if (i < na) {
                const size_t e = (size_t)i * TP + ct * 16 + fr;
                double v = carry[ct][r];
                if (square && direct) v = __builtin_fma(h.noise_var, V[e], v);
                o[e] = v;
            }
        }
}

// one column tile (t <= 16) and four (t <= 64), as k_cov_apply's two
template <bool ARD, int KIND>
__global__ __launch_bounds__(256) void k_cov_apply32(const double* __restrict__ A, int na, const double* __restrict__ B, int nb,
                                                     int d, const HyperScalars* __restrict__ hd, const double* __restrict__ V,
                                                     double* __restrict__ out, int per, int square)
{
    cov_apply32_body<ARD, KIND, 1>(A, na, B, nb, d, hd, V, out, per, square);
}
template <bool ARD, int KIND>
__global__ __launch_bounds__(256) void k_cov_apply32_4(const double* __restrict__ A, int na, const double* __restrict__ B, int nb,
                                                       int d, const HyperScalars* __restrict__ hd, const double* __restrict__ V,
                                                       double* __restrict__ out, int per, int square)
{
    cov_apply32_body<ARD, KIND, 4>(A, na, B, nb, d, hd, V, out, per, square);
}

void launch_cov_apply32(const double* A, int na, const double* B, int nb, int d, const CovFn& cf, const double* V, int tp,
                        double* out, double* part, const IterPlan& pl, bool square, hipStream_t s)
{
    assert(cf.hd && (tp == 16 || tp == IT_MAXT) && (pl.split == 1 || part));
    auto kern = tp == 16 ? CUGP_COV_KERNEL(cf, k_cov_apply32) : CUGP_COV_KERNEL(cf, k_cov_apply32_4);
    hipLaunchKernelGGL(kern, dim3(pl.row_blocks, pl.split), dim3(256), 0, s, A, na, B, nb, d, cf.hd, V,
                       pl.split > 1 ? part : out, pl.per, square ? 1 : 0);
    if (pl.split > 1) {
        const size_t cnt = (size_t)na * tp;
        hipLaunchKernelGGL(k_cov_apply_finish, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, s, part, pl.split, cnt, cf.hd, V,
                           square ? 1 : 0, out);
    }
}
