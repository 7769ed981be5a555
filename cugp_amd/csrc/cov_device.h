// cov_device.h -- the covariance-function device code that runs on a host as well as on the GPU: the per-entry and
// micro-tile helpers of every pass that evaluates the covariance function, and the gradient passes built on them alone
// (the ARD trace, the test-input gradient).  Plain fp64 arithmetic, __syncthreads and wave shuffles: no MFMA, no atomics,
// no inline assembly, no stamps.  kernels.hip includes it for gfx950; the host checks (tools/*_host_check.cpp) include
// the same text behind the emulation shim tools/host_emul.h and run it under -fsanitize=address,undefined, so nothing
// here may fork on the compiler: no #ifdef around arithmetic.
//
// Include-point contract.  Included INSIDE namespace cugp, after these are declared -- the file declares none of them:
//   kernels.h                      TILE, HyperScalars, ExpertPtrs, KERNEL_*
//   kernels.hip / host_emul.h      the d2 and d4 typedefs, GP, and the device vocabulary (__device__, __global__,
//                                  __shared__, threadIdx, blockIdx, gridDim, __syncthreads, __shfl_xor, __shfl_down)
// What needs the device although it uses the helpers below: trace_body with finalize_sums (agent-scope atomics,
// s_waitcnt, a fence) and build_body (the launch stamp) with its sibling cross_body, in eval_gfx950.h;
// predict_cov_finish_body in predict_gfx950.h.  The launchers of the kernels below are in predict_gfx950.h.
#pragma once

// lower-triangular tile index: idx -> (ti >= tj)
__device__ __forceinline__ void tri_index(int idx, int& ti, int& tj)
{
    int r = (int)((sqrt(8.0 * (double)idx + 1.0) - 1.0) * 0.5);
    while ((r + 1) * (r + 2) / 2 <= idx) r++;
    while (r * (r + 1) / 2 > idx) r--;
    ti = r;
    tj = idx - r * (r + 1) / 2;
}

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

constexpr int KT = 64;      // kernel-build tile
constexpr int DC = 16;      // feature chunk staged per pass

// the 4 columns of a thread's 4x4 micro-tile inside the 64-column tile: two adjacent pairs, 32 apart, so that the 16
// lanes of a row make one 256-byte run per 16-byte access (columns 4 tx + b made two half-used runs of 512 bytes)
__device__ __forceinline__ int col4(int tx, int b) { return (b >> 1) * 32 + tx * 2 + (b & 1); }

// squared distances of a 4x4 micro-tile, accumulated over d in index order without FMA
// contraction so that the value matches the reference's sub / mul / add sequence bit for bit
// ARD: every difference is multiplied by its dimension's weight w_c = 1 / l_c before it is squared (the DIFFERENCE, not
// the coordinates: x_a - y_b of nearby points stays exact); wts: the d weights in device memory, ws: LDS for the
// current chunk's.  The isotropic instantiation is the code it was before the flag existed.
template <bool ARD = false>
__device__ __forceinline__ void sqdist_4x4(const double* __restrict__ X, const double* __restrict__ Y, int nx,
                                           int ny, int d, int i0, int j0, double (&xs)[KT][DC + 1],
                                           double (&ys)[KT][DC + 1], double (&acc)[4][4],
                                           const double* __restrict__ wts = nullptr, double* ws = nullptr)
{
#pragma clang fp contract(off)
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b = 0; b < 4; b++) acc[a][b] = 0.0;
    for (int c0 = 0; c0 < d; c0 += DC) {
        const int dc = (d - c0 < DC) ? (d - c0) : DC;
        __syncthreads();
        for (int e = t; e < KT * dc; e += 256) {
            int r = e / dc, c = e - r * dc;
            xs[r][c] = (i0 + r < nx) ? X[(size_t)(i0 + r) * d + c0 + c] : 0.0;
            ys[r][c] = (j0 + r < ny) ? Y[(size_t)(j0 + r) * d + c0 + c] : 0.0;
        }
        if (ARD && t < dc) ws[t] = wts[c0 + t];
        __syncthreads();
        for (int c = 0; c < dc; c++) {
            double xv[4], yv[4];
#pragma unroll
            for (int a = 0; a < 4; a++) { xv[a] = xs[ty * 4 + a][c]; yv[a] = ys[col4(tx, a)][c]; }
            const double wc = ARD ? ws[c] : 1.0;
#pragma unroll
            for (int a = 0; a < 4; a++)
#pragma unroll
                for (int b = 0; b < 4; b++) {
                    double df = xv[a] - yv[b];
                    if (ARD) df = df * wc;
                    acc[a][b] = acc[a][b] + df * df;
                }
        }
    }
}

// a / b for many a and one b: with y = RN(1/b) from one real division, q0 = RN(a y), the exact remainder a - b q0 by
// FMA and q = RN(q0 + rem y) give the correctly rounded quotient (Markstein; 2e7 random pairs identical to a / b) in
// three instructions instead of the ~18 of a full IEEE division per matrix entry.  Only while b and 1/b are far
// from the ends of the exponent range (the optimisers do walk l^2 = exp(2 theta) to infinity: a / inf must stay 0,
// 0 * inf is NaN): DivBy::y == 0 selects the real division (uniform over the launch).
struct DivBy { double b, y; };
// ARD handles keep the d per-dimension weights directly behind the hyper-scalars (one staging area, one copy)
__device__ __forceinline__ const double* ard_weights(const HyperScalars* hd) { return (const double*)(hd + 1); }
__device__ __forceinline__ DivBy div_prepare(double b)
{
    return DivBy{b, (b > 1e-100 && b < 1e100) ? 1.0 / b : 0.0};
}
__device__ __forceinline__ double div_by(double a, const DivBy& d)
{
    if (d.y == 0.0) return a / d.b;
    const double q0 = a * d.y;
    const double rem = __builtin_fma(-q0, d.b, a);
    return __builtin_fma(rem, d.y, q0);
}

// ---- Matern 3/2 and 5/2 (GPML covMaterniso / covMaternard, d = 3 and 5): KIND as kernels.h's KERNEL_* ----
// One entry from s = |x - x'|^2 / l^2 (by div_by, as SE's; ARD: s = sum u_c^2, u_c = (x_c - x'_c) w_c, sqdist_4x4<true>):
// r = sqrt(s) correctly rounded, a = c r with c = RN(sqrt 3) or RN(sqrt 5), ONE exp(-a), then
//   kf = sf2 (p e),   dk = dkf / dlog l = sf2 (q e),   hh = H = sf2 (g e)   with
//   3/2:  p = 1 + a,               q = a a,          g = 3
//   5/2:  p = (1 + a) + t,         q = t (1 + a),    g = RN(5/3) (1 + a),    t = (a a) RN(1/3)
// H is the factor of the per-dimension and the test-input derivatives (no singularity at a = 0):
//   dk / dtheta_c = H u_c^2,   dk / dx*_c = -H (x*_c - x_c) s_c   (s_c = 1 / l^2, ARD w_c^2)
// a a / 3 as a multiply by the rounded constant: an fp64 division is ~18 VALU instructions per entry where the multiply
// is one, and it adds one rounding (of the constant) to a polynomial without cancellation.  No FMA contraction: the
// CPU copy of these lines (tests/truth_matern.py) takes the same roundings.
// Extremes: s = 0 -> a = 0, e = 1: kf = sf2 exactly, dk = 0.  s = +inf (l^2 = 0) -> e = 0, and so for a finite a whose
// exp underflows: all three are 0 exactly (the guard: (1 + inf) * 0 and, for a > 1e154, (a a) * 0 would be NaN).
// Callers take what they need: an unused output is dead code to the compiler.
template <int KIND>
__device__ __forceinline__ void matern_entry(double s, double sf2, double& kf, double& dk, double& hh)
{
#pragma clang fp contract(off)
    static_assert(KIND == KERNEL_MATERN32 || KIND == KERNEL_MATERN52, "Matern kinds only");
    const double c = KIND == KERNEL_MATERN32 ? 1.7320508075688772 : 2.23606797749979;
    const double a = c * __builtin_sqrt(s);
    const double e = exp(-a);
    const double p1 = 1.0 + a;
    double p, q, g;
    if (KIND == KERNEL_MATERN32) {
        p = p1;
        q = a * a;
        g = 3.0;
    } else {
        const double t = (a * a) * 0.3333333333333333;
        p = p1 + t;
        q = t * p1;
        g = 1.6666666666666667 * p1;
    }
    const bool dead = e == 0.0;
    kf = dead ? 0.0 : sf2 * (p * e);
    dk = dead ? 0.0 : sf2 * (q * e);
    hh = dead ? 0.0 : sf2 * (g * e);
}
// ARD entry from the WEIGHTED squared distance s (no division, ell_sq is not read): kf and the factor H of the
// per-dimension derivatives -- SE: kf = sf2 exp(-s / 2) and H = kf; the Matern kinds matern_entry at s
template <int KIND>
__device__ __forceinline__ void ard_entry(double s, double sf2, double& kf, double& hh)
{
    if constexpr (KIND == KERNEL_SE) {
        kf = sf2 * exp(-0.5 * s);
        hh = kf;
    } else {
        double dk;
        matern_entry<KIND>(s, sf2, kf, dk, hh);
    }
}
// ---- rational quadratic (GPML covRQiso / covRQard), KERNEL_RQ: the ARD route only ----
// One entry from the WEIGHTED squared distance s = sum u_c^2 (sqdist_4x4<true>), alpha = exp(theta_alpha) and h2a =
// RN(0.5 / alpha), both evaluated on the host.  One log1p, one exp and one division per entry, every line one rounding:
//   u  = RN(s h2a)                      s / (2 alpha)
//   L  = log1p(u)
//   e  = exp(-RN(alpha L))              (1 + u)^-alpha
//   kf = RN(sf2 e)
//   r  = RN(1 / RN(1 + u))
//   hh = RN(kf r)                       H = Kf / (1 + u):  dK / dtheta_c = H u_c^2,  dk / dx*_c = -H (x*_c - x_c) w_c^2
//   da = RN(kf RN(alpha RN(RN(u r) - L)))   A = dK / dtheta_alpha = Kf alpha (u / (1 + u) - L)
// u r - L cancels to -u^2 / 2 for small u: its error is absolute, ~2 eps u, and A's ~Kf alpha 2 eps u (tests/truth_rq.py
// counts it).  No FMA contraction: the CPU copy of these lines (tests/truth_rq.py entry_fp64) takes the same roundings.
// Extremes: s = 0 -> u = 0, L = 0, e = 1, r = 1: kf = hh = sf2 and da = 0 exactly.  alpha -> inf approaches SE's
// sf2 exp(-s / 2).  An alpha whose exp overflowed (inf, h2a = 0) gives inf * 0 = NaN in every output.
struct ShapeArgs { double alpha, h2a; };
// the shape parameters of a handle's family, which lie behind the d weights (wts) in the staging area
template <int KIND>
__device__ __forceinline__ ShapeArgs shape_args(const double* __restrict__ wts, int d)
{
    if constexpr (KIND == KERNEL_RQ) return ShapeArgs{wts[d], wts[d + 1]};
    else return ShapeArgs{0.0, 0.0};
}
__device__ __forceinline__ void rq_entry(double s, double sf2, double alpha, double h2a, double& kf, double& hh, double& da)
{
#pragma clang fp contract(off)
    const double u = s * h2a;
    const double L = log1p(u);
    const double e = exp(-(alpha * L));
    kf = sf2 * e;
    const double r = 1.0 / (1.0 + u);
    hh = kf * r;
    da = kf * (alpha * (u * r - L));
}
// the same with the family's shape parameters: da = dK / dtheta_shape (RQ; the other kinds have none: 0, dead code)
template <int KIND>
__device__ __forceinline__ void ard_entry(double s, double sf2, const ShapeArgs& sh, double& kf, double& hh, double& da)
{
    if constexpr (KIND == KERNEL_RQ) {
        rq_entry(s, sf2, sh.alpha, sh.h2a, kf, hh, da);
    } else {
        ard_entry<KIND>(s, sf2, kf, hh);
        da = 0.0;
    }
}
// the value of one entry without the noise term (the three passes that need no derivative)
template <bool ARD, int KIND>
__device__ __forceinline__ double kernel_value(double d2, const DivBy& dl, double sf2, const ShapeArgs& sh = ShapeArgs{0.0, 0.0})
{
    double kf, dk, hh;
    if constexpr (KIND == KERNEL_RQ) {
        static_assert(ARD || KIND != KERNEL_RQ, "the rational quadratic kernel has ARD instantiations only");
        rq_entry(d2, sf2, sh.alpha, sh.h2a, kf, hh, dk);
    } else if constexpr (ARD)
        ard_entry<KIND>(d2, sf2, kf, hh);
    else if constexpr (KIND == KERNEL_SE)
        kf = sf2 * exp(div_by(-d2 * 0.5, dl));                    // covkernel.cpp:89
    else
        matern_entry<KIND>(div_by(d2, dl), sf2, kf, dk, hh);
    return kf;
}

// Multi-target regression (the section further down): S[a][b] = sum_t A[t][i0 + 4 ty + a] A[t][j0 + col4(tx, b)] of the thread's 4x4 micro-tile, t ascending, no contraction.
// The two 64-entry runs of A per target (contiguous, 512 B each) go through LDS, TGT_CHUNK targets at a time.
constexpr int TGT_CHUNK = 16;
__device__ __forceinline__ void targets_outer_4x4(const double* __restrict__ A, int ld, int m, int i0, int j0,
                                                  double (&la)[TGT_CHUNK][KT], double (&lb)[TGT_CHUNK][KT],
                                                  double (&S)[4][4])
{
#pragma clang fp contract(off)
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b = 0; b < 4; b++) S[a][b] = 0.0;
    for (int t0 = 0; t0 < m; t0 += TGT_CHUNK) {
        const int tc = (m - t0 < TGT_CHUNK) ? (m - t0) : TGT_CHUNK;
        __syncthreads();
        for (int e = t; e < tc * 64; e += 256) {              // 16-byte pieces: 32 of the row run, 32 of the column run
            const int r = e >> 6, q = e & 63;
            const double* row = A + (size_t)(t0 + r) * ld;
            if (q < 32) *(d2*)&la[r][2 * q] = *(const d2*)(row + i0 + 2 * q);
            else *(d2*)&lb[r][2 * (q - 32)] = *(const d2*)(row + j0 + 2 * (q - 32));
        }
        __syncthreads();
        for (int r = 0; r < tc; r++) {
            const d2 a01 = *(const d2*)&la[r][ty * 4], a23 = *(const d2*)&la[r][ty * 4 + 2];
            const d2 b01 = *(const d2*)&lb[r][tx * 2], b23 = *(const d2*)&lb[r][32 + tx * 2];
            const double ai[4] = {a01[0], a01[1], a23[0], a23[1]}, aj[4] = {b01[0], b01[1], b23[0], b23[1]};
#pragma unroll
            for (int a = 0; a < 4; a++)
#pragma unroll
                for (int b = 0; b < 4; b++) S[a][b] = S[a][b] + ai[a] * aj[b];
        }
    }
}

// ---- ARD (one length scale per input dimension; GPML covSEard / covMaternard; no reference counterpart) ----
// Gradient pass, ONE body for SE and both Matern kinds: g_c = 1/2 sum_ij W_ij H_ij ((x_ic - x_jc) w_c)^2 for every
// dimension c (ard_entry's H: SE's Kf itself), beside the two sums k_trace takes (sum W o K and tr W).  Per lower 64x64
// tile: (1) the weighted squared distances over all feature chunks, K^-1 read once, and the thread's 4x4 entries 2 (w H)
// kept in registers (off-diagonal tiles doubled, entries outside the lower triangle or the data zero; the diagonal's
// differences are zero: it has no share in any g_c); sum W o K takes Kf (+ sn2 on the diagonal); (2) a second sweep over
// the feature chunks, the X tiles staged again, DC per-dimension sums at a time in registers; wave sums by shuffles, the
// four waves added in a fixed order.
// Partials: part[c * nblocks + block], c = 0 .. d - 1 the dimensions, then the family's shape columns (RQ: one, sum W o
// dK/dtheta_alpha, off-diagonal entries doubled, reduced as the next two; the other kinds: none), then sum W o K and tr W
// (column-major, so that k_finalize_ard's lanes read a column contiguously).  No fused final sums: k_finalize_ard / k_finalize_targets follow.
// TARGETS: W = m K^-1 - sum_t alpha_t alpha_t^T from the target-major AV ([m][npad]), single handle; else W = K^-1 -
// alpha alpha^T from the vector AV, and bt (batched): blockIdx.y selects the expert -- X, n, K^-1, alpha and the
// expert's OWN partials from its table entry; hyper-scalars and weights are the group's one copy (hd).  The arithmetic
// and its order per expert are the single launch's.
template <int KIND, bool TARGETS>
__device__ __forceinline__ void trace_ard_body(const double* __restrict__ X, int n, int d, int npad,
                                               const HyperScalars* __restrict__ hd,
                                               const double* __restrict__ Kinv, const double* __restrict__ AV,
                                               int m, double* __restrict__ part,
                                               const ExpertPtrs* __restrict__ bt)
{
#pragma clang fp contract(off)
    if (!TARGETS && bt) {
        const ExpertPtrs& e = bt[blockIdx.y];
        X = GP(e.X); n = e.n; Kinv = GP(e.Kinv); AV = GP(e.alpha); part = GP(e.part);
    }
    const HyperScalars h = *hd;
    const double* __restrict__ wts = ard_weights(hd);
    __shared__ double xs[KT][DC + 1], ys[KT][DC + 1];
    __shared__ __attribute__((aligned(16))) double la[TARGETS ? TGT_CHUNK : 1][KT], lb[TARGETS ? TGT_CHUNK : 1][KT];
    __shared__ double ws[DC];
    __shared__ double red[DC][4];
    int ti, tj;
    tri_index(blockIdx.x, ti, tj);
    const int i0 = ti * KT, j0 = tj * KT;
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const size_t nblocks = gridDim.x;
    double wk[4][4], S[4][4];
    sqdist_4x4<true>(X, X, n, n, d, i0, j0, xs, ys, wk, wts, ws);
    double aj[4];
    if constexpr (TARGETS) {
        targets_outer_4x4(AV, npad, m, i0, j0, la, lb, S);
    } else {
#pragma unroll
        for (int b = 0; b < 4; b++) aj[b] = AV[j0 + col4(tx, b)];
    }
    double s2 = 0.0, s3 = 0.0, s4 = 0.0;                 // s4: sum W o dK/dtheta_shape (NS columns; RQ: one)
    constexpr int NS = shape_count(KIND);
    const ShapeArgs sh = shape_args<KIND>(wts, d);
    const double dm = (double)m;
#pragma unroll
    for (int a = 0; a < 4; a++) {
        const int i = i0 + ty * 4 + a;
        const double ai = TARGETS ? 0.0 : AV[i];
        const double* kr = Kinv + (size_t)i * npad + j0 + tx * 2;
        d2 k01 = *(const d2*)kr, k23 = *(const d2*)(kr + 32);
        const double kv[4] = {k01[0], k01[1], k23[0], k23[1]};
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const int j = j0 + col4(tx, b);
            double e = 0.0;
            if (i < n && j < n && (ti != tj || j <= i)) {
                const double w = TARGETS ? dm * kv[b] - S[a][b] : kv[b] - ai * aj[b];
                double kf, hh;
                if constexpr (NS == 0) {
                    ard_entry<KIND>(wk[a][b], h.signal_var, kf, hh);
                } else {
                    double da;
                    ard_entry<KIND>(wk[a][b], h.signal_var, sh, kf, hh, da);
                    if (i != j) s4 += 2.0 * (w * da);      // (the diagonal's da is zero: no share)
                }
                if (i == j) {
                    kf += h.noise_var;
                    s2 += w * kf;
                    s3 += w;
                } else {
                    e = 2.0 * (w * hh);
                    s2 += 2.0 * (w * kf);
                }
            }
            wk[a][b] = e;
        }
    }
    s2 = wave_sum(s2); s3 = wave_sum(s3);
    if ((t & 63) == 0) { red[0][t >> 6] = s2; red[1][t >> 6] = s3; }
    if constexpr (NS > 0) {
        s4 = wave_sum(s4);
        if ((t & 63) == 0) red[2][t >> 6] = s4;
    }
    __syncthreads();
    if (t < 2) part[(size_t)(d + NS + t) * nblocks + blockIdx.x] = (red[t][0] + red[t][1]) + (red[t][2] + red[t][3]);
    if constexpr (NS > 0) {
        if (t == 2) part[(size_t)d * nblocks + blockIdx.x] = (red[2][0] + red[2][1]) + (red[2][2] + red[2][3]);
    }
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

// ------------------------------------------------------------------------------------------
// Gradients of the predictive mean and variance with respect to the test inputs (cugp_predict_grad).  With
// k_i = k(x*, x_i), dk_i / dx*_c = -G_i (x*_c - x_ic) s_c  (G: SE and ARD k_i, Matern 3/2 sf2 3 e^-a, 5/2 sf2 (5/3)(1 + a) e^-a;
// s_c = 1 / l^2, ARD w_c^2), v = K^-1 k* = row t of V = W L^-1:
//   dmean[t][c] = -s_c sum_i (G alpha_i) (x*_c - x_ic),     dvar[t][c] = +2 s_c sum_i (G V_ti) (x*_c - x_ic)
// One 64 x 64 (test x training) tile per workgroup, the thread's 4 x 4 micro-tile and column pairs as k_cross's (16-byte
// loads of Ks and V rows).  SE, and SE with ARD, read G from Ks (k_cross's own exp, no second one: the ARD weights enter
// through the finish alone, so the two instantiations are the same code); the Matern kinds take the squared distance --
// ARD: the weighted one -- from sqdist_4x4<ARD> and G = H of matern_entry (RQ: of rq_entry), one exp per entry.  The second sweep takes
// the UNWEIGHTED differences (k_predict_grad_finish applies s_c once per output).  Per feature, X and Xt staged
// through LDS DC features at a time: the DIFFERENCE x*_c - x_ic is formed first and then multiplied -- the algebraically
// equal x*_c sum(G alpha) - sum(G alpha x_c) cancels where |x| >> |x - x'|.  A thread adds its four columns in index order,
// the 16 lanes of a row add by a butterfly of fixed shape (lane distances 1, 2, 4, 8; a + b == b + a, so all 16 hold the same
// bits), and lane c mod 16 writes the tile's partial sum: part[(ti * 2 + q) * pstride + t * d + c], q = 0 mean, 1 variance.
// No atomics; a row's sums do not depend on where in a tile or a pass the row lies.  Entries beyond row nt of Xt or row n
// of X contribute exact zeros (G alpha and G V are set to 0.0 there, the staged coordinates too) and are never read from
// X or Xt; Ks and V are [.. >= 64 * tiles][npad] and read inside that.
// k_predict_grad_finish adds the tiles' partial sums in tile order and applies -s_c and +2 s_c once per output.
// ------------------------------------------------------------------------------------------
template <bool ARD, int KIND>
__device__ __forceinline__ void predict_grad_body(const double* __restrict__ X, int n, int d, int npad,
                                                  const double* __restrict__ Xt, int nt, HyperScalars h_arg,
                                                  const double* __restrict__ Ks, const double* __restrict__ V,
                                                  const double* __restrict__ alpha, double* __restrict__ part,
                                                  size_t pstride, const HyperScalars* __restrict__ hd)
{
#pragma clang fp contract(off)
    __shared__ double xs[KT][DC + 1], ys[KT][DC + 1];
    const int tiles_i = (n + KT - 1) / KT;
    const int tt = blockIdx.x / tiles_i, ti = blockIdx.x % tiles_i;
    const int t0 = tt * KT, i0 = ti * KT;
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    double G[4][4];
    if constexpr (KIND != KERNEL_SE) {                 // (SE reads G from Ks below: h and hd are not read)
        __shared__ double ws[DC];
        const HyperScalars& h = ARD ? *hd : h_arg;
        sqdist_4x4<ARD>(Xt, X, nt, n, d, t0, i0, xs, ys, G, ARD ? ard_weights(hd) : nullptr, ws);
        const DivBy dl = div_prepare(h.ell_sq);
        ShapeArgs sh = ShapeArgs{0.0, 0.0};
        if constexpr (KIND == KERNEL_RQ) sh = shape_args<KIND>(ard_weights(hd), d);
#pragma unroll
        for (int a = 0; a < 4; a++)
#pragma unroll
            for (int b = 0; b < 4; b++) {
                double kf, dk, hh;
                if constexpr (KIND == KERNEL_RQ) rq_entry(G[a][b], h.signal_var, sh.alpha, sh.h2a, kf, hh, dk);
                else matern_entry<KIND>(ARD ? G[a][b] : div_by(G[a][b], dl), h.signal_var, kf, dk, hh);
                G[a][b] = hh;
            }
    }
    double ga[4][4], gv[4][4];
    double al[4];
#pragma unroll
    for (int b = 0; b < 4; b++) {
        const int i = i0 + col4(tx, b);
        al[b] = i < n ? alpha[i] : 0.0;
    }
#pragma unroll
    for (int a = 0; a < 4; a++) {
        const int tr = t0 + ty * 4 + a;
        const size_t off = (size_t)tr * npad + i0 + tx * 2;
        double vv[4] = {0.0, 0.0, 0.0, 0.0};
        if constexpr (KIND == KERNEL_SE) {
            const d2 k01 = *(const d2*)(Ks + off), k23 = *(const d2*)(Ks + off + 32);
            G[a][0] = k01[0]; G[a][1] = k01[1]; G[a][2] = k23[0]; G[a][3] = k23[1];
        }
        if (V) {
            const d2 v01 = *(const d2*)(V + off), v23 = *(const d2*)(V + off + 32);
            vv[0] = v01[0]; vv[1] = v01[1]; vv[2] = v23[0]; vv[3] = v23[1];
        }
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const bool in = tr < nt && i0 + col4(tx, b) < n;
            ga[a][b] = in ? G[a][b] * al[b] : 0.0;
            gv[a][b] = in ? G[a][b] * vv[b] : 0.0;
        }
    }
    // one chunk of features of the tile's test rows (xs) and training rows (ys) into LDS, zeros beyond nt and n
    auto stage = [&](int c0, int dc) {
        __syncthreads();
        for (int e = t; e < KT * dc; e += 256) {
            const int r = e / dc, c = e - r * dc;
            xs[r][c] = (t0 + r < nt) ? Xt[(size_t)(t0 + r) * d + c0 + c] : 0.0;
            ys[r][c] = (i0 + r < n) ? X[(size_t)(i0 + r) * d + c0 + c] : 0.0;
        }
        __syncthreads();
    };
    double* pm_out = part + (size_t)ti * 2 * pstride;
    double* pv_out = pm_out + pstride;
    for (int c0 = 0; c0 < d; c0 += DC) {
        const int dc = (d - c0 < DC) ? (d - c0) : DC;
        stage(c0, dc);
        for (int c = 0; c < dc; c++) {
            double xv[4], yv[4], pm[4], pv[4];
#pragma unroll
            for (int a = 0; a < 4; a++) { xv[a] = xs[ty * 4 + a][c]; yv[a] = ys[col4(tx, a)][c]; }
#pragma unroll
            for (int a = 0; a < 4; a++) {
                pm[a] = 0.0; pv[a] = 0.0;
#pragma unroll
                for (int b = 0; b < 4; b++) {
                    const double df = xv[a] - yv[b];
                    pm[a] = pm[a] + ga[a][b] * df;
                    pv[a] = pv[a] + gv[a][b] * df;
                }
            }
#pragma unroll
            for (int m = 1; m < 16; m <<= 1)
#pragma unroll
                for (int a = 0; a < 4; a++) {
                    pm[a] = pm[a] + __shfl_xor(pm[a], m, 16);
                    if (V) pv[a] = pv[a] + __shfl_xor(pv[a], m, 16);
                }
            if (tx == (c & 15)) {
#pragma unroll
                for (int a = 0; a < 4; a++) {
                    const int tr = t0 + ty * 4 + a;
                    if (tr < nt) {
                        pm_out[(size_t)tr * d + c0 + c] = pm[a];
                        if (V) pv_out[(size_t)tr * d + c0 + c] = pv[a];
                    }
                }
            }
        }
    }
}

template <bool ARD, int KIND>
__global__ __launch_bounds__(256) void k_predict_grad(const double* __restrict__ X, int n, int d, int npad,
                                                      const double* __restrict__ Xt, int nt, HyperScalars h_arg,
                                                      const double* __restrict__ Ks, const double* __restrict__ V,
                                                      const double* __restrict__ alpha, double* __restrict__ part,
                                                      size_t pstride, const HyperScalars* __restrict__ hd)
{
    predict_grad_body<ARD, KIND>(X, n, d, npad, Xt, nt, h_arg, Ks, V, alpha, part, pstride, hd);
}

// dmean[t][c] = -s_c (P_0 + P_1 + ...), dvar[t][c] = (2 s_c) (Q_0 + Q_1 + ...): the tiles' partial sums in tile order, packed
// [nt][d]; s_c = 1 / l^2, or (wts given: ARD) w_c^2.  dvar null: the mean's gradient alone.
__global__ __launch_bounds__(256) void k_predict_grad_finish(const double* __restrict__ part, size_t pstride, int tiles,
                                                             int nt, int d, double ell_sq,
                                                             const double* __restrict__ wts, double* __restrict__ dmean,
                                                             double* __restrict__ dvar)
{
#pragma clang fp contract(off)
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)nt * d) return;
    const int c = (int)(e % d);
    const double sc = wts ? wts[c] * wts[c] : 1.0 / ell_sq;
    double sm = part[e], sv = dvar ? part[pstride + e] : 0.0;
    for (int ti = 1; ti < tiles; ti++) {
        sm = sm + part[(size_t)ti * 2 * pstride + e];
        if (dvar) sv = sv + part[((size_t)ti * 2 + 1) * pstride + e];
    }
    if (dmean) dmean[e] = -(sc * sm);
    if (dvar) dvar[e] = (2.0 * sc) * sv;
}
