// iter_varcache_gfx950.h -- the variance cache of the matrix-free exact GP (cugp_iter_varcache_build, cugp_iter_predict_cached;
// DESIGN.md section 41): the fused cached variance k_cov_var, the tall kernels of the block Arnoldi build that k_pc_project and
// k_pc_correct (iter_gfx950.h) do not cover, and the launchers of these and of iter_device.h's one-workgroup kernels.
//
// Include-point contract.  Included INSIDE namespace cugp by kernels.hip, after iter_gfx950.h (everything that header needs, and
// k_cov_apply's constants) and iter_device.h (k_vc_*, k_cov_var_finish).
//
// k_cov_var<ARD, KIND>:  u[i][c] = sum_j k(xt_i, x_j) R[j][c] for a GROUP of 16 NCT = 128 columns of R, squared and summed over
//   the group inside the launch: neither K(Xt, X) nor u [nt][rp] is stored.  k_cov_apply's decomposition -- a workgroup of 4
//   waves owns ITER_ROWS = 64 test rows, lane (fr = lane & 15, fk = lane >> 4) computes the ONE entry k(xt_{i0 + fr}, x_{j + fk})
//   (differences before squares, kernel_value as it stands) and hands it to v_mfma_f64_16x16x4_f64 as the A operand -- but the
//   entry now feeds NCT = 8 MFMAs instead of 1 | 4: the exp / pow / sqrt of an entry is paid once per 128 columns of R.  B is
//   R[j + fk][128 z + 16 ct + fr] out of the LDS image of the stage's 32 rows of R's group; 8 d4 accumulators per lane.  The next
//   stage's x rows and R rows (8 d2 per thread) are in flight in registers behind the MFMAs and go into the other image: one
//   barrier per stage.  LDS: ys [2][32][16], yc [32][16], vs [2][32][144] (row pitch 128 + 16 doubles: 128 B mod 256 B, the two
//   k rows of a half-wave's ds_read_b64 fall on different banks): 84 KiB, one workgroup per CU beside a second of another launch.
//   grid (row blocks, split, groups): (., s, z) sums the stages [s per, (s + 1) per) of iter_apply_plan(nt, n, .) -- apply_cross's
//   ranges -- against column group z.  Rows of x and R beyond n and columns beyond rp are staged as zeros.
//   Epilogue, split == 1 (every nt at which the row blocks fill the device): the 64 x 128 tile of u goes through the LDS the
//   sweep has left (pitch 129) and thread i < 64 adds its row's squares in ascending column order from 0: g[z][i].  split > 1
//   (few test points): the tile goes to part[s][i][c] and k_cov_var_finish adds the ranges in ascending order before it squares
//   -- at most ITER_SLOTS row blocks x ranges exist, so part is bounded by 64 ITER_SLOTS rp doubles whatever nt.
//   k_cov_var_finish adds the groups in ascending order.  No atomics; a point's bits depend on its own row, the plan and R only.
#pragma once

template <bool ARD, int KIND, int NCT>
__device__ __forceinline__ void cov_var_body(const double* __restrict__ A, int na, const double* __restrict__ B, int nb, int d,
                                             const HyperScalars* __restrict__ hd, const double* __restrict__ R, int rp,
                                             double* __restrict__ part, double* __restrict__ g, int per)
{
#pragma clang fp contract(off)
    constexpr int TP = NCT * 16, TPL = TP + 16, NK = ITER_JT / 4, UP = TP + 1;
    static_assert(ITER_JT * DC == 2 * 256 && ITER_JT * TP == 2 * 256 * NCT, "one d2 of x and NCT d2 of R per thread and stage");
    static_assert(ITER_ROWS * UP <= 2 * ITER_JT * TPL, "the tile of u fits the two images of R");
    __shared__ __attribute__((aligned(16))) double ys[2][ITER_JT][DC];
    __shared__ __attribute__((aligned(16))) double yc[ITER_JT][DC];
    __shared__ __attribute__((aligned(16))) double vs[2][ITER_JT][TPL];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fk = lane >> 4;
    const int row = blockIdx.x * ITER_ROWS + wave * 16 + fr, z0 = blockIdx.z * TP;
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
    // the thread's share of a stage: one feature pair of one x row, NCT column pairs of R's group
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
            const int e = tid + 256 * q, j = j0 + e / (TP / 2), c = z0 + 2 * (e % (TP / 2));
            rv[q] = (j < nb && c < rp) ? *(const d2*)(R + (size_t)j * rp + c) : (d2){0.0, 0.0};
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
    const int ib = blockIdx.x * ITER_ROWS;
    if (gridDim.y > 1) {                               // the range's share of u: k_cov_var_finish adds, squares and sums
        double* __restrict__ o = part + (size_t)blockIdx.y * na * rp;
#pragma unroll
        for (int ct = 0; ct < NCT; ct++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int i = ib + wave * 16 + fk + 4 * r, c = z0 + ct * 16 + fr;
                if (i < na && c < rp) o[(size_t)i * rp + c] = acc[ct][r];
            }
        return;
    }
    double* __restrict__ us = &vs[0][0][0];            // [ITER_ROWS][UP]: the sweep's last barrier has passed
#pragma unroll
    for (int ct = 0; ct < NCT; ct++)
#pragma unroll
        for (int r = 0; r < 4; r++) us[(wave * 16 + fk + 4 * r) * UP + ct * 16 + fr] = acc[ct][r];
    __syncthreads();
    if (tid < ITER_ROWS && ib + tid < na) {
        double s = 0.0;
        for (int c = 0; c < TP; c++) {
            const double u = us[tid * UP + c];
            s = s + u * u;
        }
        g[(size_t)blockIdx.z * na + ib + tid] = s;
    }
}

template <bool ARD, int KIND>
__global__ __launch_bounds__(256) void k_cov_var(const double* __restrict__ A, int na, const double* __restrict__ B, int nb, int d,
                                                 const HyperScalars* __restrict__ hd, const double* __restrict__ R, int rp,
                                                 double* __restrict__ part, double* __restrict__ g, int per)
{
    cov_var_body<ARD, KIND, VC_NCT>(A, na, B, nb, d, hd, R, rp, part, g, per);
}

void launch_cov_var(const double* Xt, int nt, const double* X, int n, int d, const CovFn& cf, const double* R, int rp, double* part,
                    double* g, double* sq, const IterPlan& pl, hipStream_t s)
{
    constexpr int GW = VC_NCT * 16;
    const int nz = (rp + GW - 1) / GW;
    assert(cf.hd && rp % 2 == 0 && (pl.split == 1 || part));
    hipLaunchKernelGGL(CUGP_COV_KERNEL(cf, k_cov_var), dim3(pl.row_blocks, pl.split, nz), dim3(256), 0, s, Xt, nt, X, n, d, cf.hd, R,
                       rp, part, g, pl.per);
    hipLaunchKernelGGL(k_cov_var_finish, dim3((nt + 255) / 256), dim3(256), 0, s, part, pl.split, g, nz, GW, nt, rp, sq);
}

// ---- the build's tall kernels ----

// Q[i][c0 + c] = W[i][c], c < cw: the block into its slot, where k_pc_project's Q'W holds its Gram matrix in rows c0 ...
__global__ __launch_bounds__(256) void k_vc_place(const double* __restrict__ W, double* __restrict__ Q, int rp, int c0, int cw, size_t cnt)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= cnt) return;
    const int c = (int)(e & 15);
    if (c < cw) Q[(e >> 4) * rp + c0 + c] = W[e];
}

// k_vc_scale:  out [n][16] = W Ti (Ti [16][16] upper triangular: T^-1 of a CholQR round, zero beyond the live columns), and the
//   first cw columns into Q's slot at c0.  A workgroup owns 64 rows, a wave 16: A[row fr][k fk] = W[i0 + fr][4 kk + fk] and
//   B[k fk][col fr] = Ti[4 kk + fk][fr] as they lie in memory (a wave's A reads: 16 rows of 128 B, contiguous), 4 MFMAs, k
//   ascending.  Rows beyond n enter as zeros and are not written.
__global__ __launch_bounds__(256) void k_vc_scale(const double* __restrict__ W, const double* __restrict__ Ti, double* __restrict__ out,
                                                  double* __restrict__ Q, int rp, int c0, int cw, int n)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fk = lane >> 4;
    const size_t i0 = (size_t)blockIdx.x * 64 + wave * 16;
    d4 acc = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int kk = 0; kk < 4; kk++) {
        const double a = i0 + fr < (size_t)n ? W[(i0 + fr) * 16 + kk * 4 + fk] : 0.0;
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Ti[(kk * 4 + fk) * 16 + fr], acc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const size_t i = i0 + fk + 4 * r;
        if (i < (size_t)n) {
            out[i * 16 + fr] = acc[r];
            if (fr < cw) Q[i * rp + c0 + fr] = acc[r];
        }
    }
}

// k_vc_rsolve:  R = Q L^-T, row by row of Q: R L' = Q.  A workgroup is ONE wave and owns 16 rows; it walks the 16-column groups
//   in ascending order.  Group g at c0 = 16 g: acc = R[:, 0 .. c0) L[c0 .. c0 + 16, 0 .. c0)' by MFMA -- A[row fr][k fk] out of the
//   LDS image rs of the rows' finished columns (pitch rp - 14: every column but the last group's, which nothing reads again),
//   B[k fk][col fr] = L[c0 + fr][4 kk + fk] from memory (every workgroup reads the same k x k factor: cache-resident), k
//   ascending -- then x = Q[:, c0 ..] - acc goes through a 16 x 17 tile and lane i < 16 solves its row against the diagonal block
//   by substitution in column order (x_c - sum_(m < c) r_m L[c0 + c][c0 + m]) / L[c0 + c][c0 + c].  No k x k inverse is formed.
//   Columns at and beyond VC_GOT are written as zeros; rows beyond n are not written.  LDS: 64.4 KiB at any rp <= 512 (two workgroups per CU).
__global__ __launch_bounds__(64) void k_vc_rsolve(const double* __restrict__ Q, const double* __restrict__ L, double* __restrict__ R,
                                                  int rp, int n, const int* __restrict__ ctl)
{
#pragma clang fp contract(off)
    constexpr int PITCH = PCH_MAX_RANK - 14;
    __shared__ double rs[16][PITCH];
    __shared__ double xt[16][17];
    const int lane = threadIdx.x, fr = lane & 15, fk = lane >> 4;
    const size_t i0 = (size_t)blockIdx.x * 16;
    const int got = ctl[VC_GOT];
    for (int c0 = 0; c0 < rp; c0 += 16) {
        d4 acc = (d4){0.0, 0.0, 0.0, 0.0};
        if (c0 < got)
            for (int k = 0; k < c0; k += 4)
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(rs[fr][k + fk], L[(size_t)(c0 + fr) * rp + k + fk], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const size_t i = i0 + fk + 4 * r;
            xt[fk + 4 * r][fr] = (i < (size_t)n && c0 + fr < got) ? Q[i * rp + c0 + fr] - acc[r] : 0.0;
        }
        __syncthreads();
        if (lane < 16 && c0 < got) {
            double rr[16];
#pragma unroll
            for (int c = 0; c < 16; c++) {
                double v = xt[lane][c];
                if (c0 + c < got) {
                    const double* __restrict__ lc = L + (size_t)(c0 + c) * rp + c0;
#pragma unroll
                    for (int m = 0; m < c; m++) v = v - rr[m] * lc[m];
                    v = v / lc[c];
                }
                rr[c] = v;
                xt[lane][c] = v;
            }
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const size_t i = i0 + fk + 4 * r;
            const double v = xt[fk + 4 * r][fr];
            if (c0 + 16 < rp) rs[fk + 4 * r][c0 + fr] = v;
            if (i < (size_t)n) R[i * rp + c0 + fr] = v;
        }
        __syncthreads();
    }
}

void launch_vc_init(int* ctl, hipStream_t s) { hipLaunchKernelGGL(k_vc_init, dim3(1), dim3(64), 0, s, ctl); }
void launch_vc_place(const double* W, double* Q, int rp, int c0, int cw, int n, hipStream_t s)
{
    const size_t cnt = (size_t)n * 16;
    hipLaunchKernelGGL(k_vc_place, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, s, W, Q, rp, c0, cw, cnt);
}
void launch_vc_hacc(const double* C, double* Hc, int rp, int first, int* ctl, hipStream_t s)
{
    hipLaunchKernelGGL(k_vc_hacc, dim3((rp * 16 + 255) / 256), dim3(256), 0, s, C, Hc, rp * 16, first, ctl);
}
void launch_vc_factor(const double* C, int c0, int cw, int mode, int record, const double* nrm0, double* Ti, const double* Hc,
                      double* H, int rp, int c0p, int* ctl, hipStream_t s)
{
    assert(cw >= 0 && cw <= 16 && c0 + cw <= rp);
    hipLaunchKernelGGL(k_vc_factor, dim3(1), dim3(256), 0, s, C, c0, cw, mode, record, nrm0, Ti, Hc, H, rp, c0p, ctl);
}
void launch_vc_scale(const double* W, const double* Ti, double* out, double* Q, int rp, int c0, int cw, int n, hipStream_t s)
{
    assert(c0 + cw <= rp);
    hipLaunchKernelGGL(k_vc_scale, dim3((unsigned)(((size_t)n + 63) / 64)), dim3(256), 0, s, W, Ti, out, Q, rp, c0, cw, n);
}
void launch_vc_finish(const double* H, double* S, const double* Q, double* R, int rp, int bw, int n, int* ctl, hipStream_t s)
{
    assert(rp % 64 == 0 && rp <= PCH_MAX_RANK);
    hipLaunchKernelGGL(k_vc_hsym, dim3((rp * rp + 255) / 256), dim3(256), 0, s, H, S, rp, bw, ctl);
    hipLaunchKernelGGL(k_vc_chol, dim3(1), dim3(256), 0, s, S, rp, ctl);
    hipLaunchKernelGGL(k_vc_rsolve, dim3((unsigned)(((size_t)n + 15) / 16)), dim3(64), 0, s, Q, S, R, rp, n, ctl);
}
