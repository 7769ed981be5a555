// eval_gfx950.h -- one evaluation of the log-likelihood and its gradient around the factorisation: the covariance build
// (k_build) and the cross covariance (k_cross, which the prediction and the sparse model launch too), the triangular
// matrix-vector passes and the blocked forward substitution (k_trmv_*, k_copy_y_to_w, k_trsv_*), the gradient traces
// (trace_body, k_trace) and the final sums (finalize_sums, k_finalize, k_finalize_ard); each launcher directly behind
// its kernel.
//
// Include-point contract.  Needs the device; also holds launchers.  Included by kernels.hip alone, INSIDE namespace cugp,
// after these are declared -- the file includes nothing and declares none of them:
//   kernels.h        TILE, HyperScalars, CovFn, ExpertPtrs, Batch, ticket_count, ARD_ROW_GRAD, tune and the TUNE_* keys,
//                    the launcher prototypes
//   kernels.hip      d2, GP, LaunchStamp, take_stamp, tri_count, is_ard, CUGP_COV_KERNEL
//   cov_device.h     tri_index, wave_sum, KT, DC, col4, sqdist_4x4, DivBy, div_prepare, div_by, ard_weights, matern_entry,
//                    kernel_value, TGT_CHUNK, targets_outer_4x4, trace_ard_body
// Declares for dense_features_gfx950.h: FIN_THREADS, FinalizeArgs, trace_body (k_trace_targets is its TARGETS form).
#pragma once

// SE covariance build: 64x64 tile per 256-thread workgroup, 4x4 outputs per thread, X tiles in LDS
// (the tile geometry KT, DC, col4, the squared distances and the per-entry formulas: cov_device.h)
// The passes that evaluate the covariance function are ONE kernel template each, k_<pass><ARD, KIND>, with one argument
// list: the hyper-scalars by value (h) and in device memory (hd).  Isotropic: hd is optional -- when given it is read
// INSTEAD of h, so that a captured graph of the evaluation is replayed with new hyper-parameters by refreshing that one
// buffer instead of every kernel's arguments (build and trace; the other passes take h).  ARD: hd is mandatory, h is
// ignored, the d per-dimension weights lie behind the hyper-scalars and ell_sq is not read: K = sf2 exp(-acc / 2) (or the
// Matern entry) of the weighted squared distance, no division.  cov_kernel (at the launchers) maps a CovFn to the instantiation.
//
// k_build: lower 64x64 tiles of K (+ mirror when full == 1); full == 2 (isotropic SE only): the squared-distance
// intermediate of launch_sqdist.  Batched experts, ticket zeroing, device-resident hyper-scalars and stamps in every
// instantiation.
template <bool ARD, int KIND>
__device__ __forceinline__ void build_body(const double* __restrict__ X, int n, int d, int npad,
                                           HyperScalars h_arg, const HyperScalars* __restrict__ hd,
                                           double* __restrict__ K, int full, unsigned* __restrict__ tickets,
                                           const ExpertPtrs* __restrict__ bt, unsigned long long* stamp)
{
    LaunchStamp stamp_(stamp, 16);
    if (bt) {
        X = GP(bt[blockIdx.y].X); n = bt[blockIdx.y].n; K = GP(bt[blockIdx.y].A);
        if (tickets) tickets = GP(bt[blockIdx.y].tickets);
    }
    // tickets (when given): the factorisation's per-step arrival counters, zeroed here instead of by a memset node in
    // front of the factorisation (one launch boundary less on a chain that small matrices are bound by)
    // (2 per tile row: [0, nt) the step tickets of k_syrk_step, [nt, 2 nt) the stage counters of k_trtri_block; [2 nt]: the
    //  arrival counter of k_trace's fused finalize)
    if (tickets && blockIdx.x == 0)
        for (int i = threadIdx.x; i < ticket_count(npad / TILE); i += 256) tickets[i] = 0u;
    const HyperScalars h = (ARD || hd) ? *hd : h_arg;
    __shared__ double xs[KT][DC + 1], ys[KT][DC + 1];
    __shared__ double ws[DC];
    int ti, tj;
    tri_index(blockIdx.x, ti, tj);
    const int i0 = ti * KT, j0 = tj * KT;
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    double d2v[4][4];
    sqdist_4x4<ARD>(X, X, n, n, d, i0, j0, xs, ys, d2v, ARD ? ard_weights(hd) : nullptr, ws);
    double out[4][4];
    const DivBy dl = div_prepare(h.ell_sq);
    const ShapeArgs sh = shape_args<KIND>(ARD ? ard_weights(hd) : nullptr, d);
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const int i = i0 + ty * 4 + a, j = j0 + col4(tx, b);
            const bool in = i < n && j < n;
            double v;
            if (!ARD && full == 2) {
                v = (i == j) ? 0.0 : div_by(d2v[a][b], dl);    // covkernel.cpp:143-151 (squared distance / c)
            } else {
                v = kernel_value<ARD, KIND>(d2v[a][b], dl, h.signal_var, sh);   // covkernel.cpp:89
                if (i == j) v += h.noise_var;                            // covkernel.cpp:93-94
            }
            out[a][b] = in ? v : ((i == j) ? 1.0 : 0.0);                // identity padding
        }
#pragma unroll
    for (int a = 0; a < 4; a++) {
        double* p = K + (size_t)(i0 + ty * 4 + a) * npad + j0 + tx * 2;
        *(d2*)p = (d2){out[a][0], out[a][1]};
        *(d2*)(p + 32) = (d2){out[a][2], out[a][3]};
    }
    if (full && ti != tj) {
#pragma unroll
        for (int b = 0; b < 4; b++) {
            double* p = K + (size_t)(j0 + col4(tx, b)) * npad + i0 + ty * 4;
            *(d2*)p = (d2){out[0][b], out[1][b]};
            *(d2*)(p + 2) = (d2){out[2][b], out[3][b]};
        }
    }
}

template <bool ARD, int KIND>
__global__ __launch_bounds__(256) void k_build(const double* __restrict__ X, int n, int d, int npad,
                                               HyperScalars h_arg, const HyperScalars* __restrict__ hd,
                                               double* __restrict__ K, int full, unsigned* __restrict__ tickets,
                                               const ExpertPtrs* __restrict__ bt, unsigned long long* stamp)
{
    build_body<ARD, KIND>(X, n, d, npad, h_arg, hd, K, full, tickets, bt, stamp);
}

void launch_kbuild(const double* X, int n, int d, int npad, const CovFn& cf, double* K, bool full, hipStream_t s,
                   Batch bt, unsigned* tickets)
{
    const dim3 grid(tri_count(npad / KT), bt.count);
    hipLaunchKernelGGL(CUGP_COV_KERNEL(cf, k_build), grid, dim3(256), 0, s, X, n, d, npad, cf.h, cf.hd, K, full ? 1 : 0,
                       tickets, bt.tab, take_stamp());
}

void launch_sqdist(const double* X, int n, int d, int npad, double c, double* S, hipStream_t s)
{
    HyperScalars h{c, 0.0, 0.0};
    hipLaunchKernelGGL((k_build<false, KERNEL_SE>), dim3(tri_count(npad / KT)), dim3(256), 0, s, X, n, d, npad, h,
                       (const HyperScalars*)nullptr, S, 2, (unsigned*)nullptr, (const ExpertPtrs*)nullptr,
                       (unsigned long long*)nullptr);
}

// k_cross: Ks[t][i] = k(xt_t, x_i) (no noise, covkernel.cpp:105-116); zero padding
// bt (batched): blockIdx.y selects the expert -- X, n from its table entry, Ks = the expert's [ntpad][npad] slice
template <bool ARD, int KIND>
__device__ __forceinline__ void cross_body(const double* __restrict__ X, int n, int d, int npad,
                                           const double* __restrict__ Xt, int nt, int ntpad, const HyperScalars& h,
                                           const double* __restrict__ wts,
                                           double* __restrict__ Ks, const ExpertPtrs* __restrict__ bt)
{
    if (bt) {
        X = GP(bt[blockIdx.y].X); n = bt[blockIdx.y].n;
        Ks += (size_t)blockIdx.y * ntpad * npad;
    }
    __shared__ double xs[KT][DC + 1], ys[KT][DC + 1];
    const int tiles_i = npad / KT;
    const int tt = blockIdx.x / tiles_i, ti = blockIdx.x % tiles_i;
    const int t0 = tt * KT, i0 = ti * KT;
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    double d2v[4][4];
    // the reference subtracts X[i] - xtest (covkernel.cpp:112); squares are sign-independent but keep the order
    __shared__ double ws[DC];
    sqdist_4x4<ARD>(Xt, X, nt, n, d, t0, i0, xs, ys, d2v, wts, ws);
    const DivBy dl = div_prepare(h.ell_sq);
    const ShapeArgs sh = shape_args<KIND>(wts, d);
#pragma unroll
    for (int a = 0; a < 4; a++) {
        const int tr = t0 + ty * 4 + a;
        double o[4];
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const int i = i0 + col4(tx, b);
            o[b] = (tr < nt && i < n) ? kernel_value<ARD, KIND>(d2v[a][b], dl, h.signal_var, sh) : 0.0;
        }
        double* p = Ks + (size_t)tr * npad + i0 + tx * 2;
        *(d2*)p = (d2){o[0], o[1]};
        *(d2*)(p + 32) = (d2){o[2], o[3]};
    }
}

template <bool ARD, int KIND>
__global__ __launch_bounds__(256) void k_cross(const double* __restrict__ X, int n, int d, int npad,
                                               const double* __restrict__ Xt, int nt, int ntpad, HyperScalars h_arg,
                                               double* __restrict__ Ks, const ExpertPtrs* __restrict__ bt,
                                               const HyperScalars* __restrict__ hd)
{
    cross_body<ARD, KIND>(X, n, d, npad, Xt, nt, ntpad, ARD ? *hd : h_arg, ARD ? ard_weights(hd) : nullptr, Ks, bt);
}

void launch_kcross(const double* X, int n, int d, int npad, const double* Xt, int nt, int ntpad, const CovFn& cf,
                   double* Ks, hipStream_t s, Batch bt)
{
    const dim3 grid((ntpad / KT) * (npad / KT), bt.count);
    hipLaunchKernelGGL(CUGP_COV_KERNEL(cf, k_cross), grid, dim3(256), 0, s, X, n, d, npad, Xt, nt, ntpad, cf.h, Ks,
                       bt.tab, cf.hd);
}

// z[i] = sum_{k < (ti+1)*128} T[i][k] x[k]  (one wave per row; the diagonal tile is zero above the diagonal)
__global__ __launch_bounds__(256) void k_trmv_lower(const double* __restrict__ T, int ld, int npad,
                                                    const double* __restrict__ x, double* __restrict__ z,
                                                    const ExpertPtrs* __restrict__ bt)
{
    if (bt) { T = GP(bt[blockIdx.y].T); x = GP(bt[blockIdx.y].y); z = GP(bt[blockIdx.y].z); }
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= npad) return;
    const int kend = (row / TILE + 1) * TILE;
    const double* tr = T + (size_t)row * ld;
    double s = 0.0;
    for (int k = lane * 2; k < kend; k += 128) {
        d2 v = *(const d2*)(tr + k), xv = *(const d2*)(x + k);
        s += v[0] * xv[0] + v[1] * xv[1];
    }
    s = wave_sum(s);
    if (lane == 0) z[row] = s;
}

void launch_trmv_lower(const double* T, int ld, int npad, const double* x, double* z, hipStream_t s, Batch bt)
{
    hipLaunchKernelGGL(k_trmv_lower, dim3(npad / 4, bt.count), dim3(256), 0, s, T, ld, npad, x, z, bt.tab);
}

// a[i] = sum_{k >= ti*128} U[i][k] x[k]
__global__ __launch_bounds__(256) void k_trmv_upper(const double* __restrict__ U, int ld, int npad,
                                                    const double* __restrict__ x, double* __restrict__ a,
                                                    const ExpertPtrs* __restrict__ bt)
{
    if (bt) { U = GP(bt[blockIdx.y].U); x = GP(bt[blockIdx.y].z); a = GP(bt[blockIdx.y].alpha); }
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= npad) return;
    const int kbeg = (row / TILE) * TILE;
    const double* ur = U + (size_t)row * ld;
    double s = 0.0;
    for (int k = kbeg + lane * 2; k < npad; k += 128) {
        d2 v = *(const d2*)(ur + k), xv = *(const d2*)(x + k);
        s += v[0] * xv[0] + v[1] * xv[1];
    }
    s = wave_sum(s);
    if (lane == 0) a[row] = s;
}

void launch_trmv_upper(const double* U, int ld, int npad, const double* x, double* a, hipStream_t s, Batch bt)
{
    hipLaunchKernelGGL(k_trmv_upper, dim3(npad / 4, bt.count), dim3(256), 0, s, U, ld, npad, x, a, bt.tab);
}

// w = y for every expert of a batched launch (the forward substitution consumes w)
__global__ __launch_bounds__(256) void k_copy_y_to_w(int npad, const ExpertPtrs* __restrict__ bt)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < npad) GP(bt[blockIdx.y].w)[i] = GP(bt[blockIdx.y].y)[i];
}

void launch_copy_y_to_w(int npad, hipStream_t s, Batch bt)
{
    hipLaunchKernelGGL(k_copy_y_to_w, dim3((npad + 255) / 256, bt.count), dim3(256), 0, s, npad, bt.tab);
}

// blocked forward substitution L z = y (LL-only path): step kb = (1) z_kb = T_kk w_kb, (2) w[rows below] -= L21 z_kb
__global__ __launch_bounds__(256) void k_trsv_diag(const double* __restrict__ T, int ld, int kb,
                                                   const double* __restrict__ w, double* __restrict__ z,
                                                   const ExpertPtrs* __restrict__ bt)
{
    if (bt) { T = GP(bt[blockIdx.y].T); w = GP(bt[blockIdx.y].w); z = GP(bt[blockIdx.y].z); }
    // z_kb = T_kk w_kb (128x128, lower): two threads per row, 64 columns each, 16-byte loads
    __shared__ double ws[TILE];
    const int k0 = kb * TILE, t = threadIdx.x;
    if (t < TILE) ws[t] = w[k0 + t];
    __syncthreads();
    const int r = t >> 1, h = t & 1;
    const double* tr = T + (size_t)(k0 + r) * ld + k0 + h * 64;
    double s0 = 0.0, s1 = 0.0;
#pragma unroll 8
    for (int c = 0; c < 64; c += 2) {
        const d2 v = *(const d2*)(tr + c);
        s0 = __builtin_fma(v[0], ws[h * 64 + c], s0);
        s1 = __builtin_fma(v[1], ws[h * 64 + c + 1], s1);
    }
    double sum = s0 + s1;
    sum += __shfl_xor(sum, 1, 64);
    if (h == 0) z[k0 + r] = sum;
}

__global__ __launch_bounds__(256) void k_trsv_update(const double* __restrict__ A, int ld, int kb, int npad,
                                                     const double* __restrict__ z, double* __restrict__ w,
                                                     const ExpertPtrs* __restrict__ bt)
{
    if (bt) { A = GP(bt[blockIdx.y].A); z = GP(bt[blockIdx.y].z); w = GP(bt[blockIdx.y].w); }
    const int k0 = kb * TILE;
    const int row = k0 + TILE + blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= npad) return;
    const double* ar = A + (size_t)row * ld + k0;
    d2 v = *(const d2*)(ar + lane * 2), xv = *(const d2*)(z + k0 + lane * 2);
    double s = wave_sum(v[0] * xv[0] + v[1] * xv[1]);
    if (lane == 0) w[row] -= s;
}

void launch_trsv_lower(const double* A, const double* T, int ld, int nt, const double* y, double* z, hipStream_t s,
                       Batch bt)
{
    // y is consumed as the running right-hand side w (caller passes a scratch copy)
    double* w = const_cast<double*>(y);
    const int npad = nt * TILE;
    for (int kb = 0; kb < nt; kb++) {
        hipLaunchKernelGGL(k_trsv_diag, dim3(1, bt.count), dim3(256), 0, s, T, ld, kb, w, z, bt.tab);
        const int rows = npad - (kb + 1) * TILE;
        if (rows > 0)
            hipLaunchKernelGGL(k_trsv_update, dim3(rows / 4, bt.count), dim3(256), 0, s, A, ld, kb, npad, z, w, bt.tab);
    }
}

// Final sums of an evaluation by ONE workgroup of NTHR threads, in the order 1024 threads would take them whatever NTHR
// is (so the stand-alone k_finalize, 1024 threads, and the last block of k_trace, 256 threads, give the same bits):
// virtual thread v = 0..1023 sums the entries i = v, v + 1024, ... ascending, then the halving tree red[v] += red[v + w],
// w = 512 .. 1.  A real thread takes the virtual threads t, t + NTHR, ... and the tree levels above NTHR in registers.
// HANDED: the trace partials were written by other workgroups of this launch -- agent-scope loads.
// red: 5 * NTHR / ... doubles of LDS: [5][NTHR].
constexpr int FIN_THREADS = 1024;     // one workgroup; at N = 8192 it sums 3 x 8256 trace partials and 8192 squares (23 us with 256 threads)
template <int NTHR, bool HANDED>
__device__ __forceinline__ void finalize_sums(const double* __restrict__ z, int npad, int n,
                                              const double* __restrict__ logdet_part, int nt,
                                              const double* __restrict__ part, int nblocks, HyperScalars h,
                                              double* __restrict__ out, double* __restrict__ hout, double* red)
{
    constexpr int V = FIN_THREADS / NTHR;              // virtual threads per real thread
    const int t = threadIdx.x;
    double acc[5][V];
#pragma unroll
    for (int j = 0; j < V; j++) {
        const int v = t + j * NTHR;
        double q = 0.0, ld = 0.0, s0 = 0.0, s1 = 0.0, s2 = 0.0;
        for (int i = v; i < npad; i += FIN_THREADS) q += z[i] * z[i];
        for (int i = v; i < nt; i += FIN_THREADS) ld += logdet_part[i];
        if (part)
            for (int i0 = v; i0 < nblocks; i0 += 4 * FIN_THREADS) {
                // four entries' loads in flight before the first is added (agent-scope loads one by one cost a memory
                // latency each: 40 us for the 8256 partials of an 8192-row matrix); the sums are taken in order
                double p[4][3];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int i = i0 + u * FIN_THREADS;
                    const double* pp = part + (size_t)(i < nblocks ? i : v) * 3;
#pragma unroll
                    for (int c = 0; c < 3; c++)
                        p[u][c] = HANDED ? __hip_atomic_load(pp + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : pp[c];
                }
#pragma unroll
                for (int u = 0; u < 4; u++)
                    if (i0 + u * FIN_THREADS < nblocks) { s0 += p[u][0]; s1 += p[u][1]; s2 += p[u][2]; }
            }
        acc[0][j] = q; acc[1][j] = ld; acc[2][j] = s0; acc[3][j] = s1; acc[4][j] = s2;
    }
    // tree levels w >= NTHR: red[v] += red[v + w] pairs virtual threads of the SAME real thread (v and v + w differ by a multiple of NTHR)
#pragma unroll
    for (int w = V / 2; w > 0; w >>= 1)
#pragma unroll
        for (int c = 0; c < 5; c++)
#pragma unroll
            for (int j = 0; j < w; j++) acc[c][j] += acc[c][j + w];
    __syncthreads();                                   // (red may alias LDS the caller used before)
#pragma unroll
    for (int c = 0; c < 5; c++) red[c * NTHR + t] = acc[c][0];
    __syncthreads();
    for (int w = NTHR / 2; w > 0; w >>= 1) {
        if (t < w)
            for (int c = 0; c < 5; c++) red[c * NTHR + t] += red[c * NTHR + t + w];
        __syncthreads();
    }
    if (t == 0) {
        const double quad = red[0], logdet = 2 * red[NTHR];
        out[0] = -0.5 * (quad + logdet + n * 1.83787);
        if (part) {
            const double s1 = red[2 * NTHR], s2 = red[3 * NTHR], s3 = red[4 * NTHR];
            out[1] = s1 / 2.0;
            out[2] = (2.0 * s2 - 2.0 * h.noise_var * s3) / 2.0;
            out[3] = (2.0 * h.noise_var * s3) / 2.0;
        }
        out[4] = quad;
        out[5] = logdet;
        if (hout)
            for (int i = 0; i < 6; i++) hout[i] = out[i];
    }
}

// what the last block of k_trace needs to finish the evaluation (out == nullptr: no fused finalize)
struct FinalizeArgs {
    const double* z; const double* logdet_part; int nt; double* out; double* hout; unsigned* ticket;
};

// gradient traces, fused: for every lower 64x64 tile recompute k(xi,xj) and |xi-xj|^2/l^2, read K^-1 once,
// W = K^-1 - alpha alpha^T, accumulate  s1 = sum W*K*S, s2 = sum W*K, s3 = sum_i W_ii  (off-diagonal tiles x2)
// KIND: s1 is sum W o dK/dlog l -- SE's K o S, or a Matern kind's dk of matern_entry (one exp(-a) for k and dk; zero on
// the diagonal, where a = 0); s2, s3 and everything behind the sums keep their meaning
// TARGETS (multi-target regression, k_trace_targets): the same tile, thread layout, entry formulas, doubling of the
// off-diagonal entries, diagonal handling and partial sums (part[3 * block + c]) with W = m K^-1 - sum_t alpha_t alpha_t^T
// from the target-major AV ([m][npad]) in place of K^-1 - alpha alpha^T.  K^-1 is read once whatever m is; no N x N
// intermediate is written.  Single handle, h by value, always the separate final sums (bt, hd and fin.out null).
template <int KIND, bool TARGETS>
__device__ __forceinline__ void trace_body(const double* __restrict__ X, int n, int d, int npad,
                                           HyperScalars h_arg, const HyperScalars* __restrict__ hd,
                                           const double* __restrict__ Kinv, const double* __restrict__ AV, int m,
                                           double* __restrict__ part, const ExpertPtrs* __restrict__ bt,
                                           FinalizeArgs fin)
{
    if (!TARGETS && bt) {
        const ExpertPtrs& e = bt[blockIdx.y];
        X = GP(e.X); n = e.n; Kinv = GP(e.Kinv); AV = GP(e.alpha); part = GP(e.part);
        if (fin.out) {
            fin.z = GP(e.z); fin.logdet_part = GP(e.logdet); fin.out = GP(e.out); fin.ticket = GP(e.tickets) + 2 * fin.nt;
            if (fin.hout) fin.hout += (size_t)blockIdx.y * 8;
        }
    }
    const HyperScalars h = hd ? *hd : h_arg;
    // (one buffer: the two X tiles of the squared distances, later the [5][256] sums of the fused finalize)
    __shared__ double lds[2 * KT * (DC + 1)];
    static_assert(2 * KT * (DC + 1) >= 5 * 256, "the fused finalize reduces in the X tiles' LDS");
    double (&xs)[KT][DC + 1] = *reinterpret_cast<double (*)[KT][DC + 1]>(lds);
    double (&ys)[KT][DC + 1] = *reinterpret_cast<double (*)[KT][DC + 1]>(lds + KT * (DC + 1));
    __shared__ double red[3][4];
    int ti, tj;
    tri_index(blockIdx.x, ti, tj);
    const int i0 = ti * KT, j0 = tj * KT;
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    double d2v[4][4], S[4][4];
    sqdist_4x4(X, X, n, n, d, i0, j0, xs, ys, d2v);
    if constexpr (TARGETS) {
        __shared__ __attribute__((aligned(16))) double la[TGT_CHUNK][KT], lb[TGT_CHUNK][KT];
        targets_outer_4x4(AV, npad, m, i0, j0, la, lb, S);
    }
    double s1 = 0.0, s2 = 0.0, s3 = 0.0;
    const DivBy dl = div_prepare(h.ell_sq);
    const double dm = (double)m;
    double aj[4];
    if constexpr (!TARGETS) {
#pragma unroll
        for (int b = 0; b < 4; b++) aj[b] = AV[j0 + col4(tx, b)];
    }
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
            if (i < n && j < n && (ti != tj || j <= i)) {
                double w;
                if constexpr (TARGETS) w = dm * kv[b] - S[a][b];
                else w = kv[b] - ai * aj[b];
                if constexpr (KIND == KERNEL_SE) {
                    double kse = h.signal_var * exp(div_by(-d2v[a][b] * 0.5, dl));
                    const double sd = div_by(d2v[a][b], dl);
                    if (i == j) {
                        kse += h.noise_var;
                        s1 += w * (kse * sd);
                        s2 += w * kse;
                        s3 += w;
                    } else {
                        s1 += 2.0 * (w * (kse * sd));
                        s2 += 2.0 * (w * kse);
                    }
                } else {
                    double kf, dk, hh;
                    matern_entry<KIND>(div_by(d2v[a][b], dl), h.signal_var, kf, dk, hh);
                    if (i == j) {
                        kf += h.noise_var;
                        s1 += w * dk;
                        s2 += w * kf;
                        s3 += w;
                    } else {
                        s1 += 2.0 * (w * dk);
                        s2 += 2.0 * (w * kf);
                    }
                }
            }
        }
    }
    s1 = wave_sum(s1); s2 = wave_sum(s2); s3 = wave_sum(s3);
    if ((t & 63) == 0) { red[0][t >> 6] = s1; red[1][t >> 6] = s2; red[2][t >> 6] = s3; }
    __syncthreads();
    if (!fin.out) {
        if (t < 3) part[(size_t)blockIdx.x * 3 + t] = (red[t][0] + red[t][1]) + (red[t][2] + red[t][3]);
        return;
    }
    // Fused finalize (round 6): the partial sums leave write-through, the block draws a ticket, and the LAST block of the
    // launch (of this expert) goes on to the final sums and the scalar formulas -- what k_finalize did as one more launch
    // behind this one (a kernel boundary and a 1-workgroup launch on the serial tail of every evaluation: ~9 us of a
    // 590-us evaluation at 1500 rows).  The hand-off is the step kernel's (k_syrk_step): write-through (agent-scope)
    // stores by lanes of wave 0, that wave's vmcnt(0), one relaxed agent-scope ticket; the last arriver reads every
    // partial with agent-scope loads.  Same sums in the same order as k_finalize: identical bits.
    __shared__ unsigned s_ticket;
    if (t < 3) __hip_atomic_store(part + (size_t)blockIdx.x * 3 + t, (red[t][0] + red[t][1]) + (red[t][2] + red[t][3]),
                                  __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (t < 64) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (t == 0) s_ticket = __hip_atomic_fetch_add(fin.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (s_ticket != gridDim.x - 1) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (t == 0) *fin.ticket = 0u;                          // (ready for the next evaluation; nobody else touches it any more)
    finalize_sums<256, true>(fin.z, npad, n, fin.logdet_part, fin.nt, part, (int)gridDim.x, h, fin.out, fin.hout, lds);
}

// single workgroup: deterministic final sums and the scalar formulas
//   LL = -0.5 (z'z + 2 sum log L_ii + n * 1.83787)                     covkernel.cpp:127
//   g0 = s1/2, g1 = (2 s2 - 2 sn2 s3)/2, g2 = (2 sn2 s3)/2              covkernel.cpp:244-261
__global__ __launch_bounds__(FIN_THREADS) void k_finalize(const double* __restrict__ z, int npad, int n,
                                                  const double* __restrict__ logdet_part, int nt,
                                                  const double* __restrict__ part, int nblocks,
                                                  HyperScalars h_arg, const HyperScalars* __restrict__ hd,
                                                  double* __restrict__ out, double* __restrict__ hout,
                                                  const ExpertPtrs* __restrict__ bt)
{
    // hout: the same 6 results straight into the caller's pinned host buffer ([expert][8]) -- visible to the host
    // when the launch has completed, no copy node (and its ~10-us boundary) behind the evaluation
    if (bt) {
        const ExpertPtrs& e = bt[blockIdx.y];
        z = GP(e.z); n = e.n; logdet_part = GP(e.logdet); out = GP(e.out);
        if (part) part = GP(e.part);
        if (hout) hout += (size_t)blockIdx.y * 8;
    }
    const HyperScalars h = hd ? *hd : h_arg;
    __shared__ double red[5 * FIN_THREADS];
    finalize_sums<FIN_THREADS, false>(z, npad, n, logdet_part, nt, part, nblocks, h, out, hout, red);
}

void launch_finalize(const double* z, int npad, int n, const double* logdet_part, int nt, const double* part,
                     int nblocks, HyperScalars h, double* out, double* hout, hipStream_t s, const HyperScalars* hd,
                     Batch bt)
{
    hipLaunchKernelGGL(k_finalize, dim3(1, bt.count), dim3(FIN_THREADS), 0, s, z, npad, n, logdet_part, nt, part, nblocks, h,
                       hd, out, hout, bt.tab);
}

// k_trace: the gradient pass of a single-target evaluation.  ARD (trace_ard_body: cov_device.h): always followed by
// k_finalize_ard (fin is not read).
template <bool ARD, int KIND>
__global__ __launch_bounds__(256) void k_trace(const double* __restrict__ X, int n, int d, int npad,
                                               HyperScalars h_arg, const HyperScalars* __restrict__ hd,
                                               const double* __restrict__ Kinv, const double* __restrict__ alpha,
                                               double* __restrict__ part, const ExpertPtrs* __restrict__ bt,
                                               FinalizeArgs fin)
{
    if constexpr (ARD) trace_ard_body<KIND, false>(X, n, d, npad, hd, Kinv, alpha, 1, part, bt);
    else trace_body<KIND, false>(X, n, d, npad, h_arg, hd, Kinv, alpha, 1, part, bt, fin);
}

// Final sums of an ARD gradient evaluation, one workgroup.  LL, y'K^-1y and log|K| by finalize_sums (the isotropic
// order and bits); then wave w takes the columns w, w + 16, ... of the trace partials: lane l adds the blocks l, l + 64,
// ... ascending, the lanes by wave_sum -- a fixed order whatever the timing.  Results row (out, hout): [0] LL, [4] quad,
// [5] log|K|, [6] status word, [8 + c] the d + 2 gradient components (d: the columns
// with g_c = S_c / 2 -- a family's shape columns, RQ's one, count with the length columns: the launcher passes d + 1):
//   g_c = S_c / 2 (c < d), g_d = (2 s2 - 2 sn2 s3) / 2, g_{d+1} = (2 sn2 s3) / 2   (the last two as k_finalize's g1, g2)
// bt (batched): grid (1, experts) -- z, n, logdet_part, part and out from the expert's table entry, hout + expert * hstride
__global__ __launch_bounds__(FIN_THREADS) void k_finalize_ard(const double* __restrict__ z, int npad, int n, int d,
                                                              const double* __restrict__ logdet_part, int nt,
                                                              const double* __restrict__ part, int nblocks,
                                                              const HyperScalars* __restrict__ hd,
                                                              double* __restrict__ out, double* __restrict__ hout,
                                                              size_t hstride, const ExpertPtrs* __restrict__ bt)
{
    if (bt) {
        const ExpertPtrs& e = bt[blockIdx.y];
        z = GP(e.z); n = e.n; logdet_part = GP(e.logdet); part = GP(e.part); out = GP(e.out);
        hout += (size_t)blockIdx.y * hstride;
    }
    const HyperScalars h = *hd;
    __shared__ double red[5 * FIN_THREADS];
    finalize_sums<FIN_THREADS, false>(z, npad, n, logdet_part, nt, nullptr, 0, h, out, hout, red);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    for (int c = wave; c < d + 2; c += FIN_THREADS / 64) {
        const double* col = part + (size_t)c * nblocks;
        double s = 0.0;
        for (int i = lane; i < nblocks; i += 64) s += col[i];
        s = wave_sum(s);
        if (lane == 0 && c < d) { out[8 + c] = s / 2.0; hout[8 + c] = s / 2.0; }
        if (lane == 0 && c >= d) red[16 + (c - d)] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double s2 = red[16], s3 = red[17];
        const double gf = (2.0 * s2 - 2.0 * h.noise_var * s3) / 2.0, gn = (2.0 * h.noise_var * s3) / 2.0;
        out[8 + d] = gf; out[9 + d] = gn;
        hout[8 + d] = gf; hout[9 + d] = gn;
    }
}

// The same for a handle whose d length columns belong to ONE tied length scale (nh = nl - d + 3; nl: length and shape
// columns).  Every column is summed as above -- wave w takes the columns w, w + 16, ..., lane l the blocks l, l + 64, ... --
// TIED_COLS of them at a time into LDS; thread 0 then adds the d length columns' finished results S_c / 2 in index order
// into g_0 (the chain rule at equal scales, and bit for bit the index-order sum of the untied handle's components); the
// remaining columns' results move up to g_1 ...  The lines are k_finalize_ard's, repeated rather than shared through a
// function, so that the kernel that exists keeps its instructions.
constexpr int TIED_COLS = 1024;
__global__ __launch_bounds__(FIN_THREADS) void k_finalize_ard_tied(const double* __restrict__ z, int npad, int n, int nl,
                                                                   int d, const double* __restrict__ logdet_part, int nt,
                                                                   const double* __restrict__ part, int nblocks,
                                                                   const HyperScalars* __restrict__ hd,
                                                                   double* __restrict__ out, double* __restrict__ hout,
                                                                   size_t hstride, const ExpertPtrs* __restrict__ bt)
{
    if (bt) {
        const ExpertPtrs& e = bt[blockIdx.y];
        z = GP(e.z); n = e.n; logdet_part = GP(e.logdet); part = GP(e.part); out = GP(e.out);
        hout += (size_t)blockIdx.y * hstride;
    }
    const HyperScalars h = *hd;
    __shared__ double red[5 * FIN_THREADS];
    static_assert(TIED_COLS <= 5 * FIN_THREADS, "the columns' sums reuse the final sums' LDS");
    finalize_sums<FIN_THREADS, false>(z, npad, n, logdet_part, nt, nullptr, 0, h, out, hout, red);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int o = nl - d + 1;                              // components in front of g_f: the tied scale and the shape columns
    double g0 = 0.0, s2 = 0.0;                             // (thread 0's)
    for (int c0 = 0; c0 < nl + 2; c0 += TIED_COLS) {
        const int cc = (nl + 2 - c0 < TIED_COLS) ? (nl + 2 - c0) : TIED_COLS;
        __syncthreads();
        for (int c = wave; c < cc; c += FIN_THREADS / 64) {
            const double* col = part + (size_t)(c0 + c) * nblocks;
            double s = 0.0;
            for (int i = lane; i < nblocks; i += 64) s += col[i];
            s = wave_sum(s);
            if (lane == 0) red[c] = s;
        }
        __syncthreads();
        if (threadIdx.x == 0)
            for (int c = c0; c < c0 + cc; c++) {
                const double s = red[c - c0];
                if (c < d) g0 = c == 0 ? s / 2.0 : g0 + s / 2.0;
                else if (c < nl) { out[9 + (c - d)] = s / 2.0; hout[9 + (c - d)] = s / 2.0; }
                else if (c == nl) s2 = s;
                else {
                    const double s3 = s;
                    const double gf = (2.0 * s2 - 2.0 * h.noise_var * s3) / 2.0, gn = (2.0 * h.noise_var * s3) / 2.0;
                    out[8 + o] = gf; out[9 + o] = gn;
                    hout[8 + o] = gf; hout[9 + o] = gn;
                }
            }
    }
    if (threadIdx.x == 0) { out[8] = g0; hout[8] = g0; }
}

int trace_num_blocks(int npad) { return tri_count(npad / KT); }

void launch_trace(const double* X, int n, int d, int npad, const CovFn& cf, const double* Kinv, const double* alpha,
                  double* part, hipStream_t s, Batch bt, const double* z, const double* logdet_part, double* out,
                  double* hout, unsigned* ticket)
{
    const int nblocks = tri_count(npad / KT);
    const bool ard = is_ard(cf);
    // the last block takes the final sums where the launch is small (its 256 threads against k_finalize's 1024: at 8192
    // rows -- 8256 blocks -- the separate launch is as fast and keeps the blocks' stores plain); TUNE_FINALIZE_FUSE_MAX.
    // ARD: always both launches -- there is no fused form of the ARD final sums
    const bool fuse = !ard && out != nullptr && nblocks <= tune(TUNE_FINALIZE_FUSE_MAX);
    const FinalizeArgs fin{z, logdet_part, npad / TILE, fuse ? out : nullptr, hout, ticket};
    hipLaunchKernelGGL(CUGP_COV_KERNEL(cf, k_trace), dim3(nblocks, bt.count), dim3(256), 0, s, X, n, d, npad, cf.h, cf.hd,
                       Kinv, alpha, part, bt.tab, fin);
    if (ard) {
        assert(hout && (out || bt.tab));
        const int nl = d + shape_count(cf.kind);
        const size_t hstride = (size_t)(ARD_ROW_GRAD + ard_num_hyper(cf, d));
        if (cf.tied)
            hipLaunchKernelGGL(k_finalize_ard_tied, dim3(1, bt.count), dim3(FIN_THREADS), 0, s, z, npad, n, nl, d,
                               logdet_part, npad / TILE, part, nblocks, cf.hd, out, hout, hstride, bt.tab);
        else
            hipLaunchKernelGGL(k_finalize_ard, dim3(1, bt.count), dim3(FIN_THREADS), 0, s, z, npad, n, nl, logdet_part,
                               npad / TILE, part, nblocks, cf.hd, out, hout, hstride, bt.tab);
    } else if (out != nullptr && !fuse) {
        launch_finalize(z, npad, n, logdet_part, npad / TILE, part, nblocks, cf.h, out, hout, s, cf.hd, bt);
    }
}
