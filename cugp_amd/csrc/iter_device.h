// iter_device.h -- the vector kernels of the matrix-free exact GP (cugp_iter_*): t independent
// conjugate-gradient recurrences that share each product with K, and the right-hand sides of the predictive variance.
// Plain fp64 arithmetic and __syncthreads: emulable (tools/iter_host_check.cpp runs this text behind tools/host_emul.h).
// The product itself, k_cov_apply, needs the MFMA and stands in iter_gfx950.h with every launcher.
//
// Include-point contract.  Included INSIDE namespace cugp, after kernels.h (HyperScalars, KERNEL_*, IT_*, SC_*, ST_*) and
// cov_device.h (DivBy, div_prepare, ard_weights, ShapeArgs, shape_args, kernel_value).
//
// Layout.  Every vector block is [n][tp] row-major, tp = 16 or 64 columns (t padded; the padding columns are zero in b and
// therefore frozen from the start).  A vector kernel's workgroup owns IT_ROWS consecutive rows; thread (g, c) = (tid / tp,
// tid % tp) walks the rows r0 + g, r0 + g + G, ... (G = 256 / tp) of column c in ascending order.
// Sums.  A column's dot product: a workgroup's rows fall into IT_LANES = 16 residue classes (row - r0) mod 16, each summed
// in row order (a thread owns 16 / G of them); the 16 class sums are added in ascending class order by the column's first
// thread; the workgroups' shares in ascending block order by thread c of the one-workgroup step kernel behind it.  First
// term copied, then s = s + term: no atomics, no shuffles, the same bits on every run, and column c's bits depend neither
// on what the other columns hold nor on tp.
// Scalars.  sc[SC_ROWS][IT_MAXT] in device memory, one column per recurrence; the host reads it (a copy into pinned
// memory) every check_every sweeps and nowhere else.  A column whose state is not ST_ACTIVE is frozen: no kernel below
// changes its x, r or p (ST_RESTART: k_iter_dir with restart_only sets p = r, the next k_iter_step_a makes it active again).
#pragma once

// part[blk * tp + c] = sum over the block's rows of a[i][c] b[i][c]
__device__ __forceinline__ void iter_dot_body(const double* __restrict__ a, const double* __restrict__ b, int n, int tp,
                                              double* __restrict__ part)
{
#pragma clang fp contract(off)
    __shared__ double red[IT_LANES * IT_MAXT];
    const int t = threadIdx.x, c = t % tp, g = t / tp, G = 256 / tp;
    const size_t r0 = (size_t)blockIdx.x * IT_ROWS, r1 = r0 + IT_ROWS < (size_t)n ? r0 + IT_ROWS : (size_t)n;
    for (int rho = g; rho < IT_LANES; rho += G) {
        double s = 0.0;
        for (size_t i = r0 + rho; i < r1; i += IT_LANES) s = s + a[i * tp + c] * b[i * tp + c];
        red[rho * tp + c] = s;
    }
    __syncthreads();
    if (g == 0) {
        double s = red[c];
        for (int q = 1; q < IT_LANES; q++) s = s + red[q * tp + c];
        part[(size_t)blockIdx.x * tp + c] = s;
    }
}
__global__ __launch_bounds__(256) void k_iter_dot(const double* __restrict__ a, const double* __restrict__ b, int n, int tp,
                                                  double* __restrict__ part)
{
    iter_dot_body(a, b, n, tp, part);
}

// the workgroups' shares of column c in block order
__device__ __forceinline__ double iter_sum_parts(const double* __restrict__ part, int nblk, int tp, int c)
{
#pragma clang fp contract(off)
    double s = part[c];
    for (int b = 1; b < nblk; b++) s = s + part[(size_t)b * tp + c];
    return s;
}
// out[c] = the whole dot product (the variance's ks' K^-1 ks); one workgroup
__global__ __launch_bounds__(256) void k_iter_sum(const double* __restrict__ part, int nblk, int tp, double* __restrict__ out)
{
    const int c = threadIdx.x;
    if (c < tp) out[c] = iter_sum_parts(part, nblk, tp, c);
}

// x = 0, r = p = b over cnt = n * tp entries
__global__ __launch_bounds__(256) void k_iter_start(const double* __restrict__ b, double* __restrict__ x, double* __restrict__ r,
                                                    double* __restrict__ p, size_t cnt)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= cnt) return;
    const double v = b[e];
    x[e] = 0.0; r[e] = v; p[e] = v;
}

// one workgroup: b'b from its shares; the column's scalars.  b = 0: done in 0 iterations with x = 0; b'b not finite: broken
__global__ __launch_bounds__(256) void k_iter_init(const double* __restrict__ part, int nblk, int tp, double tol,
                                                   double* __restrict__ sc)
{
#pragma clang fp contract(off)
    const int c = threadIdx.x;
    if (c >= tp) return;
    const double bb = iter_sum_parts(part, nblk, tp, c);
    sc[SC_RR * IT_MAXT + c] = bb;
    sc[SC_BB * IT_MAXT + c] = bb;
    sc[SC_TOL2 * IT_MAXT + c] = (tol * tol) * bb;
    sc[SC_A * IT_MAXT + c] = 0.0;
    sc[SC_B * IT_MAXT + c] = 0.0;
    sc[SC_ITERS * IT_MAXT + c] = 0.0;
    sc[SC_TRUE * IT_MAXT + c] = bb;
    sc[SC_STATE * IT_MAXT + c] = bb == 0.0 ? ST_DONE : (bb - bb == 0.0 ? ST_ACTIVE : ST_BROKEN);
}

// one workgroup, behind the shares of p'q: a = r'r / p'Kp; p'Kp <= 0 or NaN: the column is broken
__global__ __launch_bounds__(256) void k_iter_step_a(const double* __restrict__ part, int nblk, int tp, double* __restrict__ sc)
{
    const int c = threadIdx.x;
    if (c >= tp) return;
    double st = sc[SC_STATE * IT_MAXT + c];
    if (st == ST_RESTART) st = ST_ACTIVE;
    if (st == ST_ACTIVE) {
        const double pq = iter_sum_parts(part, nblk, tp, c);
        if (pq > 0.0 && pq - pq == 0.0) sc[SC_A * IT_MAXT + c] = sc[SC_RR * IT_MAXT + c] / pq;
        else st = ST_BROKEN;
    }
    sc[SC_STATE * IT_MAXT + c] = st;
}

// active columns: x += a p, r -= a q; every column: the block's share of r'r
__global__ __launch_bounds__(256) void k_iter_update(double* __restrict__ x, double* __restrict__ r, const double* __restrict__ p,
                                                     const double* __restrict__ q, int n, int tp, const double* __restrict__ sc,
                                                     double* __restrict__ part)
{
#pragma clang fp contract(off)
    const int t = threadIdx.x, c = t % tp, g = t / tp, G = 256 / tp;
    if (sc[SC_STATE * IT_MAXT + c] == ST_ACTIVE) {
        const double a = sc[SC_A * IT_MAXT + c];
        const size_t r0 = (size_t)blockIdx.x * IT_ROWS, r1 = r0 + IT_ROWS < (size_t)n ? r0 + IT_ROWS : (size_t)n;
        for (size_t i = r0 + g; i < r1; i += G) {
            const size_t e = i * tp + c;
            x[e] = x[e] + a * p[e];
            r[e] = r[e] - a * q[e];
        }
    }
    iter_dot_body(r, r, n, tp, part);              // (a thread reads back its own entries only)
}

// one workgroup, behind the shares of the new r'r: b = r'r_new / r'r, the sweep counted; the recurrence's residual at or
// below tol |b|: the column waits for its true residual (ST_CANDIDATE)
__global__ __launch_bounds__(256) void k_iter_step_b(const double* __restrict__ part, int nblk, int tp, double* __restrict__ sc)
{
    const int c = threadIdx.x;
    if (c >= tp || sc[SC_STATE * IT_MAXT + c] != ST_ACTIVE) return;
    const double rn = iter_sum_parts(part, nblk, tp, c);
    sc[SC_ITERS * IT_MAXT + c] += 1.0;
    if (!(rn - rn == 0.0)) { sc[SC_STATE * IT_MAXT + c] = ST_BROKEN; return; }
    sc[SC_B * IT_MAXT + c] = rn / sc[SC_RR * IT_MAXT + c];
    sc[SC_RR * IT_MAXT + c] = rn;
    if (rn <= sc[SC_TOL2 * IT_MAXT + c]) sc[SC_STATE * IT_MAXT + c] = ST_CANDIDATE;
}

// active columns: p = r + b p (a sweep's last launch); restart_only, behind a failed true-residual check: p = r for the
// columns that go on from it, nothing else
__global__ __launch_bounds__(256) void k_iter_dir(double* __restrict__ p, const double* __restrict__ r, int n, int tp,
                                                  const double* __restrict__ sc, int restart_only)
{
#pragma clang fp contract(off)
    const int t = threadIdx.x, c = t % tp, g = t / tp, G = 256 / tp;
    const double st = sc[SC_STATE * IT_MAXT + c];
    if (st != (restart_only ? ST_RESTART : ST_ACTIVE)) return;
    const double b = st == ST_ACTIVE ? sc[SC_B * IT_MAXT + c] : 0.0;
    const size_t r0 = (size_t)blockIdx.x * IT_ROWS, r1 = r0 + IT_ROWS < (size_t)n ? r0 + IT_ROWS : (size_t)n;
    for (size_t i = r0 + g; i < r1; i += G) {
        const size_t e = i * tp + c;
        p[e] = st == ST_ACTIVE ? r[e] + b * p[e] : r[e];
    }
}

// the true residual, q = K x given: columns that wait for it (and, final, the active ones) get r = b - q; every column: the
// block's share of r'r
__global__ __launch_bounds__(256) void k_iter_resid(const double* __restrict__ bv, const double* __restrict__ q,
                                                    double* __restrict__ r, int n, int tp, const double* __restrict__ sc,
                                                    int final, double* __restrict__ part)
{
#pragma clang fp contract(off)
    const int t = threadIdx.x, c = t % tp, g = t / tp, G = 256 / tp;
    const double st = sc[SC_STATE * IT_MAXT + c];
    if (st == ST_CANDIDATE || (final && st == ST_ACTIVE)) {
        const size_t r0 = (size_t)blockIdx.x * IT_ROWS, r1 = r0 + IT_ROWS < (size_t)n ? r0 + IT_ROWS : (size_t)n;
        for (size_t i = r0 + g; i < r1; i += G) {
            const size_t e = i * tp + c;
            r[e] = bv[e] - q[e];
        }
    }
    iter_dot_body(r, r, n, tp, part);
}

// one workgroup, behind k_iter_resid: the true |r|^2 is what the column reports; at or below tol |b|: done; else the column
// goes on from the true residual (final: it stays as it is, unconverged)
__global__ __launch_bounds__(256) void k_iter_step_v(const double* __restrict__ part, int nblk, int tp, int final,
                                                     double* __restrict__ sc)
{
    const int c = threadIdx.x;
    if (c >= tp) return;
    const double st = sc[SC_STATE * IT_MAXT + c];
    if (!(st == ST_CANDIDATE || (final && st == ST_ACTIVE))) return;
    const double rt = iter_sum_parts(part, nblk, tp, c);
    sc[SC_TRUE * IT_MAXT + c] = rt;
    if (!(rt - rt == 0.0)) sc[SC_STATE * IT_MAXT + c] = ST_BROKEN;
    else if (rt <= sc[SC_TOL2 * IT_MAXT + c]) sc[SC_STATE * IT_MAXT + c] = ST_DONE;
    else if (!final) { sc[SC_RR * IT_MAXT + c] = rt; sc[SC_STATE * IT_MAXT + c] = ST_RESTART; }
}

// broken columns: x = NaN (the header's convention for a covariance that cannot be factored)
__global__ __launch_bounds__(256) void k_iter_poison(double* __restrict__ x, int n, int tp, const double* __restrict__ sc)
{
    const int t = threadIdx.x, c = t % tp, g = t / tp, G = 256 / tp;
    if (sc[SC_STATE * IT_MAXT + c] != ST_BROKEN) return;
    const size_t r0 = (size_t)blockIdx.x * IT_ROWS, r1 = r0 + IT_ROWS < (size_t)n ? r0 + IT_ROWS : (size_t)n;
    for (size_t i = r0 + g; i < r1; i += G) x[i * tp + c] = __builtin_nan("");
}

// R[j][c] = k(x_j, xt_c), j < n, c < count; columns count .. tp - 1 zero: the right-hand sides of the variance.  Differences
// before squares, the features in index order, no contraction (k_cov_apply's entry of the same pair has the same bits)
template <bool ARD, int KIND>
__global__ __launch_bounds__(256) void k_iter_cross_rhs(const double* __restrict__ X, int n, int d, const double* __restrict__ Xt,
                                                        int count, int tp, const HyperScalars* __restrict__ hd,
                                                        double* __restrict__ R)
{
#pragma clang fp contract(off)
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)n * tp) return;
    const size_t j = e / tp;
    const int c = (int)(e % tp);
    double v = 0.0;
    if (c < count) {
        const HyperScalars h = *hd;
        const double* __restrict__ wts = ard_weights(hd);
        ShapeArgs sh = ShapeArgs{0.0, 0.0};
        if constexpr (KIND == KERNEL_RQ) sh = shape_args<KIND>(wts, d);
        double acc = 0.0;
        for (int f = 0; f < d; f++) {
            double df = X[j * d + f] - Xt[(size_t)c * d + f];
            if (ARD) df = df * wts[f];
            acc = acc + df * df;
        }
        v = kernel_value<ARD, KIND>(acc, div_prepare(h.ell_sq), h.signal_var, sh);
    }
    R[e] = v;
}
