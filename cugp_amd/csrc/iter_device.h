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

// ---- the pathwise posterior draws: the vector arithmetic around the feature product k_rff_apply ----

// The right-hand sides of the paths' solve: r[i][c] = (y_i - f[i][c]) - sn E[i][c] in exactly that order, no contraction
// (E null: the first difference alone), c < count; columns count .. tp - 1 zero.  yb: y as column 0 of an [n][16] block
__global__ __launch_bounds__(256) void k_iter_paths_rhs(const double* __restrict__ yb, const double* __restrict__ f,
                                                        const double* __restrict__ E, double sn, int count, int tp, size_t cnt,
                                                        double* __restrict__ r)
{
#pragma clang fp contract(off)
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= cnt) return;
    double v = 0.0;
    if ((int)(e % tp) < count) {
        v = yb[e / tp * 16] - f[e];
        if (E) v = v - sn * E[e];
    }
    r[e] = v;
}

// A path at the test points: k = f + k, the feature term first, one addition per entry
__global__ __launch_bounds__(256) void k_iter_paths_add(const double* __restrict__ f, double* __restrict__ k, size_t cnt)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e < cnt) k[e] = f[e] + k[e];
}

// ---- the preconditioned recurrences: z = M^-1 r, p = z + b p, a = r'z / p'Kp, b = r'z_new / r'z ----
// The plain recurrence's kernels serve wherever the arithmetic is the same: k_iter_update (x, r and the shares of r'r),
// k_iter_step_b (the sweep counted, the candidate test on r'r; the ratio it leaves in SC_B is overwritten by k_iter_step_z
// before anything reads it), k_iter_dir with z in r's place (p = z + b p, restart: p = z), k_iter_resid, k_iter_step_v.
// r'z lives in row SC_RZ, behind the rows the host reads.

// one workgroup, behind the shares of p'q: a = r'z / p'Kp; p'Kp <= 0 or NaN: the column is broken
__global__ __launch_bounds__(256) void k_iter_step_a_pc(const double* __restrict__ part, int nblk, int tp, double* __restrict__ sc)
{
    const int c = threadIdx.x;
    if (c >= tp) return;
    double st = sc[SC_STATE * IT_MAXT + c];
    if (st == ST_RESTART) st = ST_ACTIVE;
    if (st == ST_ACTIVE) {
        const double pq = iter_sum_parts(part, nblk, tp, c);
        if (pq > 0.0 && pq - pq == 0.0) sc[SC_A * IT_MAXT + c] = sc[SC_RZ * IT_MAXT + c] / pq;
        else st = ST_BROKEN;
    }
    sc[SC_STATE * IT_MAXT + c] = st;
}

// one workgroup, behind the shares of r'z for a fresh z = M^-1 r.  Active columns: b = r'z / (the r'z before it) unless
// `first` (the start: b stays 0, so that k_iter_dir leaves p = z); columns that go on from their true residual: r'z alone.
// r'z <= 0 or NaN: the column is broken
__global__ __launch_bounds__(256) void k_iter_step_z(const double* __restrict__ part, int nblk, int tp, int first,
                                                     double* __restrict__ sc)
{
    const int c = threadIdx.x;
    if (c >= tp) return;
    const double st = sc[SC_STATE * IT_MAXT + c];
    if (st != ST_ACTIVE && st != ST_RESTART) return;
    const double rz = iter_sum_parts(part, nblk, tp, c);
    if (!(rz > 0.0 && rz - rz == 0.0)) { sc[SC_STATE * IT_MAXT + c] = ST_BROKEN; return; }
    if (st == ST_ACTIVE && !first) sc[SC_B * IT_MAXT + c] = rz / sc[SC_RZ * IT_MAXT + c];
    sc[SC_RZ * IT_MAXT + c] = rz;
}

// ---- the mixed mode's cycles: the sweeps run on an fp32 product, so the recurrence's residual goes
// on falling after the true one has stalled.  A column therefore also waits for its true residual once r'r has fallen to
// rho2 times its value at the last true residual (b'b at the start): row SC_GOAL.  Rows SC_PREV and SC_STALL let the host see
// a column whose true r'r fell by less than a factor 4 between two verifications.  The kernels above keep their text.

// one workgroup, behind k_iter_init: the first cycle's goal
__global__ __launch_bounds__(256) void k_iter_goal_init(int tp, double rho2, double* __restrict__ sc)
{
    const int c = threadIdx.x;
    if (c >= tp) return;
    const double bb = sc[SC_BB * IT_MAXT + c];
    sc[SC_GOAL * IT_MAXT + c] = rho2 * bb;
    sc[SC_PREV * IT_MAXT + c] = bb;
    sc[SC_STALL * IT_MAXT + c] = 0.0;
}

// k_iter_step_b with the cycle goal beside the tolerance, and a growth limit
__global__ __launch_bounds__(256) void k_iter_step_b_mx(const double* __restrict__ part, int nblk, int tp, double* __restrict__ sc)
{
    const int c = threadIdx.x;
    if (c >= tp || sc[SC_STATE * IT_MAXT + c] != ST_ACTIVE) return;
    const double rn = iter_sum_parts(part, nblk, tp, c);
    sc[SC_ITERS * IT_MAXT + c] += 1.0;
    if (!(rn - rn == 0.0)) { sc[SC_STATE * IT_MAXT + c] = ST_BROKEN; return; }
    sc[SC_B * IT_MAXT + c] = rn / sc[SC_RR * IT_MAXT + c];
    sc[SC_RR * IT_MAXT + c] = rn;
    // |r|^2 <= cond(K) |r_0|^2 along exact CG: r'r grown 2^20-fold since the last true residual shows a K beyond what fp32
    // refines (or a recurrence that has lost the truth) without waiting for a goal that will not come
    if (rn <= sc[SC_TOL2 * IT_MAXT + c] || rn <= sc[SC_GOAL * IT_MAXT + c] || rn > 1048576.0 * sc[SC_PREV * IT_MAXT + c])
        sc[SC_STATE * IT_MAXT + c] = ST_CANDIDATE;
}

// k_iter_step_v; a column that goes on from its true residual gets the next cycle's goal, and its stall flag where the
// true r'r has not fallen by a factor 4 since the previous verification (by less where less was asked: below)
__global__ __launch_bounds__(256) void k_iter_step_v_mx(const double* __restrict__ part, int nblk, int tp, int final, double rho2,
                                                        double* __restrict__ sc)
{
#pragma clang fp contract(off)
    const int c = threadIdx.x;
    if (c >= tp) return;
    const double st = sc[SC_STATE * IT_MAXT + c];
    if (!(st == ST_CANDIDATE || (final && st == ST_ACTIVE))) return;
    const double rt = iter_sum_parts(part, nblk, tp, c);
    sc[SC_TRUE * IT_MAXT + c] = rt;
    if (!(rt - rt == 0.0)) sc[SC_STATE * IT_MAXT + c] = ST_BROKEN;
    else if (rt <= sc[SC_TOL2 * IT_MAXT + c]) sc[SC_STATE * IT_MAXT + c] = ST_DONE;
    else if (!final) {
        sc[SC_RR * IT_MAXT + c] = rt;
        sc[SC_STATE * IT_MAXT + c] = ST_RESTART;
        // the cycle asked r'r to fall from prev to max(goal, tol^2): a last leg that starts close above the tolerance is
        // not asked for a factor 4, and is held to the root of what it was asked for instead
        const double prev = sc[SC_PREV * IT_MAXT + c];
        const double goal = sc[SC_GOAL * IT_MAXT + c], tol2 = sc[SC_TOL2 * IT_MAXT + c];
        const double asked = prev / (goal > tol2 ? goal : tol2);
        const double need = asked < 16.0 ? __builtin_sqrt(asked) : 4.0;
        if (need * rt > prev) sc[SC_STALL * IT_MAXT + c] = 1.0;
        sc[SC_PREV * IT_MAXT + c] = rt;
        sc[SC_GOAL * IT_MAXT + c] = rho2 * rt;
    }
}

// The fall back to the fp64 product.  Conjugate gradients on a K32 that fp32 cannot refine drive x along directions in which
// K32 and K differ, and the true residual of such an x can lie orders of magnitude above |b|: going on from it would ask fp64
// CG for that much more than the tolerance.  So every unfinished column starts again -- x = 0, r = b, the sweeps spent stay
// counted -- and the rest of the call is the fp64 mode's solve.  k_iter_again: the vectors; k_iter_again_sc, one workgroup
// behind it: r'r = b'b, and ST_RESTART, so that k_iter_dir's restart pass sets p = r (or z) as after a failed verification
__global__ __launch_bounds__(256) void k_iter_again(const double* __restrict__ bv, double* __restrict__ x, double* __restrict__ r,
                                                    int n, int tp, const double* __restrict__ sc)
{
    const int t = threadIdx.x, c = t % tp, g = t / tp, G = 256 / tp;
    const double st = sc[SC_STATE * IT_MAXT + c];
    if (st != ST_ACTIVE && st != ST_RESTART) return;
    const size_t r0 = (size_t)blockIdx.x * IT_ROWS, r1 = r0 + IT_ROWS < (size_t)n ? r0 + IT_ROWS : (size_t)n;
    for (size_t i = r0 + g; i < r1; i += G) {
        const size_t e = i * tp + c;
        x[e] = 0.0;
        r[e] = bv[e];
    }
}
__global__ __launch_bounds__(256) void k_iter_again_sc(int tp, double* __restrict__ sc)
{
    const int c = threadIdx.x;
    if (c >= tp) return;
    const double st = sc[SC_STATE * IT_MAXT + c];
    if (st != ST_ACTIVE && st != ST_RESTART) return;
    sc[SC_RR * IT_MAXT + c] = sc[SC_BB * IT_MAXT + c];
    sc[SC_TRUE * IT_MAXT + c] = sc[SC_BB * IT_MAXT + c];
    sc[SC_STATE * IT_MAXT + c] = ST_RESTART;
}

// ---- the pivoted Cholesky factor L L' ~ Kf of the preconditioner, one launch per step ----
// State: L [n][rp] row-major (zero beyond the achieved rank), the residual diagonal dres [n] (-inf: the row is a pivot),
// piv [rp], ctl = {achieved rank, -1 while the factor runs; NaN seen}, and the workgroups' argmax shares of the step before
// (value, row), two sets used in turn.  A workgroup owns PCH_ROWS rows, one per thread.

// the better of two argmax candidates: the larger value, the lower row on equal values (a total order: the tree's shape
// does not matter); `bad` collects NaN residuals
__device__ __forceinline__ void pchol_argmax(double* rv, int* ri, int* rb, int tid)
{
    for (int h = PCH_ROWS / 2; h > 0; h >>= 1) {
        __syncthreads();
        if (tid < h) {
            const double v = rv[tid + h];
            const int i = ri[tid + h];
            if (v > rv[tid] || (v == rv[tid] && i < ri[tid])) { rv[tid] = v; ri[tid] = i; }
            rb[tid] |= rb[tid + h];
        }
    }
    __syncthreads();
}

// L = 0, dres = k(x, x) (the family's kernel_value at distance 0), piv = -1, ctl = {-1, 0}; e over n * rp entries
template <bool ARD, int KIND>
__global__ __launch_bounds__(256) void k_pchol_init(const HyperScalars* __restrict__ hd, int d, int n, int rp,
                                                    double* __restrict__ L, double* __restrict__ dres, int* __restrict__ piv,
                                                    int* __restrict__ ctl)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)n * rp) return;
    L[e] = 0.0;
    if (e < (size_t)n) {
        const HyperScalars h = *hd;
        ShapeArgs sh = ShapeArgs{0.0, 0.0};
        if constexpr (KIND == KERNEL_RQ) sh = shape_args<KIND>(ard_weights(hd), d);
        dres[e] = kernel_value<ARD, KIND>(0.0, div_prepare(h.ell_sq), h.signal_var, sh);
    }
    if (e < (size_t)rp) piv[e] = -1;
    if (e < 2) ctl[e] = e == 0 ? -1 : 0;
}

// Step k (k == kmax: the closing launch, which only decides).  Every workgroup reduces the shares of the step before --
// in ascending order, the largest residual wins, the lowest row on ties -- and so knows the pivot p without a second
// launch or a host wait.  The factor ends here (ctl[0] = k; every later launch returns at once) when the largest residual
// is NaN, or not above PCH_FLOOR (k + 1) u sf2.  Else thread i forms c = k(x_i, x_p) - sum_{m < k} L[i][m] L[p][m] (the
// distance as k_iter_cross_rhs: differences before squares, features ascending, no contraction; the sum m ascending,
// unfused; L[p][0 .. k) and x_p staged in LDS), L[i][k] = c / sqrt(dres_p), dres_i = dres_i - L[i][k]^2; rows that are pivots
// get 0, the pivot row sqrt(dres_p); and the workgroup writes its share of the next argmax
template <bool ARD, int KIND>
__global__ __launch_bounds__(PCH_ROWS) void k_pchol_step(const double* __restrict__ X, int n, int d,
                                                         const HyperScalars* __restrict__ hd, double* __restrict__ L, int rp,
                                                         double* __restrict__ dres, int* __restrict__ piv, int* __restrict__ ctl,
                                                         const double* __restrict__ shv_in, const int* __restrict__ shi_in,
                                                         double* __restrict__ shv_out, int* __restrict__ shi_out, int nwg, int k,
                                                         int kmax)
{
#pragma clang fp contract(off)
    __shared__ double rv[PCH_ROWS];
    __shared__ int ri[PCH_ROWS], rb[PCH_ROWS];
    __shared__ double lp[PCH_MAX_RANK];
    __shared__ double xs[PCH_ROWS];
    __shared__ int ended;
    const int tid = threadIdx.x;
    if (tid == 0) ended = ctl[0];
    __syncthreads();
    if (ended >= 0) return;
    const double ninf = -__builtin_inf();
    // the pivot: step 0 has no shares, every residual is k(x, x) and row 0 is the lowest
    double bv = ninf;
    int bi = PCH_NO_ROW, bad = 0;
    if (k == 0) {
        if (tid == 0) { bv = dres[0]; bi = 0; bad = bv != bv; }
    } else {
        for (int b = tid; b < nwg; b += PCH_ROWS) {
            const double v = shv_in[b];
            if (v != v) bad = 1;
            else if (v > bv) { bv = v; bi = shi_in[b]; }
        }
    }
    rv[tid] = bad ? ninf : bv; ri[tid] = bi; rb[tid] = bad;
    pchol_argmax(rv, ri, rb, tid);
    const double dp = rv[0];
    const int p = ri[0], nan_seen = rb[0];
    __syncthreads();                                   // (rv, ri, rb are written again below)
    const HyperScalars h = *hd;
    const bool stop = nan_seen || !(dp > PCH_FLOOR * (double)(k + 1) * 1.1102230246251565e-16 * h.signal_var);
    if (stop || k == kmax) {
        if (blockIdx.x == 0 && tid == 0) { ctl[0] = k; if (nan_seen) ctl[1] = 1; }
        return;
    }
    if (blockIdx.x == 0 && tid == 0) piv[k] = p;
    const double* __restrict__ wts = ard_weights(hd);
    ShapeArgs sh = ShapeArgs{0.0, 0.0};
    if constexpr (KIND == KERNEL_RQ) sh = shape_args<KIND>(wts, d);
    for (int m = tid; m < k; m += PCH_ROWS) lp[m] = L[(size_t)p * rp + m];
    const size_t i = (size_t)blockIdx.x * PCH_ROWS + tid;
    const bool live = i < (size_t)n;
    double acc = 0.0;
    for (int c0 = 0; c0 < d; c0 += PCH_ROWS) {
        __syncthreads();
        if (c0 + tid < d) xs[tid] = X[(size_t)p * d + c0 + tid];
        __syncthreads();
        const int cnt = d - c0 < PCH_ROWS ? d - c0 : PCH_ROWS;
        if (live)
            for (int f = 0; f < cnt; f++) {
                double df = X[i * d + c0 + f] - xs[f];
                if (ARD) df = df * wts[c0 + f];
                acc = acc + df * df;
            }
    }
    double mine = ninf;
    bad = 0;
    if (live) {
        const double kv = kernel_value<ARD, KIND>(acc, div_prepare(h.ell_sq), h.signal_var, sh);
        const double di = dres[i], root = __builtin_sqrt(dp);
        const double* __restrict__ li = L + i * rp;
        double s = 0.0;
        int m = 0;
        for (; m + 4 <= k; m += 4) {                   // (rp is a multiple of 64: a row starts on a 512-byte boundary)
            const double l0 = li[m], l1 = li[m + 1], l2 = li[m + 2], l3 = li[m + 3];
            s = s + l0 * lp[m];
            s = s + l1 * lp[m + 1];
            s = s + l2 * lp[m + 2];
            s = s + l3 * lp[m + 3];
        }
        for (; m < k; m++) s = s + li[m] * lp[m];
        double l = (kv - s) / root;
        if (i == (size_t)p) { l = root; mine = ninf; }
        else if (di == ninf) l = 0.0;
        else mine = di - l * l;
        L[i * rp + k] = l;
        dres[i] = mine;
        bad = mine != mine;
    }
    rv[tid] = bad ? ninf : mine; ri[tid] = live ? (int)i : PCH_NO_ROW; rb[tid] = bad;
    pchol_argmax(rv, ri, rb, tid);
    if (tid == 0) {
        shv_out[blockIdx.x] = rb[0] ? __builtin_nan("") : rv[0];
        shi_out[blockIdx.x] = ri[0];
    }
}

// ---- the log marginal likelihood's value by Lanczos quadrature (cugp_iter_loglik) ----
// A column's conjugate-gradient coefficients (a_j, b_j) are the Lanczos tridiagonal of K (preconditioned: of M^-1/2 K M^-1/2)
// started at its right-hand side.  The recording mode of solve_dev logs them, k_slq_quad turns a log into the Gauss
// quadrature of log.  No kernel above changes its text; without the mode nothing below is launched.
// rec[2][cap][IT_MAXT]: a_j in plane 0, b_j in plane 1, sweep j in row j.  meta[ML_ROWS][IT_MAXT]: the log's length, 1 once it
// is closed, 1 where the column broke down, the start weight (z'z, preconditioned r0' M^-1 r0).

// one workgroup, thread c is column c.  start: behind the solve's first scalar kernels -- an empty open log and the weight
// (row wrow of sc: SC_BB, preconditioned SC_RZ).  Else behind a sweep's last scalar kernel (k_iter_step_b, preconditioned the
// k_iter_step_z of that sweep): an active column appends (a_j, b_j); a column found outside ST_ACTIVE closes its log for the
// rest of the solve -- a candidate's last step length still counts (its sweep ran; T needs no b behind it), a broken column
// is marked.  A closed log never reopens: the sweeps after a failed true-residual check restart another Krylov space
__global__ __launch_bounds__(256) void k_iter_record(const double* __restrict__ sc, int tp, int start, int wrow, int cap,
                                                     double* __restrict__ rec, double* __restrict__ meta)
{
    const int c = threadIdx.x;
    if (c >= tp) return;
    if (start) {
        meta[ML_LEN * IT_MAXT + c] = 0.0;
        meta[ML_CLOSED * IT_MAXT + c] = 0.0;
        meta[ML_BROKEN * IT_MAXT + c] = 0.0;
        meta[ML_W * IT_MAXT + c] = sc[wrow * IT_MAXT + c];
        return;
    }
    if (meta[ML_CLOSED * IT_MAXT + c] != 0.0) return;
    const double st = sc[SC_STATE * IT_MAXT + c];
    const int j = (int)meta[ML_LEN * IT_MAXT + c];
    if (st != ST_ACTIVE) {
        meta[ML_CLOSED * IT_MAXT + c] = 1.0;
        if (st == ST_BROKEN) meta[ML_BROKEN * IT_MAXT + c] = 1.0;
        if (st != ST_CANDIDATE) return;
    }
    if (j >= cap) return;
    rec[(size_t)j * IT_MAXT + c] = sc[SC_A * IT_MAXT + c];
    rec[((size_t)cap + j) * IT_MAXT + c] = st == ST_ACTIVE ? sc[SC_B * IT_MAXT + c] : 0.0;
    meta[ML_LEN * IT_MAXT + c] = (double)(j + 1);
}

// one workgroup, thread c < cnt is column c: quad[c] = w_c sum_i tau_i^2 log lambda_i for the Jacobi matrix T of the column's
// log of length m,  T_00 = 1 / a_0,  T_jj = 1 / a_j + b_(j-1) / a_(j-1),  T_j,j+1 = sqrt(b_j) / a_j  (j + 1 < m):  lambda its
// eigenvalues, tau the first components of its eigenvectors (Golub-Welsch).  Implicit-shift QL on (dg, of) carrying the first
// row of the eigenvector matrix only: work[3][cap][IT_MAXT] doubles of device memory (dg, of, tau; a column strides IT_MAXT),
// no LDS, no barrier.  The eigenvalues are then sorted ascending (insertion, tau with them) and the terms added in ascending
// i: the first copied, then s = s + term.  m = 0 (z = 0): 0.  NaN: a broken column, an eigenvalue that is not positive and
// finite, or an eigenvalue that has not split off after 30 QL sweeps
__global__ __launch_bounds__(256) void k_slq_quad(const double* __restrict__ rec, const double* __restrict__ meta, int cnt, int cap,
                                                  double* __restrict__ work, double* __restrict__ quad)
{
#pragma clang fp contract(off)
    const int c = threadIdx.x;
    if (c >= cnt) return;
    const int m = (int)meta[ML_LEN * IT_MAXT + c];
    const double nan = __builtin_nan("");
    if (meta[ML_BROKEN * IT_MAXT + c] != 0.0) { quad[c] = nan; return; }
    if (m == 0) { quad[c] = 0.0; return; }
    double* __restrict__ dg = work + c;
    double* __restrict__ of = work + (size_t)cap * IT_MAXT + c;
    double* __restrict__ tau = work + (size_t)2 * cap * IT_MAXT + c;
    const double* __restrict__ ra = rec + c;
    const double* __restrict__ rb = rec + (size_t)cap * IT_MAXT + c;
#define AT(v, i) v[(size_t)(i) * IT_MAXT]
    for (int j = 0; j < m; j++) {
        const double a = AT(ra, j);
        AT(dg, j) = j == 0 ? 1.0 / a : 1.0 / a + AT(rb, j - 1) / AT(ra, j - 1);
        AT(of, j) = j + 1 < m ? __builtin_sqrt(AT(rb, j)) / a : 0.0;
        AT(tau, j) = j == 0 ? 1.0 : 0.0;
    }
    bool bad = false;
    for (int l = 0; l < m && !bad; l++) {
        int iter = 0, mm;
        do {
            for (mm = l; mm < m - 1; mm++) {
                const double dd = __builtin_fabs(AT(dg, mm)) + __builtin_fabs(AT(dg, mm + 1));
                if (__builtin_fabs(AT(of, mm)) + dd == dd) break;
            }
            if (mm == l) break;
            if (iter++ == 30) { bad = true; break; }
            double g = (AT(dg, l + 1) - AT(dg, l)) / (2.0 * AT(of, l));
            double r = __builtin_sqrt(g * g + 1.0);
            g = AT(dg, mm) - AT(dg, l) + AT(of, l) / (g + (g >= 0.0 ? r : -r));
            double s = 1.0, cs = 1.0, p = 0.0;
            int i;
            for (i = mm - 1; i >= l; i--) {
                double f = s * AT(of, i);
                const double b = cs * AT(of, i);
                r = __builtin_sqrt(f * f + g * g);
                AT(of, i + 1) = r;
                if (r == 0.0) { AT(dg, i + 1) = AT(dg, i + 1) - p; AT(of, mm) = 0.0; break; }
                s = f / r;
                cs = g / r;
                g = AT(dg, i + 1) - p;
                r = (AT(dg, i) - g) * s + 2.0 * cs * b;
                p = s * r;
                AT(dg, i + 1) = g + p;
                g = cs * r - b;
                f = AT(tau, i + 1);
                AT(tau, i + 1) = s * AT(tau, i) + cs * f;
                AT(tau, i) = cs * AT(tau, i) - s * f;
            }
            if (r == 0.0 && i >= l) continue;
            AT(dg, l) = AT(dg, l) - p;
            AT(of, l) = g;
            AT(of, mm) = 0.0;
        } while (true);
    }
    if (bad) { quad[c] = nan; return; }
    for (int i = 1; i < m; i++) {                          // ascending eigenvalues, their weights with them
        const double v = AT(dg, i), w = AT(tau, i);
        int k = i - 1;
        for (; k >= 0 && AT(dg, k) > v; k--) { AT(dg, k + 1) = AT(dg, k); AT(tau, k + 1) = AT(tau, k); }
        AT(dg, k + 1) = v;
        AT(tau, k + 1) = w;
    }
    double s = 0.0;
    for (int i = 0; i < m; i++) {
        const double lam = AT(dg, i);
        if (!(lam > 0.0 && lam - lam == 0.0)) { quad[c] = nan; return; }
        const double term = (AT(tau, i) * AT(tau, i)) * log(lam);
        s = i == 0 ? term : s + term;
    }
#undef AT
    quad[c] = meta[ML_W * IT_MAXT + c] * s;
}

// one workgroup, the call's last launch: out[0] = y'alpha from the shares of k_iter_dot over (y, alpha) (column 0 of two
// [n][16] blocks), out[1] = (1 / t) sum_p quad[p] in probe order, out[2] = -2 sum_(j < r) log U[j][j] (U = Lc^-T of the
// preconditioner's r x r side, row stride ldu: 2 sum log diag Lc; r = 0: 0).  First term copied, then s = s + term
__global__ __launch_bounds__(64) void k_slq_finish(const double* __restrict__ part, int nblk, const double* __restrict__ quad, int t,
                                                   const double* __restrict__ Ud, int ldu, int r, double* __restrict__ out)
{
#pragma clang fp contract(off)
    if (threadIdx.x == 0) out[0] = iter_sum_parts(part, nblk, 16, 0);
    if (threadIdx.x == 1) {
        double s = quad[0];
        for (int p = 1; p < t; p++) s = s + quad[p];
        out[1] = s / (double)t;
    }
    if (threadIdx.x == 2) {
        double s = 0.0;
        for (int j = 0; j < r; j++) {
            const double term = log(Ud[(size_t)j * ldu + j]);
            s = j == 0 ? term : s + term;
        }
        out[2] = -2.0 * s;
    }
}

// ---- the variance cache's small kernels (cugp_iter_varcache_build; the tall kernels and every
// launcher: iter_varcache_gfx950.h).  ctl: VC_GOT columns accepted so far, VC_REASON 0 | 1 basis ended | 2 pivot ended,
// VC_PRODUCTS products whose block was live, VC_LIVE live columns of the block orthonormalised last ----

__global__ __launch_bounds__(64) void k_vc_init(int* __restrict__ ctl)
{
    if (threadIdx.x < VC_CTL) ctl[threadIdx.x] = 0;
}

// Hc = C (first; a live block's product is counted) or Hc = Hc + C: the two Gram-Schmidt passes' coefficients, [rp][16]
__global__ __launch_bounds__(256) void k_vc_hacc(const double* __restrict__ Cm, double* __restrict__ Hc, int cnt, int first,
                                                 int* __restrict__ ctl)
{
#pragma clang fp contract(off)
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < cnt) Hc[e] = first ? Cm[e] : Hc[e] + Cm[e];
    if (first && e == 0 && ctl[VC_LIVE] > 0) ctl[VC_PRODUCTS] = ctl[VC_PRODUCTS] + 1;
}

// One workgroup: a round of CholQR on the block of cw columns at c0, and the block column of H behind the second round.
//   G = rows [c0, c0 + cw) of C = Q'W (the block lies in its slot of Q: its Gram matrix) = T'T, T upper triangular, by thread 0
//   in column order; Ti = T^-1 (zero beyond the live columns) for k_vc_scale.
//   mode 0, first round: pivot c is the column's squared norm after both projection passes and the block's earlier columns; the
//     basis ends at the first c with pivot <= VC_FLOOR (c0 + c + 1) u nrm0[c] (nrm0: the squared norm before projection), or not
//     finite: VC_GOT = c0 + c, VC_REASON = 1.  A basis that ended before: no live column.
//   mode 1, second round on the VC_LIVE columns of the first: ends only at a pivot that is not positive and finite.
//   mode 2: no round (the last block's product: nothing is orthonormalised behind it).
//   record (modes 1, 2): block column c0p of H, rows r < c0 and columns c0p + b < c0, from Hc -- both passes' Q'(K P), the
//     product's block P measured against every column up to its own.  The rows below, of the block orthonormalised here, are
//     not taken from T: a ragged last block keeps fewer columns than the product has, and the entry's mirror image in the block
//     column of the NEXT product is complete (k_vc_hsym).
__global__ __launch_bounds__(256) void k_vc_factor(const double* __restrict__ Cm, int c0, int cw, int mode, int record,
                                                   const double* __restrict__ nrm0, double* __restrict__ Ti,
                                                   const double* __restrict__ Hc, double* __restrict__ H, int rp, int c0p,
                                                   int* __restrict__ ctl)
{
#pragma clang fp contract(off)
    __shared__ double G[16][17], T[16][17], V[16][17];
    __shared__ int live_s;
    const int tid = threadIdx.x, a = tid >> 4, b = tid & 15;
    if (mode == 1) cw = ctl[VC_LIVE] < cw ? ctl[VC_LIVE] : cw;
    if (mode == 0 && ctl[VC_REASON] != 0) cw = 0;
    if (mode == 2) cw = 0;
    G[a][b] = (a < cw && b < cw) ? Cm[(size_t)(c0 + a) * 16 + b] : 0.0;
    T[a][b] = 0.0;
    V[a][b] = 0.0;
    __syncthreads();
    if (tid == 0) {
        int live = cw;
        for (int c = 0; c < cw; c++) {
            double p = G[c][c];
            for (int m = 0; m < c; m++) p = p - T[m][c] * T[m][c];
            const double floor = mode == 0 ? VC_FLOOR * (double)(c0 + c + 1) * 1.1102230246251565e-16 * nrm0[c] : 0.0;
            if (!(p > floor) || !(p < INFINITY)) { live = c; break; }
            const double t = __builtin_sqrt(p);
            T[c][c] = t;
            for (int q = c + 1; q < cw; q++) {
                double v = G[c][q];
                for (int m = 0; m < c; m++) v = v - T[m][c] * T[m][q];
                T[c][q] = v / t;
            }
        }
        for (int q = 0; q < live; q++) {               // V = T^-1 over the live columns, column q upwards from the diagonal
            V[q][q] = 1.0 / T[q][q];
            for (int r = q - 1; r >= 0; r--) {
                double s = 0.0;
                for (int m = r + 1; m <= q; m++) s = s + T[r][m] * V[m][q];
                V[r][q] = -s / T[r][r];
            }
        }
        live_s = live;
        if (mode != 2) {
            if (live < cw) { ctl[VC_GOT] = c0 + live; ctl[VC_REASON] = 1; }
            else if (mode == 0 && cw > 0) ctl[VC_GOT] = c0 + cw;
            ctl[VC_LIVE] = live;
        }
    }
    __syncthreads();
    const int live = live_s;
    if (mode != 2) Ti[tid] = (a < live && b < live) ? V[a][b] : 0.0;
    if (!record) return;
    for (int e = tid; e < c0 * 16; e += 256)
        if (c0p + (e & 15) < c0) H[(size_t)(e >> 4) * rp + c0p + (e & 15)] = Hc[e];
}

// S = the symmetric matrix the factor is taken of, over the leading VC_GOT rows and columns (blocks of bw): a diagonal block
// is (H + H') / 2 (the sum is commutative: S is symmetric to the bit), every other entry the one of H's UPPER block triangle --
// Q_i'(K P_j), i < j, measured by the projections -- on both sides.  Beyond VC_GOT: the identity.
__global__ __launch_bounds__(256) void k_vc_hsym(const double* __restrict__ H, double* __restrict__ S, int rp, int bw,
                                                 const int* __restrict__ ctl)
{
#pragma clang fp contract(off)
    const int e = blockIdx.x * 256 + threadIdx.x, got = ctl[VC_GOT];
    if (e >= rp * rp) return;
    const int i = e / rp, j = e % rp, bi = i / bw, bj = j / bw;
    const double hij = H[(size_t)i * rp + j], hji = H[(size_t)j * rp + i];
    S[e] = (i < got && j < got) ? (bi == bj ? (hij + hji) * 0.5 : bi < bj ? hij : hji) : (i == j ? 1.0 : 0.0);
}

// One workgroup: S = L L' in place over the leading VC_GOT columns (lower triangle; right-looking, a column at a time, every
// entry's updates in ascending column order).  Column c's scaled entries go through LDS; the trailing update walks rows four
// at a time per wave (wave w: rows c + 1 + w, + 4, ...), a wave's lanes along the row: row-contiguous reads and writes.
// A pivot that is not positive and finite ends the factor there: VC_GOT = c, VC_REASON = 2; k_vc_rsolve reads no column beyond.
__global__ __launch_bounds__(256) void k_vc_chol(double* __restrict__ S, int rp, int* __restrict__ ctl)
{
#pragma clang fp contract(off)
    __shared__ double col[PCH_MAX_RANK];
    const int tid = threadIdx.x, ty = tid >> 6, tx = tid & 63;
    const int got = ctl[VC_GOT];
    for (int c = 0; c < got; c++) {
        __syncthreads();
        const double piv = S[(size_t)c * rp + c];
        if (!(piv > 0.0) || !(piv < INFINITY)) {
            if (tid == 0) { ctl[VC_GOT] = c; ctl[VC_REASON] = 2; }
            return;
        }
        const double l = __builtin_sqrt(piv);
        for (int i = c + 1 + tid; i < got; i += 256) {
            const double v = S[(size_t)i * rp + c] / l;
            S[(size_t)i * rp + c] = v;
            col[i] = v;
        }
        __syncthreads();
        if (tid == 0) S[(size_t)c * rp + c] = l;
        for (int i = c + 1 + ty; i < got; i += 4) {
            const double li = col[i];
            for (int j = c + 1 + tx; j <= i; j += 64) S[(size_t)i * rp + j] = S[(size_t)i * rp + j] - li * col[j];
        }
    }
}

// s[i] = the squared norm of R'k*_i from k_cov_var's sums, i < nt.  split == 1: g[z][i] holds the column group's sum of squares;
// else part[k][i][c] the ranges' shares of u_ic: added in range order, squared and summed in column order inside the group
// (from 0, as the kernel does).  The groups are added in ascending order, first copied.
__global__ __launch_bounds__(256) void k_cov_var_finish(const double* __restrict__ part, int split, const double* __restrict__ g,
                                                        int nz, int gw, int nt, int rp, double* __restrict__ s)
{
#pragma clang fp contract(off)
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nt) return;
    double tot = 0.0;
    for (int z = 0; z < nz; z++) {
        double sz;
        if (split == 1) {
            sz = g[(size_t)z * nt + i];
        } else {
            sz = 0.0;
            for (int c = z * gw; c < (z + 1) * gw && c < rp; c++) {
                double u = part[(size_t)i * rp + c];
                for (int k = 1; k < split; k++) u = u + part[((size_t)k * nt + i) * rp + c];
                sz = sz + u * u;
            }
        }
        tot = z == 0 ? sz : tot + sz;
    }
    s[i] = tot;
}
