// sparse_targets_device.h -- the passes of the sparse model that depend on the labels: p targets over one set of inducing
// points (cugp_sparse_*_targets), and the handle's own y, which is the case p = 1 (section 25).
// Everything that costs O(N M^2) -- W_c, P, B and its inverse, W_c R^T, both trace passes -- is shared by the p targets
// (sparse_device.h, sparse_gfx950.h); only what is below reads Y.  Plain fp64 arithmetic, __syncthreads and wave shuffles: no MFMA, no atomics, no
// inline assembly and no #ifdef around arithmetic -- the host check (tools/sparse_targets_host_check.cpp) runs this text
// behind tools/host_emul.h under -fsanitize=address,undefined.
//
// Include-point contract: sparse_device.h's (inside namespace cugp, behind kernels.h, the device vocabulary and
// cov_device.h); SparseFinalTargets is kernels.h's.
//
// Y: [p][ystride] target-major, each row zero beyond its n rows up to the chunks' 128-row tiles.
// Q = [q_1 .. q_p], C' = Q LB^-T, Gamma' = C' LB^-1, Beta' = Gamma' Lu^-1: [>= p][ld] target-major, one row per target.
//   H = p (I - B^-1) - sum_t gamma_t gamma_t^T   (gamma_t = gamma'_t / s2),   H2 = H - p P / s2,
//   G_c^T = W_c R^T + sum_t y_t,c (beta'_t / s2^2)^T,   F = sum_t F_t
// Every sum has a fixed order -- over the targets always ascending --: repeated launches give identical bits, and a
// target's own sums (q_t, y_t'y_t, c'_t'c'_t, F_t) do not depend on how many targets there are or where it stands.
// All kernels: 256 threads, grid (blocks, 1).
#pragma once

constexpr int SPT_GROUP = 8;     // targets per workgroup of k_sparse_wty_targets: accumulators per thread
constexpr int SPT_STAGE = 16;    // targets staged per round of k_sparse_h_targets and k_sparse_weights_targets

// The slab's share of q_t = W^T y_t for the SPT_GROUP targets of a group, W read once for all of them:
// part[(t * slabs + sl) * ld + col] = sum over the 128 rows r of slab sl of W[r][col] Y[t][r], each target's sum in one
// order -- thread (col, g) adds the rows g, g + 4, ... ascending, the four groups as (g0 + g1) + (g2 + g3).
// The targets' slab values are staged through LDS; targets beyond p are neither read nor written.
// W: [slabs * 128][ld], Y: the chunk's first row of target 0.  Grid: (ld / 64) * slabs * groups, groups = ceil(p / 8).
__global__ __launch_bounds__(256) void k_sparse_wty_targets(const double* __restrict__ W, int ld, int slabs,
                                                            const double* __restrict__ Y, size_t ystride, int p,
                                                            double* __restrict__ part)
{
#pragma clang fp contract(off)
    __shared__ double ys[SPT_GROUP][TILE];
    __shared__ double red[SPT_GROUP][4][KT];
    const int ncb = ld / KT, cb = blockIdx.x % ncb, rest = blockIdx.x / ncb, sl = rest % slabs, t0 = (rest / slabs) * SPT_GROUP;
    const int t = threadIdx.x, col = cb * KT + (t & 63), g = t >> 6;
    for (int e = t; e < SPT_GROUP * TILE; e += 256) {
        const int k = e / TILE, r = e % TILE;
        ys[k][r] = t0 + k < p ? Y[(size_t)(t0 + k) * ystride + sl * TILE + r] : 0.0;
    }
    __syncthreads();
    double acc[SPT_GROUP];
#pragma unroll
    for (int k = 0; k < SPT_GROUP; k++) acc[k] = 0.0;
    for (int j = 0; j < TILE / 4; j++) {
        const int r = g + 4 * j;
        const double w = W[(size_t)(sl * TILE + r) * ld + col];
#pragma unroll
        for (int k = 0; k < SPT_GROUP; k++) acc[k] = acc[k] + w * ys[k][r];
    }
#pragma unroll
    for (int k = 0; k < SPT_GROUP; k++) red[k][g][t & 63] = acc[k];
    __syncthreads();
    for (int e = t; e < SPT_GROUP * KT; e += 256) {
        const int k = e / KT, c = e % KT;
        if (t0 + k < p)
            part[((size_t)(t0 + k) * slabs + sl) * ld + cb * KT + c] = (red[k][0][c] + red[k][1][c]) + (red[k][2][c] + red[k][3][c]);
    }
}

// Q[t] = (first ? 0 : Q[t]) + part[t][0] + part[t][1] + ... in slab order; grid p * ceil(ld / 256)
__global__ __launch_bounds__(256) void k_sparse_wty_targets_finish(const double* __restrict__ part, int slabs, int ld, int p,
                                                                   double* __restrict__ Q, int first)
{
#pragma clang fp contract(off)
    const int nb = (ld + 255) / 256, tt = blockIdx.x / nb, i = (blockIdx.x % nb) * 256 + threadIdx.x;
    if (tt >= p || i >= ld) return;
    double s = first ? 0.0 : Q[(size_t)tt * ld + i];
    for (int j = 0; j < slabs; j++) s = s + part[((size_t)tt * slabs + j) * ld + i];
    Q[(size_t)tt * ld + i] = s;
}

// out[t] = y_t'y_t, one workgroup per target: thread v adds the squares v, v + 256, ... ascending,
// the lanes by wave_sum, the four waves as (w0 + w1) + (w2 + w3).  Grid: p.
__global__ __launch_bounds__(256) void k_sparse_yy_targets(const double* __restrict__ Y, size_t ystride, int n,
                                                           double* __restrict__ out)
{
#pragma clang fp contract(off)
    __shared__ double red[4];
    const int t = threadIdx.x;
    const double* __restrict__ y = Y + (size_t)blockIdx.x * ystride;
    double s = 0.0;
    for (int i = t; i < n; i += 256) s = s + y[i] * y[i];
    s = wave_sum(s);
    if ((t & 63) == 0) red[t >> 6] = s;
    __syncthreads();
    if (t == 0) out[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// H = p (I - B^-1) - sum_t gamma_t gamma_t^T (t ascending) and H2 = H - p (P / s2), full row-major ld x ld and zero
// beyond m, from the lower triangles of B^-1 and P (entry (i, k) is read at (max, min)); gamma_t = Gm[t] / s2, its two
// 64-entry pieces of a tile staged through LDS, SPT_STAGE targets per round.  Every workgroup also writes its share of
// Bs[t][j] = (Bt[t][j] / s2) / s2 (zero beyond m), t < p.  With p = 1 the factor p is an exact 1.0: H = (I - B^-1) - gamma
// gamma^T and H2 = H - P / s2, as section 25 writes them.
// One 64x64 tile per workgroup in four passes of 16 rows -- thread v holds the entries (16 q + v / 64 + 4 a, v % 64), a < 4,
// of pass q, and every pass stages its rounds again: four divisions in flight, not sixteen --, grid (ld / 64)^2.
__global__ __launch_bounds__(256) void k_sparse_h_targets(const double* __restrict__ Binv, const double* __restrict__ P,
                                                          const double* __restrict__ Gm, const double* __restrict__ Bt,
                                                          int p, int m, int ld, double s2, double* __restrict__ H,
                                                          double* __restrict__ H2, double* __restrict__ Bs)
{
#pragma clang fp contract(off)
    __shared__ double gi[SPT_STAGE][KT], gk[SPT_STAGE][KT];
    const int nb = ld / KT, bi = blockIdx.x / nb, bj = blockIdx.x % nb, t = threadIdx.x;
    for (size_t e = (size_t)blockIdx.x * 256 + t; e < (size_t)p * ld; e += (size_t)gridDim.x * 256)
        Bs[e] = (int)(e % ld) < m ? (Bt[e] / s2) / s2 : 0.0;
    const double pd = (double)p;
    const int k = bj * KT + (t & 63);
#pragma unroll 1
    for (int q = 0; q < 4; q++) {
        const int ir = 16 * q + (t >> 6);
        double h[4];
#pragma unroll
        for (int a = 0; a < 4; a++) {
            const int i = bi * KT + ir + 4 * a;
            h[a] = 0.0;
            if (i < m && k < m) {
                const size_t src = i >= k ? (size_t)i * ld + k : (size_t)k * ld + i;
                h[a] = pd * ((i == k ? 1.0 : 0.0) - Binv[src]);
            }
        }
#pragma unroll 1
        for (int t0 = 0; t0 < p; t0 += SPT_STAGE) {
            const int nt = p - t0 < SPT_STAGE ? p - t0 : SPT_STAGE;
            __syncthreads();
            for (int e = t; e < nt * KT; e += 256) {
                const int tt = e / KT, c = e % KT;
                const double* __restrict__ gr = Gm + (size_t)(t0 + tt) * ld;
                gi[tt][c] = bi * KT + c < m ? gr[bi * KT + c] / s2 : 0.0;
                gk[tt][c] = bj * KT + c < m ? gr[bj * KT + c] / s2 : 0.0;
            }
            __syncthreads();
#pragma unroll 2
            for (int tt = 0; tt < nt; tt++) {               // (every entry: its targets ascending)
                const double gkv = gk[tt][t & 63];
#pragma unroll
                for (int a = 0; a < 4; a++) h[a] = h[a] - gi[tt][ir + 4 * a] * gkv;
            }
        }
#pragma unroll
        for (int a = 0; a < 4; a++) {
            const int i = bi * KT + ir + 4 * a;
            double hv = 0.0, h2 = 0.0;
            if (i < m && k < m) {
                const size_t src = i >= k ? (size_t)i * ld + k : (size_t)k * ld + i;
                hv = h[a];
                h2 = hv - pd * (P[src] / s2);
            }
            H[(size_t)i * ld + k] = hv;
            H2[(size_t)i * ld + k] = h2;
        }
    }
}

// The rank-p part folded into a chunk's weights in place, over the 64x64 tiles of G ([>= 64 * row tiles][ld]):
//   G[i][j] = ((G[i][j] + Y[0][i] Bs[0][j]) + Y[1][i] Bs[1][j]) + ...      (i < nr, j < m; every other entry stays)
// the Y and Bs pieces of a tile staged through LDS, SPT_STAGE targets per round.  Y: the chunk's first row of target 0.
// Thread v holds the entries (v / 64 + 4 a, v % 64), a < 16.  Grid: row tiles * (ld / 64).
__global__ __launch_bounds__(256) void k_sparse_weights_targets(double* __restrict__ G, int ld, const double* __restrict__ Y,
                                                                size_t ystride, const double* __restrict__ Bs, int p, int nr,
                                                                int m)
{
#pragma clang fp contract(off)
    __shared__ double ys[SPT_STAGE][KT], bs[SPT_STAGE][KT];
    const int nct = ld / KT, i0 = (blockIdx.x / nct) * KT, j0 = (blockIdx.x % nct) * KT;
    if (i0 >= nr || j0 >= m) return;                       // (the whole workgroup: nothing of this tile changes)
    const int t = threadIdx.x, j = j0 + (t & 63), ir = t >> 6;
    double g[16];
#pragma unroll
    for (int a = 0; a < 16; a++) {
        const int i = i0 + ir + 4 * a;
        g[a] = (i < nr && j < m) ? G[(size_t)i * ld + j] : 0.0;
    }
    for (int t0 = 0; t0 < p; t0 += SPT_STAGE) {
        const int nt = p - t0 < SPT_STAGE ? p - t0 : SPT_STAGE;
        __syncthreads();
        for (int e = t; e < nt * KT; e += 256) {
            const int tt = e / KT, c = e % KT;
            ys[tt][c] = i0 + c < nr ? Y[(size_t)(t0 + tt) * ystride + i0 + c] : 0.0;
            bs[tt][c] = j0 + c < m ? Bs[(size_t)(t0 + tt) * ld + j0 + c] : 0.0;
        }
        __syncthreads();
#pragma unroll 2
        for (int tt = 0; tt < nt; tt++) {                   // (every entry: its targets ascending)
            const double bv = bs[tt][t & 63];
#pragma unroll
            for (int a = 0; a < 16; a++) g[a] = g[a] + ys[tt][ir + 4 * a] * bv;
        }
    }
#pragma unroll
    for (int a = 0; a < 16; a++) {
        const int i = i0 + ir + 4 * a;
        if (i < nr && j < m) G[(size_t)i * ld + j] = g[a];
    }
}

// Cs[t][j] = C[t][j] / s2 for t < p and j < m, zero beyond m and for the rows up to rows (whole 64-row target tiles: what
// k_targets_mean reads); grid-stride over rows * ld entries
__global__ __launch_bounds__(256) void k_sparse_scale_targets(const double* __restrict__ Cm, int p, int rows, int m, int ld,
                                                              double s2, double* __restrict__ Cs)
{
#pragma clang fp contract(off)
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < (size_t)rows * ld; e += (size_t)gridDim.x * 256)
        Cs[e] = (e < (size_t)p * ld && (int)(e % ld) < m) ? Cm[e] / s2 : 0.0;
}

// One workgroup (f: kernels.h SparseFinalTargets): F = sum_t F_t, (part_uf given) the nh = nl + 2 components of
// d(-F) / dtheta in the handle's order, and every F_t.
//   columns   wave w takes the columns w, w + 4, ... of the trace partials, lane l the blocks l, l + 64, ... ascending,
//             the lanes by wave_sum -- first of the rectangle (uf), then of the square (uu)
//   scalars   tr P, sum_i (1 - [B^-1]_ii) and the log-determinant shares; then target after target c'_t'c'_t and
//             gamma'_t'gamma'_t over i < m: thread v adds the entries v, v + 256, ... ascending, lanes by wave_sum, the
//             four waves as (w0 + w1) + (w2 + w3)
//   F_t  = ((((-N/2 log 2 pi - ld) - N/2 log s2) - y_t'y_t / (2 s2)) + c'_t'c'_t / (2 s2^2)) - (N sf2 - tr P) / (2 s2)
//   F    = F_0 + F_1 + ... in target order; yy, cc, gg below are the sums over the targets in the same order
//   g_c  = -(S_uf,c + S_uu,c / 2)                          (c < nl)
//   g_f  = -(2 (S_uf,nl + S_uu,nl / 2) - p N sf2 / s2)
//   g_n  = -(((p sum_i (1 - [B^-1]_ii) - p N) + (((yy - cc / s2) + p (N sf2 - tr P)) / s2)) - gg / s2^2)
// out / hout (pinned): [0] F, [1 .. nh] the gradient (left as they are without part_uf), [1 + nh + t] F_t.
__global__ __launch_bounds__(256) void k_sparse_finalize_targets(SparseFinalTargets f, const double* __restrict__ part_uf,
                                                                 size_t nb_uf, const double* __restrict__ part_uu,
                                                                 size_t nb_uu, int nl, double* __restrict__ out,
                                                                 double* __restrict__ hout)
{
#pragma clang fp contract(off)
    __shared__ double red[3][4];
    __shared__ double tred[2][2][4];
    __shared__ double tail;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (part_uf) {
        for (int c = wave; c <= nl; c += 4) {
            const double* cf = part_uf + (size_t)c * nb_uf;
            const double* cu = part_uu + (size_t)c * nb_uu;
            double a = 0.0, b = 0.0;
            for (size_t i = lane; i < nb_uf; i += 64) a = a + cf[i];
            for (size_t i = lane; i < nb_uu; i += 64) b = b + cu[i];
            a = wave_sum(a);
            b = wave_sum(b);
            const double s = a + b / 2.0;
            if (lane == 0 && c < nl) { out[1 + c] = -s; hout[1 + c] = -s; }
            if (lane == 0 && c == nl) tail = s;
        }
    }
    double v[3] = {0.0, 0.0, 0.0};
    for (int i = t; i < f.m; i += 256) {
        const size_t dg = (size_t)i * f.ld + i;
        v[0] = v[0] + f.P[dg];
        v[1] = v[1] + (1.0 - f.Binv[dg]);
    }
    for (int i = t; i < f.nt; i += 256) v[2] = v[2] + f.logdet[i];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        v[k] = wave_sum(v[k]);
        if (lane == 0) red[k][wave] = v[k];
    }
    __syncthreads();
    const double trp = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    const double tb = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    const double ld = (red[2][0] + red[2][1]) + (red[2][2] + red[2][3]);
    const double nsf = f.n * f.sf2;
    const int nh = nl + 2;
    double F = 0.0, yy = 0.0, cc = 0.0, gg = 0.0;          // (thread 0's: the sums over the targets, in target order)
    for (int tt = 0; tt < f.p; tt++) {
        const double* __restrict__ cr = f.Cp + (size_t)tt * f.ld;
        const double* __restrict__ gr = f.Gm + (size_t)tt * f.ld;
        double c = 0.0, g = 0.0;
        for (int i = t; i < f.m; i += 256) {
            c = c + cr[i] * cr[i];
            if (part_uf) g = g + gr[i] * gr[i];
        }
        c = wave_sum(c);
        g = wave_sum(g);
        if (lane == 0) { tred[tt & 1][0][wave] = c; tred[tt & 1][1][wave] = g; }
        __syncthreads();                                    // (two buffers by parity: one barrier per target)
        if (t == 0) {
            const double (*r)[4] = tred[tt & 1];
            const double cct = (r[0][0] + r[0][1]) + (r[0][2] + r[0][3]), ggt = (r[1][0] + r[1][1]) + (r[1][2] + r[1][3]);
            const double yyt = f.yy[tt];
            const double Ft = ((((-0.5 * f.n * 1.8378770664093453 - ld) - 0.5 * f.n * f.log_s2) - yyt / (2.0 * f.s2))
                               + cct / (2.0 * f.s2 * f.s2)) - (nsf - trp) / (2.0 * f.s2);
            out[1 + nh + tt] = Ft;
            hout[1 + nh + tt] = Ft;
            F = tt == 0 ? Ft : F + Ft;
            yy = tt == 0 ? yyt : yy + yyt;
            cc = tt == 0 ? cct : cc + cct;
            gg = tt == 0 ? ggt : gg + ggt;
        }
    }
    if (t == 0) {
        const double pd = (double)f.p;
        out[0] = F;
        hout[0] = F;
        if (part_uf) {
            const double gf = -(2.0 * tail - pd * nsf / f.s2);
            const double gn = -(((pd * tb - pd * f.n) + (((yy - cc / f.s2) + pd * (nsf - trp)) / f.s2)) - gg / (f.s2 * f.s2));
            out[1 + nl] = gf; out[2 + nl] = gn;
            hout[1 + nl] = gf; hout[2 + nl] = gn;
        }
    }
}
