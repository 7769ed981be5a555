// sparse_shard_device.h -- the sparse variational model with its data rows sharded over ranks (cugp_sparse_sharded_*;
// DESIGN.md section 32): the three passes that are new beside sparse_device.h and sparse_targets_device.h -- the sum of the
// shards' slots of a gathered block in global shard order, a shard's trace sums, and the final sums with the global N and
// y'y read from the device.  Plain fp64 arithmetic, __syncthreads and wave shuffles: no MFMA, no atomics, no inline
// assembly and no #ifdef around arithmetic -- the host check (tools/sparse_shard_host_check.cpp) runs this text behind
// tools/host_emul.h under -fsanitize=address,undefined.
//
// Include-point contract: sparse_device.h's (inside namespace cugp, behind kernels.h, the device vocabulary and
// cov_device.h: wave_sum); SparseFinalSharded is kernels.h's.
//
// Shard k of K lives on rank k mod W in slot k / W of that rank's block (bcm.py's gather_row_index).  Every sum over the
// shards runs k = 0, 1, .. K - 1: the first term is copied, every further one added as a = a + b, so the bits depend on
// (data, K) and on neither W nor the slots per rank, and K = 1 hands the one shard's numbers on unchanged.
// All kernels: 256 threads, grid (blocks, 1).
#pragma once

// out[e] = sum over the shards k = 0 .. nshards - 1, in that order, of entry off + e of shard k's slot, e < len.
// src: the gathered blocks, rank r's at src + r * rstride: [hdr doubles | slots of `slot` doubles]; a world of one hands its
// own send block in (rstride unread).  Slots beyond a rank's shards are never read.  Grid-stride over len.
__global__ __launch_bounds__(256) void k_sparse_shard_reduce(const double* __restrict__ src, size_t rstride, size_t hdr,
                                                             size_t slot, size_t off, size_t len, int world, int nshards,
                                                             double* __restrict__ out)
{
#pragma clang fp contract(off)
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < len; e += (size_t)gridDim.x * 256) {
        double a = src[hdr + off + e];                     // shard 0: rank 0, slot 0
        for (int k = 1; k < nshards; k++)
            a = a + src[(size_t)(k % world) * rstride + hdr + (size_t)(k / world) * slot + off + e];
        out[e] = a;
    }
}

// One workgroup: out[c] = the sum of column c of a shard's trace partials, c <= nl, in k_sparse_finalize_targets' order --
// wave w takes the columns w, w + 4, ..., lane l the blocks l, l + 64, ... ascending, the lanes by wave_sum.
__global__ __launch_bounds__(256) void k_sparse_shard_sums(const double* __restrict__ part_uf, size_t nb_uf, int nl,
                                                           double* __restrict__ out)
{
#pragma clang fp contract(off)
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    for (int c = wave; c <= nl; c += 4) {
        const double* cf = part_uf + (size_t)c * nb_uf;
        double a = 0.0;
        for (size_t i = lane; i < nb_uf; i += 64) a = a + cf[i];
        a = wave_sum(a);
        if (lane == 0) out[c] = a;
    }
}

// One workgroup (f: kernels.h SparseFinalSharded): k_sparse_finalize_targets at p = 1 with the rectangle's sums handed in
// reduced (suf[c] = sum over the shards of S_uf,c) and N and y'y read from the device (f.yyn = {y'y, N}, both summed over
// the shards): s_c = suf[c] + S_uu,c / 2 with S_uu,c summed as there, and every expression below as there, term for term.
//   F    = ((((-N/2 log 2 pi - ld) - N/2 log s2) - y'y / (2 s2)) + c''c' / (2 s2^2)) - (N sf2 - tr P) / (2 s2)
//   g_c  = -s_c   (c < nl),   g_f = -(2 s_nl - N sf2 / s2)
//   g_n  = -(((sum_i (1 - [B^-1]_ii) - N) + (((y'y - c''c' / s2) + (N sf2 - tr P)) / s2)) - gamma''gamma' / s2^2)
// out / hout (pinned): [0] F, [1 .. nh] the gradient (left as they are without suf), [1 + nh] F again (the one target's).
__global__ __launch_bounds__(256) void k_sparse_finalize_sharded(SparseFinalSharded f, const double* __restrict__ suf,
                                                                 const double* __restrict__ part_uu, size_t nb_uu, int nl,
                                                                 double* __restrict__ out, double* __restrict__ hout)
{
#pragma clang fp contract(off)
    __shared__ double red[3][4];
    __shared__ double tred[2][4];
    __shared__ double tail;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (suf) {
        for (int c = wave; c <= nl; c += 4) {
            const double* cu = part_uu + (size_t)c * nb_uu;
            double b = 0.0;
            for (size_t i = lane; i < nb_uu; i += 64) b = b + cu[i];
            b = wave_sum(b);
            const double s = suf[c] + b / 2.0;
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
    double c = 0.0, g = 0.0;
    for (int i = t; i < f.m; i += 256) {
        c = c + f.Cp[i] * f.Cp[i];
        if (suf) g = g + f.Gm[i] * f.Gm[i];
    }
    c = wave_sum(c);
    g = wave_sum(g);
    if (lane == 0) { tred[0][wave] = c; tred[1][wave] = g; }
    __syncthreads();
    if (t == 0) {
        const double trp = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
        const double tb = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
        const double ld = (red[2][0] + red[2][1]) + (red[2][2] + red[2][3]);
        const double cc = (tred[0][0] + tred[0][1]) + (tred[0][2] + tred[0][3]);
        const double gg = (tred[1][0] + tred[1][1]) + (tred[1][2] + tred[1][3]);
        const double yy = f.yyn[0], n = f.yyn[1];
        const double nsf = n * f.sf2;
        const int nh = nl + 2;
        const double F = ((((-0.5 * n * 1.8378770664093453 - ld) - 0.5 * n * f.log_s2) - yy / (2.0 * f.s2))
                          + cc / (2.0 * f.s2 * f.s2)) - (nsf - trp) / (2.0 * f.s2);
        out[1 + nh] = F;
        hout[1 + nh] = F;
        out[0] = F;
        hout[0] = F;
        if (suf) {
            const double gf = -(2.0 * tail - nsf / f.s2);
            const double gn = -(((tb - n) + (((yy - cc / f.s2) + (nsf - trp)) / f.s2)) - gg / (f.s2 * f.s2));
            out[1 + nl] = gf; out[2 + nl] = gn;
            hout[1 + nl] = gf; hout[2 + nl] = gn;
        }
    }
}
