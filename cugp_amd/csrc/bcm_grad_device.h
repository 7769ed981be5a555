// bcm_grad_device.h -- the test-input gradient of a product of experts (cugp_bcm_predict_grad, the form across ranks):
// the batched twins of k_predict_grad / k_predict_grad_finish, one launch for the experts of a group, and the chain rule
// of the combination on the device.  Plain fp64 arithmetic on cov_device.h's bodies: emulable on a host like that file
// (tools/bcm_predict_grad_host_check.cpp), and under its rules -- no #ifdef around arithmetic.
//
// Include-point contract: INSIDE namespace cugp, directly after cov_device.h (predict_grad_body, KT,
// ExpertPtrs, GP).
//
// Rows of one expert, wherever they travel (device scratch, pinned host memory, the exchange's slots):
//   [m nt | v nt | dmean nt*d | dvar nt*d]        (2 + 2 d) nt doubles; dvar is left untouched when it is not wanted
#pragma once

// k_predict_grad for the experts of a group: blockIdx.y selects the expert -- X, n and alpha from its table entry, Ks, V
// and the partial sums its own slices (kslice, pslice doubles apart); ARD reads the group's one hd.  The experts share
// npad but not n, and the body derives its tile split from its own n: the grid is sized for the expert with the most
// 64-row training tiles, and a workgroup beyond its expert's tiles_t x tiles_i returns before the body (uniformly: no
// thread of it reaches a barrier).  The arithmetic per expert is the single launch's: predict_grad_body unchanged.
template <bool ARD, int KIND>
__global__ __launch_bounds__(256) void k_predict_grad_batched(int d, int npad, const double* __restrict__ Xt, int nt,
                                                              HyperScalars h_arg, const double* __restrict__ Ks,
                                                              const double* __restrict__ V, size_t kslice,
                                                              double* __restrict__ part, size_t pstride, size_t pslice,
                                                              const HyperScalars* __restrict__ hd,
                                                              const ExpertPtrs* __restrict__ bt)
{
    const ExpertPtrs& e = bt[blockIdx.y];
    const int n = e.n;
    const int tiles_t = (nt + KT - 1) / KT, tiles_i = (n + KT - 1) / KT;
    if ((int)blockIdx.x >= tiles_t * tiles_i) return;
    predict_grad_body<ARD, KIND>(GP(e.X), n, d, npad, Xt, nt, h_arg, Ks + (size_t)blockIdx.y * kslice,
                                 V ? V + (size_t)blockIdx.y * kslice : nullptr, GP(e.alpha),
                                 part + (size_t)blockIdx.y * pslice, pstride, hd);
}

// k_predict_grad_finish for the experts of a group: each expert sums its OWN number of tiles, in tile order, and writes
// straight into its rows: dmean + blockIdx.y * row_stride (dvar alike; null: the mean's gradient alone).  The lines are
// k_predict_grad_finish's, repeated rather than shared through a function: inlining one into that kernel reordered its
// instructions, and the kernels that exist keep theirs.  The host check holds the two to the same bits.
__global__ __launch_bounds__(256) void k_predict_grad_finish_batched(const double* __restrict__ part, size_t pstride,
                                                                     size_t pslice, int nt, int d, double ell_sq,
                                                                     const double* __restrict__ wts,
                                                                     double* __restrict__ dmean, double* __restrict__ dvar,
                                                                     size_t row_stride, const ExpertPtrs* __restrict__ bt)
{
#pragma clang fp contract(off)
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)nt * d) return;
    const int tiles = (bt[blockIdx.y].n + KT - 1) / KT;
    part += (size_t)blockIdx.y * pslice;
    dmean += (size_t)blockIdx.y * row_stride;
    if (dvar) dvar += (size_t)blockIdx.y * row_stride;
    const int c = (int)(e % d);
    const double sc = wts ? wts[c] * wts[c] : 1.0 / ell_sq;
    double sm = part[e], sv = dvar ? part[pstride + e] : 0.0;
    for (int ti = 1; ti < tiles; ti++) {
        sm = sm + part[(size_t)ti * 2 * pstride + e];
        if (dvar) sv = sv + part[((size_t)ti * 2 + 1) * pstride + e];
    }
    dmean[e] = -(sc * sm);
    if (dvar) dvar[e] = (2.0 * sc) * sv;
}

// The combined prediction and its gradients over the gathered exchange buffer (comm.cpp: cugp_bcm_predict_grad_allgather).
// g: [world][rstride] doubles, rank r's block = {status, local expert count, [per] rows as above}.  One thread per (t, c);
// the experts k = 0..K-1 in GLOBAL order -- expert k is rank k mod world's (k / world)-th.  Device twin of the host path of
// cugp_bcm_predict_grad (bcm.cpp), operation by operation, every one rounded on its own:
//   mean, var   p = 1 / v, pm = p m (poe_row), then cugp_poe_combine's sums, prec, 1 / prec, mean = tv spm, var = tv
//               (+ sn2 when with_noise); mode -1 (CUGP_COMBINE_REFERENCE): the two sums of cugp_bcm_predict_partial and
//               cugp_poe_finish -- POE's operations on the noisy rows, no sn2
//   dmean, dvar cugp_poe_combine_grad's operations in its order; p_k, beta_k, prec, mu and w_k are recomputed over the
//               experts by every thread instead of kept in K-long arrays (the same arithmetic: nothing is reassociated)
// The thread with c == 0 writes mean[t] and var[t].  want_dvar == 0: out's dvar part is not written (the experts' dvar
// is still read: the mean's gradient needs it in every mode).
// out: [mean nt | var nt | dmean nt*d | dvar nt*d | world x {status, count}], the status words copied as k_poe_reduce's.
__global__ __launch_bounds__(256) void k_poe_reduce_grad(const double* __restrict__ g, size_t rstride, int world, int K,
                                                         int nt, int d, int mode, double sf2, double sn2, int with_noise,
                                                         int want_dvar, double* __restrict__ out)
{
#pragma clang fp contract(off)
    const size_t nd = (size_t)nt * d, slot = (2 + 2 * (size_t)d) * nt, words = 2 * (size_t)nt + 2 * nd;
    if (blockIdx.x == 0)
        for (int r = threadIdx.x; r < world; r += 256) {
            out[words + 2 * r] = g[(size_t)r * rstride];
            out[words + 2 * r + 1] = g[(size_t)r * rstride + 1];
        }
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= nd) return;
    const size_t t = e / d;
    const bool prior = mode >= 2, rbcm = mode == 3;
    const double bg = 1.0 / (double)K;
    double sp = 0.0, spm = 0.0, sb = 0.0;
    for (int k = 0; k < K; k++) {
        const double* b = g + (size_t)(k % world) * rstride + 2 + (size_t)(k / world) * slot;
        const double p = 1.0 / b[nt + t], pm = p * b[t];
        double beta = 1.0;
        if (mode == 1) beta = bg;
        else if (rbcm) beta = 0.5 * log(sf2 * p);
        sp = sp + beta * p;
        spm = spm + beta * pm;
        sb = sb + beta;
    }
    double prec = sp;
    if (prior) prec = sp + (1.0 - sb) / sf2;
    if (e == t * d) {
        const double tv = 1.0 / prec;
        out[t] = tv * spm;
        out[nt + t] = (mode >= 0 && with_noise) ? tv + sn2 : tv;
    }
    double mu = 0.0;
    for (int k = 0; k < K; k++) {
        const double* b = g + (size_t)(k % world) * rstride + 2 + (size_t)(k / world) * slot;
        const double p = 1.0 / b[nt + t];
        double beta = 1.0;
        if (mode == 1) beta = bg;
        else if (rbcm) beta = 0.5 * log(sf2 * p);
        const double w = (beta * p) / prec;
        mu = mu + w * b[t];
    }
    double dprec = 0.0, sdm = 0.0, sam = 0.0, sdb = 0.0;
    for (int k = 0; k < K; k++) {
        const double* b = g + (size_t)(k % world) * rstride + 2 + (size_t)(k / world) * slot;
        const double m = b[t], v = b[nt + t], dm = b[2 * (size_t)nt + e], dv = b[2 * (size_t)nt + nd + e];
        const double p = 1.0 / v;
        double beta = 1.0;
        if (mode == 1) beta = bg;
        else if (rbcm) beta = 0.5 * log(sf2 * p);
        const double w = (beta * p) / prec;
        double a = beta * -(dv / (v * v));
        if (rbcm) {
            const double db = -0.5 * (dv / v);
            a = db * p + a;
            sdb = sdb + db;
        }
        dprec = dprec + a;
        sdm = sdm + w * dm;
        sam = sam + a * (m - mu);
    }
    double dmo = sdm + sam / prec;
    if (prior) {
        const double pr = sdb / sf2;
        dprec = dprec - pr;
        dmo = dmo + (mu * pr) / prec;
    }
    out[2 * (size_t)nt + e] = dmo;
    if (want_dvar) out[2 * (size_t)nt + nd + e] = -(dprec / (prec * prec));
}
