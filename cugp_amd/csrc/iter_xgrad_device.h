// iter_xgrad_device.h -- the test-input gradients of the matrix-free exact GP (cugp_iter_input_grad, cugp_iter_predict_grad;
// DESIGN.md section 37): sums over ALL n training rows of dk(x*, x_j) / dx* times a weight, at O(n) memory, G in registers.
// Plain fp64 arithmetic, LDS, __syncthreads and __shfl_xor: emulable (tools/iter_host_check.cpp runs this text behind
// tools/host_emul.h).  The launcher stands in iter_gfx950.h.
//
// Include-point contract.  Included INSIDE namespace cugp, after kernels.h (ITER_*, IT_MAXT, HyperScalars, KERNEL_*), the d2
// typedef and cov_device.h (DC, DivBy, div_prepare, div_by, ard_weights, ShapeArgs, shape_args, kernel_value, matern_entry,
// rq_entry).
//
// k_cov_xgrad<ARD, KIND, VAR>:  with dk_ij / dx*_ia = -G_ij (xt[i][a] - x[j][a]) s_a (cov_device.h, predict_grad_body's block),
//     pm[i][a] = sum_j (G_ij wm[j])         (xt[i][a] - x[j][a])      (always; wm is column 0 of an [n][16] block, or null: zeros)
//     pv[i][a] = sum_j (G_ij Wv[j][col(i)]) (xt[i][a] - x[j][a])      (VAR; Wv [n][tp], col(i) = i: one row block, nt <= tp)
//   G: kernel_value for SE and SE-ARD, hh of matern_entry for the Matern kinds, H of rq_entry for RQ: one exp per entry, nothing
//   divides by r.  k_cov_xgrad_finish applies -s_a (the mean's and the forms' sign) or +2 s_a (the variance's) once per output.
//   NO MFMA, on purpose.  The difference xt[i][a] - x[j][a] must be formed first and then multiplied: the GEMM-shaped form
//   x*_a sum(G w) - sum(G w x_a), which a matrix instruction would serve, cancels where |x| >> |x - x'|
//   (tests/truth_predict_grad.py keeps it as the mutation coordinate=True; its case n257_d3_shift and this kernel's shifted
//   test catch it).  So the lane that computes an entry also multiplies it, on the VALU.
//   Decomposition: k_cov_apply's.  Workgroup = 4 waves x 16 test rows (ITER_ROWS); lane (fr, fk) = (lane & 15, lane >> 4) owns
//   test row fr of its wave and, of each stage of ITER_JT = 32 training rows, the 8 entries j = 4 kk + fk.  The wave's test rows
//   sit in registers, DC features at a time.  The x rows of a stage go through the double-buffered LDS image ys, the stage's 32
//   mean weights through ws and (VAR) its Wv rows through vs; the next stage travels in registers behind the current one: one
//   barrier per stage.  vs rows are tp = 16 doubles apart (the two k rows of a half-wave's ds_read_b64 are adjacent: 64 banks)
//   or, tp = 64, XG_TPL = 80 (640 B = 128 B mod 256 B: the two rows' 16-double runs fall on different banks), as k_cov_apply's.
//   Per entry: the squared distance in k_cov_apply's arithmetic (differences before squares, feature order, no contraction:
//   the product's bits), G once, e_m = G wm[j], e_v = G Wv[j][c].  A second loop over the features of the workgroup's chunk
//   (blockIdx.z; read again from the stage's LDS image, ys or yz) forms df = a_c - b_c UNWEIGHTED and adds e_m df, e_v df into
//   DC (+ DC) per-lane sums that live across the whole sweep, j ascending.  Every z recomputes the whole distance (d > DC is
//   served, not tuned, as in k_cov_grad).
//   End of sweep: the four fk groups of a row add as (0 + 1) + (2 + 3) by two __shfl_xor (16, 32; a + b == b + a: all four hold
//   the same bits); the fk == 0 lanes write part[s][q][i][a], q = 0 mean, 1 variance.  grid (row blocks, split, feature chunks),
//   the split from iter_apply_plan; k_cov_xgrad_finish adds the ranges in ascending s (first copied, then a = a + b).
//   Rows beyond nt or n enter as zeros with zero weight and are never read; a wave whose 16 rows all lie beyond nt skips the
//   arithmetic and keeps the barriers.  No atomics, no scratch.  A row's bits depend on (X, theta, its x*, its weights, split)
//   only -- not on nt, on its place in a block or batch, or on the rows beside it: a lane owns one row from the first
//   difference to the last sum.
//   LDS: ys [2][32][16], yc, yz [32][16], ws [2][32] and (VAR) vs [2][32][80] doubles: 16.5 KiB | 56.5 KiB.
#pragma once

constexpr int XG_TPL = IT_MAXT + 16;    // the row stride of vs at tp = 64

// the radial factor G of dk / dx* from the squared distance (weighted: ARD), as predict_grad_body takes it
template <bool ARD, int KIND>
__device__ __forceinline__ double xgrad_factor(double sq, const DivBy& dl, double sf2, const ShapeArgs& sh)
{
    if constexpr (KIND == KERNEL_SE) {
        return kernel_value<ARD, KERNEL_SE>(sq, dl, sf2);
    } else if constexpr (KIND == KERNEL_RQ) {
        double kf, hh, da;
        rq_entry(sq, sf2, sh.alpha, sh.h2a, kf, hh, da);
        return hh;
    } else {
        double kf, dk, hh;
        matern_entry<KIND>(ARD ? sq : div_by(sq, dl), sf2, kf, dk, hh);
        return hh;
    }
}

template <bool ARD, int KIND, bool VAR>
__global__ __launch_bounds__(256) void k_cov_xgrad(const double* __restrict__ Xt, int nt, const double* __restrict__ X, int n, int d,
                                                   const HyperScalars* __restrict__ hd, const double* __restrict__ wm,
                                                   const double* __restrict__ Wv, int tp, double* __restrict__ part, int per)
{
#pragma clang fp contract(off)
    constexpr int NK = ITER_JT / 4, NQ = VAR ? 2 : 1;
    static_assert(ITER_JT * DC == 2 * 256 && ITER_JT * IT_MAXT == 2 * 256 * 4, "one d2 of x and at most four d2 of Wv per thread and stage");
    static_assert(ITER_JT == 32 && ITER_ROWS == 64, "8 entries per lane and stage, four waves of 16 test rows");
    __shared__ __attribute__((aligned(16))) double ys[2][ITER_JT][DC];
    __shared__ __attribute__((aligned(16))) double yc[ITER_JT][DC];
    __shared__ __attribute__((aligned(16))) double yz[ITER_JT][DC];
    __shared__ double ws[2][ITER_JT];
    __shared__ __attribute__((aligned(16))) double vs[VAR ? 2 * ITER_JT * XG_TPL : 2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fk = lane >> 4;
    const int row = blockIdx.x * ITER_ROWS + wave * 16 + fr;
    const bool live = blockIdx.x * ITER_ROWS + wave * 16 < nt;     // (the same for the 64 lanes of a wave)
    const HyperScalars h = *hd;
    const double* __restrict__ wts = ard_weights(hd);
    const DivBy dl = div_prepare(h.ell_sq);
    const ShapeArgs sh = shape_args<KIND>(wts, d);
    const int nst = (n + ITER_JT - 1) / ITER_JT, nch = (d + DC - 1) / DC;
    const int s0 = blockIdx.y * per, s1 = s0 + per < nst ? s0 + per : nst;
    const int cz = blockIdx.z;                         // the feature chunk of this workgroup's sums
    const int nct = tp / 16, tph = tp / 2, tpl = tp == 16 ? 16 : XG_TPL, col = wave * 16 + fr;

    double ar[DC];
    auto load_a = [&](int c0) {
#pragma unroll
        for (int c = 0; c < DC; c++) ar[c] = (row < nt && c0 + c < d) ? Xt[(size_t)row * d + c0 + c] : 0.0;
    };
    // the thread's share of a stage: one feature pair of one x row, a mean weight (32 threads), nct column pairs of Wv rows
    const int br = tid >> 3, bc = (tid & 7) * 2;
    d2 rb;
    double rw = 0.0;
    [[maybe_unused]] d2 rv[VAR ? 4 : 1];
    auto fetch_b = [&](int j0, int c0) {
        const int j = j0 + br, c = c0 + bc;
        rb[0] = (j < n && c < d) ? X[(size_t)j * d + c] : 0.0;
        rb[1] = (j < n && c + 1 < d) ? X[(size_t)j * d + c + 1] : 0.0;
    };
    auto fetch = [&](int st) {
        const int j0 = st * ITER_JT;
        fetch_b(j0, 0);
        if (tid < ITER_JT) rw = (wm && j0 + tid < n) ? wm[(size_t)(j0 + tid) * 16] : 0.0;
        if constexpr (VAR) {
#pragma unroll
            for (int q = 0; q < 4; q++)
                if (q < nct) {
                    const int e = tid + 256 * q, j = j0 + e / tph;
                    rv[q] = j < n ? *(const d2*)(Wv + (size_t)j * tp + 2 * (e % tph)) : (d2){0.0, 0.0};
                }
        }
    };
    auto put = [&](int buf) {
        *(d2*)&ys[buf][br][bc] = rb;
        if (tid < ITER_JT) ws[buf][tid] = rw;
        if constexpr (VAR) {
#pragma unroll
            for (int q = 0; q < 4; q++)
                if (q < nct) {
                    const int e = tid + 256 * q;
                    *(d2*)&vs[(buf * ITER_JT + e / tph) * tpl + 2 * (e % tph)] = rv[q];
                }
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
    double gm[DC];                                     // sum_j e_m (a_c - b_c) for the DC features of chunk cz
    [[maybe_unused]] double gv[VAR ? DC : 1];          // ... e_v
#pragma unroll
    for (int c = 0; c < DC; c++) gm[c] = 0.0;
#pragma unroll
    for (int c = 0; c < (VAR ? DC : 1); c++) gv[c] = 0.0;

    load_a(0);
    fetch(s0);
    put(0);
    __syncthreads();
    for (int st = s0; st < s1; st++) {
        const int cur = (st - s0) & 1;
        const bool more = st + 1 < s1;
        if (more) fetch(st + 1);
        if (live) {
#pragma unroll
            for (int kk = 0; kk < NK; kk++) sq[kk] = 0.0;
            accumulate(ys[cur], 0);
        }
        for (int ch = 1; ch < nch; ch++) {
            const d2 keep = rb;
            fetch_b(st * ITER_JT, ch * DC);
            __syncthreads();
            *(d2*)&yc[br][bc] = rb;
            if (ch == cz) *(d2*)&yz[br][bc] = rb;
            rb = keep;
            if (live) load_a(ch * DC);
            __syncthreads();
            if (live) accumulate(yc, ch * DC);
        }
        if (live) {
            if (nch > 1) load_a(cz * DC);
            double em[NK];
            [[maybe_unused]] double ev[VAR ? NK : 1];
#pragma unroll
            for (int kk = 0; kk < NK; kk++) {
                const double g = xgrad_factor<ARD, KIND>(sq[kk], dl, h.signal_var, sh);
                em[kk] = g * ws[cur][kk * 4 + fk];
                if constexpr (VAR) ev[kk] = g * vs[(cur * ITER_JT + kk * 4 + fk) * tpl + col];
            }
            double (*yb)[DC] = cz == 0 ? ys[cur] : yz;
#pragma unroll
            for (int cp = 0; cp < DC / 2; cp++) {
                const int c = 2 * cp;
                if (cz * DC + c < d) {
#pragma unroll
                    for (int kk = 0; kk < NK; kk++) {
                        const d2 yv = *(const d2*)&yb[kk * 4 + fk][c];
                        double df = ar[c] - yv[0];
                        gm[c] = gm[c] + em[kk] * df;
                        if constexpr (VAR) gv[c] = gv[c] + ev[kk] * df;
                        df = ar[c + 1] - yv[1];
                        gm[c + 1] = gm[c + 1] + em[kk] * df;
                        if constexpr (VAR) gv[c + 1] = gv[c + 1] + ev[kk] * df;
                    }
                }
            }
            if (cz != 0) load_a(0);
        }
        if (more) put(cur ^ 1);
        __syncthreads();
    }
    if (!live) return;
    // the row's four fk groups: (0 + 1) + (2 + 3), the same bits in all four
    double* __restrict__ o = part + (size_t)blockIdx.y * NQ * nt * d + (size_t)row * d + cz * DC;
#pragma unroll
    for (int c = 0; c < DC; c++) {
        double g = gm[c];
        g = g + __shfl_xor(g, 16, 64);
        g = g + __shfl_xor(g, 32, 64);
        [[maybe_unused]] double v = 0.0;
        if constexpr (VAR) {
            v = gv[c];
            v = v + __shfl_xor(v, 16, 64);
            v = v + __shfl_xor(v, 32, 64);
        }
        if (fk == 0 && row < nt && cz * DC + c < d) {
            o[c] = g;
            if constexpr (VAR) o[(size_t)nt * d + c] = v;
        }
    }
}

// outm[e] = -s_c (P_0 + P_1 + ...), outv[e] = (fv s_c) (Q_0 + Q_1 + ...), e = i d + c < cnt = nt d: the ranges' partial sums in
// ascending s (first copied, then a = a + b); part [split][nq][nt][d], Q the blocks q = 1 (nq == 2 where outv is given).
// s_c = w_c^2 on the ARD route (a tied rational quadratic handle: its equal weights), else 1 / l^2.  fv: +2 for the variance's
// gradient, -1 for a form.  Either output may be null.
__global__ __launch_bounds__(256) void k_cov_xgrad_finish(const double* __restrict__ part, int split, int nq, size_t cnt, int d,
                                                          const HyperScalars* __restrict__ hd, int route, double fv,
                                                          double* __restrict__ outm, double* __restrict__ outv)
{
#pragma clang fp contract(off)
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= cnt) return;
    const int c = (int)(e % d);
    const double* __restrict__ wts = ard_weights(hd);
    const double sc = route ? wts[c] * wts[c] : 1.0 / hd->ell_sq;
    if (outm) {
        double s = part[e];
        for (int k = 1; k < split; k++) s = s + part[(size_t)k * nq * cnt + e];
        outm[e] = -(sc * s);
    }
    if (outv) {
        double s = part[cnt + e];
        for (int k = 1; k < split; k++) s = s + part[((size_t)k * nq + 1) * cnt + e];
        outv[e] = (fv * sc) * s;
    }
}
