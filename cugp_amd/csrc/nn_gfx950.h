// nn_gfx950.h -- the nearest-neighbour (Vecchia) GP (cugp_nn_*): one WAVEFRONT factors one
// conditioning block from gather to result, the factor in registers, one row per lane.
//
// Include-point contract.  Included INSIDE namespace cugp by kernels.hip, after kernels.h (CovFn, HyperScalars, KERNEL_*),
// CUGP_COV_KERNEL, cov_device.h (DC, wave_sum, DivBy, div_prepare, div_by, ard_weights, ShapeArgs, shape_args, ard_entry,
// matern_entry, kernel_value) and chol_gfx950.h (readlane_f64).
//
// k_nn_block<MP, ARD, KIND, MODE>.  Block `b` (training row b, or test point b in the prediction mode) is the MP x MP matrix
//   C = k(P, P) + sn2 I over its points P: position MP - 1 is the block's OWN point, positions MP - 1 - m .. MP - 2 the m slots
//   of its index row, and every position whose slot is -1 or that lies in front of the slots is PADDING: an identity row with
//   y = 0, which factors to itself, adds log 1 and z = 0 and couples with nothing.  The own point is therefore always row
//   MP - 1: every index into the factor is static.
//   Lanes: MP = 64: lane r owns row r.  MP = 32: a wavefront carries two blocks, MP = 16: four (lane = sub MP + r), so all 64
//   lanes hold a row at every size; broadcasts are v_readlane pairs at MP = 64, two of them and a select at MP = 32 (with
//   ds_bpermute broadcasts, whose results are VGPR pairs, the 32-row kernels needed 512 registers and spilled; through SGPRs
//   they need 141 to 267 and no scratch), and __shfl over the 16-lane group at MP = 16.
//   A 256-thread workgroup runs four wavefronts; they share nothing until the sums at the end.
//   (1) gather: every lane loads its point's coordinates, DC features at a time, into the wavefront's LDS image [64][DC + 1];
//       lane r adds ((x_r - x_c) w)^2 for ALL c < MP in feature order, differences before squares, no contraction
//       (sqdist_4x4's arithmetic), the other point read from LDS (a broadcast read at MP = 64).
//   (2) entries by kernel_value as it stands; c < r between two real points is kept, the diagonal is sf2 + sn2 (padding: 1),
//       everything else 0.  MP doubles per lane: the row of the factor.
//   (3) right-looking Cholesky, fully unrolled: step k broadcasts the pivot from lane k, every lane divides its column-k entry
//       (one real division per step: div_prepare / div_by), the forward substitution z = L^-1 y rides in the same step, and
//       the trailing update takes column k's entry of lane c by one broadcast per c > k.  A pivot that is not above 2^-44 (sf2
//       + sn2) has no digit left: NaN from there on (the header's convention for a matrix that is not positive definite).
//   (4) value: l = -1/2 (z_last^2 + 2 log L_last,last + 1.83787) (the library's literal for log 2 pi).  Prediction: y_own = 0,
//       mean = -z_last L_last,last, var = L_last,last^2 (- sn2).
//   (5) gradient: the two back-substitutions need COLUMNS of L.  The rows go once through a packed lower-triangle LDS image
//       (MP (MP + 1) / 2 doubles per block, 16.6 KB per wavefront at MP = 64; it aliases the coordinate image) and come back
//       as columns, MP doubles per lane again; p = L^-T [z_N; 0] = pad(alpha_N) and u = L^-T e_last then run as (3)'s
//       forward substitution does, one broadcast pair per step.  With a = p + z_last u:
//         dW_rc = a_r a_c - p_r p_c - u_r u_c = z_last (p_r u_c + u_r p_c) + (z_last^2 - 1) u_r u_c       (no cancellation)
//       Lane r contracts row r, c <= r, with the derivative factors, which are RECOMPUTED (a second distance sweep and one
//       more ard_entry / matern_entry per entry) rather than kept: keeping them would double the MP doubles per lane.
//       ARD: dW_rc hh_rc replaces the entries and a third sweep over the features forms the d per-dimension sums.
//   Sums: lanes by wave_sum, the four wavefronts in index order through LDS; one partial row [l, columns] per WORKGROUP in
//   part[blockIdx.x][1 + ncol], columns as the trace partials' ([length: 1 | d][shape][sf][sn]).  k_nn_finish adds the rows in
//   ascending order (first copied, then a = a + b), folds a tied handle's d length columns and changes the gradient's sign (g
//   is d(-L)/dtheta).  No atomics: equal inputs give equal bits.
//   Reads: idx only inside [rows][m], X only at validated indices (nn.cpp checks them when they are set), Xt and y below
//   rows; wavefronts beyond the last block run on padding alone and write nothing.
#pragma once

constexpr int NN_XS = DC + 1;                       // row stride of the coordinate image
constexpr int NN_IMG = 64 * NN_XS;                  // doubles of a wavefront's coordinate image
constexpr int nn_tri(int mp) { return mp * (mp + 1) / 2; }
// doubles of LDS per wavefront: the coordinate image, and in the gradient mode the packed factor image it aliases
constexpr int nn_lds(int mp, int mode)
{
    return mode == NN_GRAD && (64 / mp) * nn_tri(mp) > NN_IMG ? (64 / mp) * nn_tri(mp) : NN_IMG;
}

// lane c's value within the lane's MP-lane group
template <int MP>
__device__ __forceinline__ double nn_bcast(double v, int c)
{
    if constexpr (MP == 64) return readlane_f64(v, c);
    else if constexpr (MP == 32) {                    // both blocks' values through SGPRs, as at 64 rows, then one select
        const double lo = readlane_f64(v, c), hi = readlane_f64(v, 32 + c);
        return (threadIdx.x & 32) ? hi : lo;
    } else return __shfl(v, c, MP);
}

// LDS written by one lane of the wavefront, read by another: wait for it, and keep the compiler from moving accesses across
__device__ __forceinline__ void nn_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

template <int MP, bool ARD, int KIND, int MODE>
__global__ __launch_bounds__(256) void k_nn_block(const double* __restrict__ X, const double* __restrict__ y,
                                                  const int* __restrict__ idx, const double* __restrict__ Xt, int rows, int m,
                                                  int d, const HyperScalars* __restrict__ hd, double* __restrict__ part,
                                                  double* __restrict__ mean, double* __restrict__ var, int with_noise)
{
#pragma clang fp contract(off)
    static_assert(MP == 16 || MP == 32 || MP == 64, "padded block sizes");
    static_assert(ARD || KIND != KERNEL_RQ, "the rational quadratic kernel has ARD instantiations only");
    constexpr int TRI = nn_tri(MP), NS = shape_count(KIND);
    __shared__ double lds[4][nn_lds(MP, MODE)];
    __shared__ double red[DC > 5 ? DC : 5][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g0 = lane & ~(MP - 1), r = lane & (MP - 1);         // first lane of the lane's block, row inside it
    const long long blk = ((long long)blockIdx.x * 4 + wave) * (64 / MP) + lane / MP;
    const bool live = blk < rows, own = r == MP - 1;
    double* img = lds[wave];

    const HyperScalars h = *hd;
    const double* __restrict__ wts = ard_weights(hd);
    const DivBy dl = div_prepare(h.ell_sq);
    ShapeArgs sh = ShapeArgs{0.0, 0.0};
    if constexpr (KIND == KERNEL_RQ) sh = shape_args<KIND>(wts, d);
    const double sf2 = h.signal_var, sn2 = h.noise_var, dg = sf2 + sn2;

    // the lane's point: its coordinates and label, or padding
    const double* xrow = nullptr;
    double yv = 0.0;
    if (live) {
        if (own) {
            xrow = (MODE == NN_PREDICT ? Xt : X) + (size_t)blk * d;
            if (MODE != NN_PREDICT) yv = y[blk];
        } else if (r >= MP - 1 - m) {
            const int j = idx[(size_t)blk * m + (r - (MP - 1 - m))];
            if (j >= 0) { xrow = X + (size_t)j * d; yv = y[j]; }
        }
    }
    const bool pad = xrow == nullptr;
    const unsigned long long padmask = __ballot(pad);
    auto padded = [&](int c) { return ((padmask >> (g0 + c)) & 1ull) != 0; };

    double A[MP];
    // features [c0, c0 + dc) of every lane's point into the wavefront's image (padding: zeros)
    auto stage = [&](int c0, int dc) {
        nn_wave_sync();
        for (int f = 0; f < dc; f++) img[lane * NN_XS + f] = pad ? 0.0 : xrow[c0 + f];
        nn_wave_sync();
    };
    // A[c] = sum_f ((x_r - x_c) w_f)^2, every c
    auto sqdist = [&]() {
#pragma unroll
        for (int c = 0; c < MP; c++) A[c] = 0.0;
        for (int c0 = 0; c0 < d; c0 += DC) {
            const int dc = (d - c0 < DC) ? (d - c0) : DC;
            stage(c0, dc);
            for (int f = 0; f < dc; f++) {
                const double xr = img[lane * NN_XS + f];
                const double wf = ARD ? wts[c0 + f] : 1.0;
#pragma unroll
                for (int c = 0; c < MP; c++) {
                    double df = xr - img[(g0 + c) * NN_XS + f];
                    if (ARD) df = df * wf;
                    A[c] = A[c] + df * df;
                }
            }
        }
    };

    sqdist();
#pragma unroll
    for (int c = 0; c < MP; c++) {
        const double kf = kernel_value<ARD, KIND>(A[c], dl, sf2, sh);
        A[c] = (c < r && !pad && !padded(c)) ? kf : (c == r ? (pad ? 1.0 : dg) : 0.0);
    }

    // the factor, row r in A; z = L^-1 y in yv
    const double thr = dg * 0x1p-44;
    double piv = 1.0, zl = 0.0;
#pragma unroll
    for (int k = 0; k < MP; k++) {
        const double akk = nn_bcast<MP>(A[k], k);
        piv = akk > (padded(k) ? 0.0 : thr) ? sqrt(akk) : __builtin_nan("");
        const DivBy dp = div_prepare(piv);
        const double lk = r > k ? div_by(A[k], dp) : (r == k ? piv : 0.0);
        A[k] = lk;
        zl = div_by(nn_bcast<MP>(yv, k), dp);
        yv = r == k ? zl : __builtin_fma(-lk, zl, yv);
#pragma unroll
        for (int c = k + 1; c < MP; c++) A[c] = __builtin_fma(-lk, nn_bcast<MP>(lk, c), A[c]);
    }
    // piv = L_last,last and zl = z_last of the lane's block

    if constexpr (MODE == NN_PREDICT) {
        if (own && live) {
            mean[blk] = -(zl * piv);
            var[blk] = with_noise ? piv * piv : piv * piv - sn2;
        }
        return;
    }

    const bool mine = own && live;
    double sums[5] = {mine ? -0.5 * ((zl * zl + 2.0 * log(piv)) + 1.83787) : 0.0, 0.0, 0.0, 0.0, 0.0};   // l, length, shape, sf, sn
    if constexpr (MODE == NN_GRAD) {
        // rows of L -> packed LDS image -> columns: A[rr] = L[rr][r], rr >= r
        double* tri = img + (lane / MP) * TRI;
        nn_wave_sync();
#pragma unroll
        for (int c = 0; c < MP; c++)
            if (c <= r) tri[r * (r + 1) / 2 + c] = A[c];
        nn_wave_sync();
#pragma unroll
        for (int rr = 0; rr < MP; rr++) A[rr] = rr >= r ? tri[rr * (rr + 1) / 2 + r] : 0.0;
        // p = L^-T [z_N; 0], u = L^-T e_last
        double p = own ? 0.0 : yv, u = own ? 1.0 : 0.0;
#pragma unroll
        for (int rr = MP - 1; rr >= 0; rr--) {
            const DivBy dd = div_prepare(nn_bcast<MP>(A[rr], rr));
            const double xp = div_by(nn_bcast<MP>(p, rr), dd), xu = div_by(nn_bcast<MP>(u, rr), dd);
            const double t = r < rr ? A[rr] : 0.0;
            p = r == rr ? xp : __builtin_fma(-t, xp, p);
            u = r == rr ? xu : __builtin_fma(-t, xu, u);
            }
        const double zz = zl * zl - 1.0;
        sqdist();
#pragma unroll
        for (int c = 0; c < MP; c++) {
            const double uc = nn_bcast<MP>(u, c), pc = nn_bcast<MP>(p, c);
            const double w = zl * (p * uc + u * pc) + zz * (u * uc);
            const bool offd = c < r && !pad && !padded(c);
            double kf, dk = 0.0, hh = 0.0, da = 0.0;
            if constexpr (ARD) {
                ard_entry<KIND>(A[c], sf2, sh, kf, hh, da);
            } else if constexpr (KIND == KERNEL_SE) {
                kf = kernel_value<ARD, KIND>(A[c], dl, sf2, sh);
                dk = kf * div_by(A[c], dl);
            } else {
                matern_entry<KIND>(div_by(A[c], dl), sf2, kf, dk, hh);
            }
            if (offd) {
                sums[1] += w * dk;
                if constexpr (NS > 0) sums[2] += w * da;
                sums[3] += 2.0 * (w * kf);
            } else if (c == r && !pad) {
                sums[3] += w * sf2;
                sums[4] += w * sn2;
            }
            A[c] = (ARD && offd) ? w * hh : 0.0;
            }
    }

    // the workgroup's row: lanes by wave_sum, the wavefronts in index order
    double* row = part + (size_t)blockIdx.x * (MODE == NN_GRAD ? 1 + (ARD ? d : 1) + NS + 2 : 1);
    constexpr int NSUM = MODE == NN_GRAD ? 5 : 1;
#pragma unroll
    for (int j = 0; j < NSUM; j++) {
        const double s = wave_sum(sums[j]);
        if (lane == 0) red[j][wave] = s;
    }
    __syncthreads();
    if (tid < NSUM) {
        const double s = (red[tid][0] + red[tid][1]) + (red[tid][2] + red[tid][3]);
        const int nl = ARD ? d : 1;                             // [l][length nl][shape NS][sf][sn]
        if (tid == 0) row[0] = s;
        else if (tid == 1) { if (!ARD) row[1] = s; }
        else if (tid == 2) { if (NS > 0) row[1 + nl] = s; }
        else row[1 + nl + NS + (tid - 3)] = s;
    }
    if constexpr (MODE == NN_GRAD && ARD) {
        // g_f = sum_c (dW hh)_rc ((x_rf - x_cf) w_f)^2, DC dimensions at a time
        for (int c0 = 0; c0 < d; c0 += DC) {
            const int dc = (d - c0 < DC) ? (d - c0) : DC;
            __syncthreads();                                    // red is free again
            stage(c0, dc);
            for (int f = 0; f < dc; f++) {
                const double xr = img[lane * NN_XS + f], wf = wts[c0 + f];
                double acc = 0.0;
#pragma unroll
                for (int c = 0; c < MP; c++) {
                    const double df = (xr - img[(g0 + c) * NN_XS + f]) * wf;
                    acc = acc + A[c] * (df * df);
                }
                acc = wave_sum(acc);
                if (lane == 0) red[f][wave] = acc;
            }
            __syncthreads();
            if (tid < dc) row[1 + c0 + tid] = (red[tid][0] + red[tid][1]) + (red[tid][2] + red[tid][3]);
        }
    }
}

// out[0] = the sum of the workgroups' l; out[1 .. nh] = -(the columns' sums), a tied handle's nlen length columns added in
// index order into out[1]; rows ascending: first copied, then a = a + b.  One workgroup; work: nc doubles behind out's row.
__global__ __launch_bounds__(256) void k_nn_finish(const double* __restrict__ part, int nparts, int nc, int fold,
                                                   double* __restrict__ out, double* __restrict__ work)
{
#pragma clang fp contract(off)
    for (int c = threadIdx.x; c < nc; c += 256) {
        double s = part[c];
        for (int b = 1; b < nparts; b++) s = s + part[(size_t)b * nc + c];
        work[c] = s;
    }
    __syncthreads();
    const int nout = fold > 1 ? nc - fold + 1 : nc;
    for (int o = threadIdx.x; o < nout; o += 256) {
        if (o == 0) out[0] = work[0];
        else if (fold > 1 && o == 1) {
            double s = work[1];
            for (int c = 1; c < fold; c++) s = s + work[1 + c];
            out[1] = -s;
        } else out[o] = -work[fold > 1 ? o + fold - 1 : o];
    }
}

// ---- launchers ----
int nn_block_size(int m) { return m + 1 <= 16 ? 16 : (m + 1 <= 32 ? 32 : 64); }
int nn_workgroups(int rows, int m) { const int per = 4 * (64 / nn_block_size(m)); return (rows + per - 1) / per; }

#define CUGP_NN_CASE(MPV, MODEV)                                                                                            \
    if (mp == MPV && mode == MODEV) {                                                                                       \
        hipLaunchKernelGGL((k_nn_block<MPV, ARD, KIND, MODEV>), grid, dim3(256), 0, s, X, y, idx, Xt, rows, m, d, hd, part, \
                           mean, var, with_noise);                                                                          \
        return;                                                                                                             \
    }
template <bool ARD, int KIND>
static void nn_launch(int mp, int mode, dim3 grid, hipStream_t s, const double* X, const double* y, const int* idx,
                      const double* Xt, int rows, int m, int d, const HyperScalars* hd, double* part, double* mean, double* var,
                      int with_noise)
{
    CUGP_NN_CASE(16, NN_VALUE) CUGP_NN_CASE(16, NN_GRAD) CUGP_NN_CASE(16, NN_PREDICT)
    CUGP_NN_CASE(32, NN_VALUE) CUGP_NN_CASE(32, NN_GRAD) CUGP_NN_CASE(32, NN_PREDICT)
    CUGP_NN_CASE(64, NN_VALUE) CUGP_NN_CASE(64, NN_GRAD) CUGP_NN_CASE(64, NN_PREDICT)
}
#undef CUGP_NN_CASE

void launch_nn_block(int mode, const double* X, const double* y, const int* idx, const double* Xt, int rows, int m, int d,
                     const CovFn& cf, double* part, double* mean, double* var, int with_noise, hipStream_t s)
{
    const auto fn = CUGP_COV_KERNEL(cf, nn_launch);
    fn(nn_block_size(m), mode, dim3(nn_workgroups(rows, m)), s, X, y, idx, Xt, rows, m, d, cf.hd, part, mean, var, with_noise);
}

void launch_nn_finish(const double* part, int nparts, int nc, int fold, double* out, double* work, hipStream_t s)
{
    hipLaunchKernelGGL(k_nn_finish, dim3(1), dim3(256), 0, s, part, nparts, nc, fold, out, work);
}
