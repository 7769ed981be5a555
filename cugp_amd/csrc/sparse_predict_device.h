// sparse_predict_device.h -- the one elementwise pass of the sparse model's input gradients (cugp_sparse_predict_grad;
// DESIGN.md section 28).  Plain fp64 arithmetic: no MFMA, no atomics, no shuffles, no inline assembly and no #ifdef around
// arithmetic -- the host check (tools/sparse_joint_host_check.cpp) runs this text behind tools/host_emul.h under
// -fsanitize=address,undefined.
//
// Include-point contract: sparse_device.h's (inside namespace cugp, behind kernels.h and the device vocabulary).
#pragma once

// D = Wt - T over the first `rows` rows ([rows][ld] each, rows a multiple of 64: the whole tiles launch_targets_alpha
// reads), T = Vt LB^-1, so that U = D Lu^-1 = (Wt - Vt LB^-1) Lu^-1; and (a given) a[i] = bp[i] / s2 for i < m, 0.0 up to
// ld: the weights of the mean's gradient, a = beta' / s2.  One entry per thread, one rounding each: nothing is summed, so
// there is no order to fix.  bp is read in [0, m) only; Wt and T in their first `rows` rows only.  D null (no variance
// gradient asked for): a alone, Wt and T unread.
// Grid: ceil(max(rows * ld, ld) / 256).
__global__ __launch_bounds__(256) void k_sparse_predict_diff(const double* __restrict__ Wt, const double* __restrict__ T,
                                                             double* __restrict__ D, int ld, int rows,
                                                             const double* __restrict__ bp, double s2, int m,
                                                             double* __restrict__ a)
{
#pragma clang fp contract(off)
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (D && e < (size_t)rows * ld) D[e] = Wt[e] - T[e];
    if (a && e < (size_t)ld) a[e] = e < (size_t)m ? bp[e] / s2 : 0.0;
}
