// la.cpp -- the stand-alone dense-LA calls on a caller's matrix, and the bench / test hooks that time single kernels.
#include <algorithm>
#include <cstring>
#include <vector>

#include "handle.h"

using namespace cugp;

// a handle whose A holds a caller matrix (identity padded) instead of a kernel build
static int la_handle(int n, const double* K, const double* y, int device, cugp_gp** out)
{
    int rc = cugp_create(n, 1, device, out);
    if (rc) return rc;
    cugp_gp* g = *out;
    if ((rc = ensure_factor_bufs(g)) || (rc = ensure_inverse_bufs(g))) { cugp_destroy(g); return rc; }
    std::vector<double> pad((size_t)g->npad * g->npad, 0.0);
    for (int i = 0; i < g->npad; i++) {
        if (i < n) memcpy(&pad[(size_t)i * g->npad], K + (size_t)i * n, (size_t)n * sizeof(double));
        else pad[(size_t)i * g->npad + i] = 1.0;
    }
    hipError_t e = hipMemcpy(g->dA, pad.data(), pad.size() * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(g->dy, 0, (size_t)g->npad * sizeof(double));
    if (e == hipSuccess && y) e = hipMemcpy(g->dy, y, (size_t)n * sizeof(double), hipMemcpyHostToDevice);
    if (e != hipSuccess) { cugp_destroy(g); return fail(CUGP_ERR_DEVICE, "la upload", e); }
    return CUGP_OK;
}

int cugp::la_factor_inverse(cugp_gp* g, bool inverse)
{
    int rc;
    TuneScope ts(g);
    if ((rc = enqueue_potrf(g, inverse))) return rc;
    HIPCHK(hipStreamSynchronize(g->stream));
    if (barrier_expired(g->hout)) return fail(CUGP_ERR_DEVICE, "a stage barrier of k_trtri_block ran out of polls");
    g->factor_valid = true;
    g->inverse_valid = inverse;
    return CUGP_OK;
}

int cugp_potrf(int n, const double* K, double* L, int device)
{
    if (n <= 0 || !K || !L) return CUGP_ERR_INVALID;
    cugp_gp* g = nullptr;
    int rc = la_handle(n, K, nullptr, device, &g);
    if (rc) return rc;
    if (!(rc = la_factor_inverse(g, false))) rc = cugp_get_cholesky(g, L);
    cugp_destroy(g);
    return rc;
}

int cugp_potri(int n, const double* K, double* Kinv, int device)
{
    if (n <= 0 || !K || !Kinv) return CUGP_ERR_INVALID;
    cugp_gp* g = nullptr;
    int rc = la_handle(n, K, nullptr, device, &g);
    if (rc) return rc;
    if (!(rc = la_factor_inverse(g, true))) rc = cugp_get_K_inverse(g, Kinv);
    cugp_destroy(g);
    return rc;
}

static int la_solve(int n, const double* K, const double* y, double* x, double* quad, double* logdet, int device)
{
    cugp_gp* g = nullptr;
    int rc = la_handle(n, K, y, device, &g);
    if (rc) return rc;
    TuneScope ts(g);
    if (!(rc = enqueue_potrf(g, false)) && !(rc = enqueue_trtri(g))) {
        launch_trmv_lower(g->dT, g->npad, g->npad, g->dy, g->dz, g->stream);
        launch_trmv_upper(g->dU, g->npad, g->npad, g->dz, g->dalpha, g->stream);
        launch_finalize(g->dz, g->npad, g->n, g->dlogdet, g->nt, nullptr, 0, scalars(g), g->dout, g->hout, g->stream);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess && x)
            e = hipMemcpyAsync(x, g->dalpha, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, g->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(g->stream);
        if (e != hipSuccess) rc = fail(CUGP_ERR_DEVICE, "la_solve", e);
        else if (barrier_expired(g->hout)) rc = fail(CUGP_ERR_DEVICE, "a stage barrier of k_trtri_block ran out of polls");
        else {
            if (quad) *quad = g->hout[4];
            if (logdet) *logdet = g->hout[5];
        }
    }
    cugp_destroy(g);
    return rc;
}

int cugp_chol_and_det(int n, const double* K, const double* y, double* quad, double* logdet, int device)
{
    if (n <= 0 || !K || !y || !quad || !logdet) return CUGP_ERR_INVALID;
    return la_solve(n, K, y, nullptr, quad, logdet, device);
}

int cugp_potrs_vec(int n, const double* K, const double* y, double* x, int device)
{
    if (n <= 0 || !K || !y || !x) return CUGP_ERR_INVALID;
    return la_solve(n, K, y, x, nullptr, nullptr, device);
}

int cugp_test_gemm_nt(int m, int n, int k, const double* A, const double* B, double* C, int device)
{
    if (m <= 0 || n <= 0 || k <= 0 || m % TILE || n % TILE || k % 16 || !A || !B || !C)
        return fail(CUGP_ERR_INVALID, "cugp_test_gemm_nt: m,n multiples of 128 and k of 16");
    HIPCHK(hipSetDevice(device));
    double *dA = nullptr, *dB = nullptr, *dC = nullptr;
    HIPCHK(hipMalloc((void**)&dA, (size_t)m * k * sizeof(double)));
    HIPCHK(hipMalloc((void**)&dB, (size_t)n * k * sizeof(double)));
    HIPCHK(hipMalloc((void**)&dC, (size_t)m * n * sizeof(double)));
    HIPCHK(hipMemcpy(dA, A, (size_t)m * k * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dB, B, (size_t)n * k * sizeof(double), hipMemcpyHostToDevice));
    launch_test_gemm_nt(dA, dB, dC, m, n, k, nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(C, dC, (size_t)m * n * sizeof(double), hipMemcpyDeviceToHost));
    (void)hipFree(dA); (void)hipFree(dB); (void)hipFree(dC);
    return CUGP_OK;
}

// stand-alone dense-LA timings on a synthetic SPD matrix built on the device (no host traffic in the timed
// region): the like-for-like counterparts of the reference's library probes cuda_src/cholesky_cu_solver.cpp
// (cusolverDnDpotrf), tmi_cu_solver.cpp (cublasDtrsm vs identity = triangular inverse) and
// cublas_matrix_multiply.cpp (cublasDgemm).  op: 0 Cholesky, 1 triangular inverse of the factor,
// 2 K^-1 = L^-T L^-1 from the triangular inverse, 3 the three together.  ms = best of `reps`.
int cugp_bench_la(int op, int n, int device, int reps, double* ms)
{
    return cugp_bench_la_check(op, n, device, reps, ms, nullptr);
}

// the same, and (ops 0 and 3) the log-determinant of the matrix from the factor it timed, so a test can tell
// that the timed launches produced the right factor
int cugp_bench_la_check(int op, int n, int device, int reps, double* ms, double* logdet)
{
    if (!ms || n <= 0 || op < 0 || op > 5 || reps <= 0) return CUGP_ERR_INVALID;
    cugp_gp* g = nullptr;
    const int d = 4;
    int rc = cugp_create(n, d, device, &g);
    if (rc) return rc;
    std::vector<double> X((size_t)n * d), y(n, 0.0);
    unsigned long long st = 88172645463325252ull;                 // xorshift: reproducible inputs
    for (double& v : X) { st ^= st << 13; st ^= st >> 7; st ^= st << 17; v = (double)(st >> 11) / 9007199254740992.0 * 6.0 - 3.0; }
    const double hp[3] = {0.0, 0.0, -1.0};
    if ((rc = cugp_set_data(g, X.data(), y.data())) || (rc = cugp_set_loghyper(g, hp)) ||
        (rc = ensure_factor_bufs(g)) || (rc = ensure_inverse_bufs(g))) { cugp_destroy(g); return rc; }
    hipEvent_t e0, e1;
    hipError_t e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    double best = 1e300;
    TuneScope ts(g);
    // op 5: the sparse model's Gram product on one chunk of SPARSE_CHUNK_DEFAULT rows against n inducing points: W is that
    // many rows of the (full) matrix K, its rows taken round and round; the partial tiles and their fixed-order sum are timed
    const SparseShape gs = sparse_shape(SPARSE_CHUNK_DEFAULT, g->npad, 0, 0);
    double *gw = nullptr, *gscr = nullptr;
    if (op == 5 && e == hipSuccess) e = hipMalloc((void**)&gw, (size_t)gs.cpad * g->npad * sizeof(double));
    if (op == 5 && e == hipSuccess) e = hipMalloc((void**)&gscr, (size_t)gs.split * g->npad * g->npad * sizeof(double));
    for (int r = 0; r < reps + 1 && e == hipSuccess && rc == CUGP_OK; r++) {
        launch_kbuild(g->dX, g->n, g->d, g->npad, CovFn{KERNEL_SE, false, scalars(g), nullptr}, g->dA, op >= 4, g->stream);
        for (int r0 = 0; op == 5 && r == 0 && r0 < gs.cpad && e == hipSuccess; r0 += g->npad)
            e = hipMemcpyAsync(gw + (size_t)r0 * g->npad, g->dA, (size_t)std::min(g->npad, gs.cpad - r0) * g->npad * sizeof(double),
                               hipMemcpyDeviceToDevice, g->stream);
        if (op == 1 || op == 2) rc = enqueue_potrf(g, false);
        if (op == 2 && !rc) rc = enqueue_trtri(g);
        if (rc) break;
        e = hipEventRecord(e0, g->stream);
        if (op == 4) launch_test_gemm_nt(g->dA, g->dA, g->dKinv, g->npad, g->npad, g->npad, g->stream);   // uniform tiles
        if (op == 5) launch_sparse_gram(gw, g->npad, gs, g->dKinv, gscr, true, g->stream);
        if (op == 0) rc = enqueue_potrf(g, false);
        if (op == 1) rc = enqueue_trtri(g);
        if (op == 2) launch_lauum(g->dU, g->dKinv, g->npad, 0, g->nt, g->stream);
        if (op == 3) rc = enqueue_potrf(g, true);                              // as an evaluation runs them
        if (e == hipSuccess) e = hipEventRecord(e1, g->stream);
        if (e == hipSuccess) e = hipEventSynchronize(e1);
        float t = 0;
        if (e == hipSuccess) e = hipEventElapsedTime(&t, e0, e1);
        if (r > 0 && t < best) best = t;                          // first round warms up
        if (e == hipSuccess && barrier_expired(g->hout)) rc = fail(CUGP_ERR_DEVICE, "a stage barrier of k_trtri_block ran out of polls");
    }
    if (logdet && rc == CUGP_OK && e == hipSuccess) {
        *logdet = NAN;
        if (op == 0 || op == 3) {                                     // 2 * sum of the diagonal blocks' shares
            std::vector<double> part(g->nt);
            e = hipMemcpy(part.data(), g->dlogdet, (size_t)g->nt * sizeof(double), hipMemcpyDeviceToHost);
            double acc = 0.0;
            for (double v : part) acc += v;
            *logdet = 2.0 * acc;
        }
    }
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    if (gw) (void)hipFree(gw);
    if (gscr) (void)hipFree(gscr);
    cugp_destroy(g);
    if (rc) return rc;
    if (e != hipSuccess) return fail(CUGP_ERR_DEVICE, "cugp_bench_la", e);
    *ms = best;
    return CUGP_OK;
}

int cugp_mfma_peak_tflops(int device, double* tflops)
{
    if (!tflops) return CUGP_ERR_INVALID;
    HIPCHK(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    const int blocks = prop.multiProcessorCount * 2;      // 8 waves per CU = 2 per SIMD
    const int iters = 20000;
    double* sink = nullptr;
    HIPCHK(hipMalloc((void**)&sink, (size_t)blocks * 256 * sizeof(double)));
    hipEvent_t a, b;
    HIPCHK(hipEventCreate(&a));
    HIPCHK(hipEventCreate(&b));
    launch_mfma_peak(sink, blocks, 2000, nullptr);
    HIPCHK(hipEventRecord(a, nullptr));
    launch_mfma_peak(sink, blocks, iters, nullptr);
    HIPCHK(hipEventRecord(b, nullptr));
    HIPCHK(hipEventSynchronize(b));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, a, b));
    const double flop = (double)blocks * 4 /*waves*/ * iters * 8.0 * 2048.0;
    *tflops = flop / (ms * 1e-3) / 1e12;
    (void)hipEventDestroy(a); (void)hipEventDestroy(b); (void)hipFree(sink);
    return CUGP_OK;
}
