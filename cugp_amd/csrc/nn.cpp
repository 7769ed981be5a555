// nn.cpp -- the nearest-neighbour (Vecchia) GP (cugp_nn_*; include/cugp.h): the log-likelihood as a
// sum of n small conditionals, each factored by one wavefront (kernels.hip: k_nn_block), its gradient, the local
// prediction and conjugate gradients on it.  The handle holds X, y, the index rows, theta with its staging area and one
// stream; every index a kernel reads was checked here, on the host, when it was set.
#include <algorithm>
#include <cmath>
#include <new>
#include <vector>

#include "handle.h"

using namespace cugp;

namespace {

static_assert(NN_MAX_M == CUGP_NN_MAX_M, "the kernels' largest m is the header's");

size_t hs_bytes(const cugp_nn* h) { return sizeof(HyperScalars) + (size_t)(h->d + 2) * sizeof(double); }

CovFn cov_of(const cugp_nn* h) { return CovFn{h->kernel, h->route, *h->hhs, h->dhs, h->route && !h->ard}; }

// rows [rows][m]: every entry -1 or a row below `n` (training: below its own row), none twice in a row
int check_rows(const char* call, const int* idx, long long rows, int m, int n, bool training)
{
    int sorted[NN_MAX_M];
    for (long long i = 0; i < rows; i++) {
        const int* row = idx + (size_t)i * m;
        const long long lim = training ? std::min<long long>(i, n) : n;
        int cnt = 0;
        for (int s = 0; s < m; s++) {
            if (row[s] == -1) continue;
            if (row[s] < 0 || row[s] >= lim)
                return invalid_arg(call, training ? "an index is not an earlier row (or -1)" : "an index is not a training row (or -1)");
            sorted[cnt++] = row[s];
        }
        std::sort(sorted, sorted + cnt);
        if (std::adjacent_find(sorted, sorted + cnt) != sorted + cnt) return invalid_arg(call, "an index stands twice in a row");
    }
    return CUGP_OK;
}

int ready(const cugp_nn* h, const char* call, bool need_idx)
{
    if (!h->have_data) return invalid_arg(call, "no data set (cugp_nn_set_data)");
    if (need_idx && !h->have_idx) return invalid_arg(call, "no neighbours set (cugp_nn_set_neighbors)");
    if (!h->have_theta) return invalid_arg(call, "no hyper-parameters set (cugp_nn_set_loghyper)");
    return CUGP_OK;
}

// theta into the handle and its staging area, as cugp_iter_set_loghyper lays it out
int set_theta(cugp_nn* h, const double* theta)
{
    const int nh = h->nh;
    HIPCHK(hipSetDevice(h->device));
    h->have_theta = false;
    h->theta.assign(theta, theta + nh);
    const double* sf = theta + nh - 2;
    *h->hhs = HyperScalars{h->route ? 1.0 : std::exp(theta[0] * 2), std::exp(sf[0] * 2), std::exp(sf[1] * 2)};
    double* w = (double*)(h->hhs + 1);
    for (int c = 0; c < h->d; c++) w[c] = std::exp(-theta[h->ard ? c : 0]);
    const double alpha = h->kernel == KERNEL_RQ ? std::exp(theta[nh - 3]) : 0.0;
    w[h->d] = alpha;
    w[h->d + 1] = h->kernel == KERNEL_RQ ? 0.5 / alpha : 0.0;
    HIPCHK(hipMemcpyAsync(h->dhs, h->hhs, hs_bytes(h), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->have_theta = true;
    return CUGP_OK;
}

// one evaluation: the blocks' launch, the sums, the row [l, g (nh)] into h->hout; one wait
int eval(cugp_nn* h, bool grad, const char* call)
{
    HIPCHK(hipSetDevice(h->device));
    const CovFn cf = cov_of(h);
    hipStream_t s = h->stream;
    const int nwg = nn_workgroups(h->n, h->m), nc = grad ? 1 + nn_part_columns(cf, h->d) : 1;
    int rc;
    if ((rc = h->part.grow((size_t)nwg * nc, s)) || (rc = h->out.grow((size_t)1 + h->nh + nc, s)) ||
        (rc = h->hout.grow((size_t)1 + h->nh, s)))
        return rc;
    launch_nn_block(grad ? NN_GRAD : NN_VALUE, h->dX, h->dy, h->didx, nullptr, h->n, h->m, h->d, cf, h->part.p, nullptr, nullptr,
                    1, s);
    launch_nn_finish(h->part.p, nwg, nc, grad && cf.tied ? h->d : 0, h->out.p, h->out.p + 1 + h->nh, s);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess)
        e = hipMemcpyAsync(h->hout.p, h->out.p, (size_t)(grad ? 1 + h->nh : 1) * sizeof(double), hipMemcpyDeviceToHost, s);
    return sync_or_fail(s, call, e);
}

// f = -L and its gradient at th (NaN where the evaluation fails)
void nn_objective(void* ctx, const double* th, int nh, double* f, double* gr)
{
    cugp_nn* h = (cugp_nn*)ctx;
    const bool ok = set_theta(h, th) == CUGP_OK && eval(h, true, "cugp_nn_cg_solve") == CUGP_OK;
    objective_result(ok, ok ? h->hout.p[0] : NAN, h->hout.p + 1, nh, f, gr);
}

}  // namespace

int cugp_nn_check_neighbors(const int* idx, int rows, int m, int n, int training)
{
    const char* call = "cugp_nn_check_neighbors";
    if (!idx) return invalid_arg(call, "idx is NULL");
    if (rows < 1 || n < 1) return invalid_arg(call, "rows and n must be positive");
    if (m < 1 || m > CUGP_NN_MAX_M) return invalid_arg(call, "m must lie in [1, CUGP_NN_MAX_M]");
    if (training != 0 && training != 1) return invalid_arg(call, "training must be 0 or 1");
    return check_rows(call, idx, rows, m, n, training != 0);
}

int cugp_nn_create(int n, int m, int d, int device, int kernel, int ard, cugp_nn** out)
{
    const char* call = "cugp_nn_create";
    if (!out) return invalid_arg(call, "out is NULL");
    if (n < 1 || d < 1) return invalid_arg(call, "n and d must be positive");
    if (n > CUGP_ITER_MAX_N) return invalid_arg(call, "n beyond CUGP_ITER_MAX_N");
    if (m < 1 || m > CUGP_NN_MAX_M) return invalid_arg(call, "m must lie in [1, CUGP_NN_MAX_M]");
    if (kernel < 0 || kernel > KERNEL_RQ) return invalid_arg(call, "unknown kernel kind");
    if (ard != 0 && ard != 1) return invalid_arg(call, "ard must be 0 or 1");
    if (device < 0) return invalid_arg(call, "device must not be negative");
    int rc;
    if ((rc = need_device(call))) return rc;
    *out = nullptr;
    cugp_nn* h = new (std::nothrow) cugp_nn;
    if (!h) return fail(CUGP_ERR_NOMEM, "host allocation");
    h->n = n; h->m = m; h->d = d; h->device = device; h->kernel = kernel; h->ard = ard != 0;
    h->route = h->ard || kernel == KERNEL_RQ;
    h->nh = (h->ard ? d : 1) + shape_count(kernel) + 2;
    h->theta.assign(h->nh, 0.0);
    h->hout.pinned = true;
    h->hpred.pinned = true;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMalloc((void**)&h->dX, (size_t)n * d * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&h->dy, (size_t)n * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&h->didx, (size_t)n * m * sizeof(int));
    if (e == hipSuccess) e = hipMalloc((void**)&h->dhs, hs_bytes(h));
    if (e == hipSuccess) e = hipHostMalloc((void**)&h->hhs, hs_bytes(h), hipHostMallocDefault);
    if (e != hipSuccess) {
        rc = fail(e == hipErrorOutOfMemory ? CUGP_ERR_NOMEM : CUGP_ERR_DEVICE, call, e);
        cugp_nn_destroy(h);
        return rc;
    }
    *out = h;
    return CUGP_OK;
}

int cugp_nn_destroy(cugp_nn* h)
{
    if (!h) return CUGP_OK;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (Scratch* v : {&h->part, &h->out, &h->hout, &h->xt, &h->tidx, &h->pred, &h->hpred}) v->release();
    for (void* p : {(void*)h->dX, (void*)h->dy, (void*)h->didx, (void*)h->dhs})
        if (p) (void)hipFree(p);
    if (h->hhs) (void)hipHostFree(h->hhs);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return CUGP_OK;
}

int cugp_nn_num_hyper(const cugp_nn* h, int* nh)
{
    if (!h || !nh) return invalid_arg("cugp_nn_num_hyper", "null argument");
    *nh = h->nh;
    return CUGP_OK;
}

int cugp_nn_set_data(cugp_nn* h, const double* X, const double* y)
{
    const char* call = "cugp_nn_set_data";
    if (!h || !X || !y) return invalid_arg(call, "null argument");
    if (h->n < 1) return invalid_arg(call, "not a handle of cugp_nn_create");
    HIPCHK(hipSetDevice(h->device));
    h->have_data = false;
    HIPCHK(hipMemcpyAsync(h->dX, X, (size_t)h->n * h->d * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->dy, y, (size_t)h->n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->have_data = true;
    return CUGP_OK;
}

int cugp_nn_set_neighbors(cugp_nn* h, const int* idx)
{
    const char* call = "cugp_nn_set_neighbors";
    if (!h || !idx) return invalid_arg(call, "null argument");
    if (h->n < 1) return invalid_arg(call, "not a handle of cugp_nn_create");
    if (const int rc = check_rows(call, idx, h->n, h->m, h->n, true)) return rc;      // (the rows held so far stay)
    HIPCHK(hipSetDevice(h->device));
    h->have_idx = false;
    HIPCHK(hipMemcpyAsync(h->didx, idx, (size_t)h->n * h->m * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->have_idx = true;
    return CUGP_OK;
}

int cugp_nn_set_loghyper(cugp_nn* h, const double* theta, int nh)
{
    const char* call = "cugp_nn_set_loghyper";
    if (!h || !theta) return invalid_arg(call, "null argument");
    if (h->n < 1 || nh != h->nh) return invalid_arg(call, "nh is not the handle's (cugp_nn_num_hyper)");
    return set_theta(h, theta);
}

int cugp_nn_loglik(cugp_nn* h, double* ll)
{
    const char* call = "cugp_nn_loglik";
    if (!h || !ll) return invalid_arg(call, "null argument");
    int rc;
    if ((rc = ready(h, call, true)) || (rc = eval(h, false, call))) return rc;
    *ll = h->hout.p[0];
    return CUGP_OK;
}

int cugp_nn_loglik_grad(cugp_nn* h, double* ll, double* g, int nh)
{
    const char* call = "cugp_nn_loglik_grad";
    if (!h || !ll || !g) return invalid_arg(call, "null argument");
    int rc;
    if ((rc = ready(h, call, true))) return rc;
    if (nh != h->nh) return invalid_arg(call, "nh is not the handle's (cugp_nn_num_hyper)");
    if ((rc = eval(h, true, call))) return rc;
    *ll = h->hout.p[0];
    std::copy(h->hout.p + 1, h->hout.p + 1 + nh, g);
    return CUGP_OK;
}

int cugp_nn_predict(cugp_nn* h, const double* Xt, int nt, const int* idx_t, int with_noise, double* mean, double* var)
{
    const char* call = "cugp_nn_predict";
    if (!h || !Xt || !idx_t || !mean || !var) return invalid_arg(call, "null argument");
    if (nt < 1 || nt > CUGP_ITER_MAX_N) return invalid_arg(call, "nt must lie in [1, CUGP_ITER_MAX_N]");
    if (with_noise != 0 && with_noise != 1) return invalid_arg(call, "with_noise must be 0 or 1");
    int rc;
    if ((rc = ready(h, call, false)) || (rc = check_rows(call, idx_t, nt, h->m, h->n, false))) return rc;
    HIPCHK(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const size_t nti = ((size_t)nt * h->m + 1) / 2;                 // the index rows, counted in doubles
    if ((rc = h->xt.grow((size_t)nt * h->d, s)) || (rc = h->tidx.grow(nti, s)) || (rc = h->pred.grow((size_t)2 * nt, s)) ||
        (rc = h->hpred.grow((size_t)2 * nt, s)))
        return rc;
    HIPCHK(hipMemcpyAsync(h->xt.p, Xt, (size_t)nt * h->d * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(h->tidx.p, idx_t, (size_t)nt * h->m * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));                                // (the caller's arrays are pageable: read before returning)
    launch_nn_block(NN_PREDICT, h->dX, h->dy, (const int*)h->tidx.p, h->xt.p, nt, h->m, h->d, cov_of(h), nullptr, h->pred.p,
                    h->pred.p + nt, with_noise, s);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(h->hpred.p, h->pred.p, (size_t)2 * nt * sizeof(double), hipMemcpyDeviceToHost, s);
    if ((rc = sync_or_fail(s, call, e))) return rc;
    std::copy(h->hpred.p, h->hpred.p + nt, mean);
    std::copy(h->hpred.p + nt, h->hpred.p + 2 * (size_t)nt, var);
    return CUGP_OK;
}

int cugp_nn_cg_solve(cugp_nn* h, int budget, double* trace, int trace_cap, int* nevals)
{
    const char* call = "cugp_nn_cg_solve";
    if (!h) return invalid_arg(call, "null handle");
    if (budget <= 0) return invalid_arg(call, "budget must be positive");
    int rc;
    if ((rc = ready(h, call, true))) return rc;
    std::vector<double> th(h->theta);
    if ((rc = cg_iterates(nn_objective, h, th.data(), h->nh, budget, trace, trace_cap, nevals))) return rc;
    return set_theta(h, th.data());
}
