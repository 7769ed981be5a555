// iter.cpp -- the matrix-free exact GP (cugp_iter_*; include/cugp.h): products with K = Kf + sn2 I
// whose entries live in registers only (kernels.hip: k_cov_apply), t conjugate-gradient recurrences on them, and the exact
// predictive mean and variance from all n rows at O(n t) memory.  The handle holds X, the labels, theta with its staging
// area, a handful of [n][tp] vector blocks that grow on first use, and one stream.
#include <algorithm>
#include <climits>
#include <cmath>
#include <new>
#include <vector>

#include "handle.h"

using namespace cugp;

struct cugp_iter {
    int n = 0, d = 0, device = 0, kernel = KERNEL_SE, nh = 3;
    bool ard = false;              // one length scale per dimension in theta
    bool route = false;            // the kernels' ARD route: ard, or rational quadratic in either form (tied weights)
    hipStream_t stream = nullptr;
    double *dX = nullptr, *dyb = nullptr;         // X [n][d]; y as column 0 of an [n][16] block
    HyperScalars *dhs = nullptr, *hhs = nullptr;  // [HyperScalars][w_1 .. w_d][alpha, h2a]: device, pinned
    double *dsc = nullptr, *hsc = nullptr;        // the recurrences' scalars (SC_ROWS + 1 rows of IT_MAXT; the last: sums)
    std::vector<double> theta;
    bool have_data = false, have_theta = false, fit_valid = false;
    int split = 0;                 // ranges of the product's j split; 0: iter_apply_plan's rule
    Scratch vb, vx, vr, vp, vq, vk, alpha, apart, dpart, xt, res;
    std::vector<double> host;      // packing: [t][n] target-major <-> [n][tp]
};

namespace {

size_t hs_bytes(const cugp_iter* h) { return sizeof(HyperScalars) + (size_t)(h->d + 2) * sizeof(double); }

CovFn cov_of(const cugp_iter* h) { return CovFn{h->kernel, h->route, *h->hhs, h->dhs, h->route && !h->ard}; }

int ready(const cugp_iter* h, const char* call)
{
    if (!h->have_data) return invalid_arg(call, "no data set (cugp_iter_set_data)");
    if (!h->have_theta) return invalid_arg(call, "no hyper-parameters set (cugp_iter_set_loghyper)");
    return CUGP_OK;
}

int solver_args(const char* call, double tol, int max_iter, int check_every)
{
    if (!(tol > 0.0) || !std::isfinite(tol)) return invalid_arg(call, "tol must be positive and finite");
    if (max_iter < 1) return invalid_arg(call, "max_iter must be positive");
    if (check_every < 1) return invalid_arg(call, "check_every must be positive");
    return CUGP_OK;
}

// columns [c0, c0 + cnt) of a target-major host array src [.][rows] -> the device block dst [rows][tp], zero beyond cnt
int pack(cugp_iter* h, const double* src, size_t rows, int c0, int cnt, int tp, Scratch& dst)
{
    int rc;
    if ((rc = dst.grow(rows * tp, h->stream))) return rc;
    h->host.assign(rows * tp, 0.0);
    for (int c = 0; c < cnt; c++)
        for (size_t i = 0; i < rows; i++) h->host[i * tp + c] = src[(size_t)(c0 + c) * rows + i];
    HIPCHK(hipMemcpyAsync(dst.p, h->host.data(), rows * tp * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return CUGP_OK;
}

// the device block src [rows][tp] -> columns [c0, c0 + cnt) of the target-major host array dst
int unpack(cugp_iter* h, const double* src, size_t rows, int c0, int cnt, int tp, double* dst)
{
    h->host.resize(rows * tp);
    HIPCHK(hipMemcpyAsync(h->host.data(), src, rows * tp * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int c = 0; c < cnt; c++)
        for (size_t i = 0; i < rows; i++) dst[(size_t)(c0 + c) * rows + i] = h->host[i * tp + c];
    return CUGP_OK;
}

// out [na][tp] = k(A, X) V (+ sn2 V: square, A == X) on the handle's stream
int product(cugp_iter* h, const CovFn& cf, const double* A, int na, const double* V, int tp, double* out, bool square)
{
    const IterPlan pl = iter_apply_plan(na, h->n, h->split);
    int rc;
    if (pl.split > 1 && (rc = h->apart.grow((size_t)pl.split * na * tp, h->stream))) return rc;
    launch_cov_apply(A, na, h->dX, h->n, h->d, cf, V, tp, out, h->apart.p, pl, square, h->stream);
    return CUGP_OK;
}

struct Counts { int active, waiting; };
int read_status(cugp_iter* h, int tp, const char* call, Counts* k)
{
    hipError_t e = hipGetLastError();
    if (e == hipSuccess)
        e = hipMemcpyAsync(h->hsc, h->dsc, (size_t)SC_ROWS * IT_MAXT * sizeof(double), hipMemcpyDeviceToHost, h->stream);
    if (const int rc = sync_or_fail(h->stream, call, e)) return rc;
    k->active = k->waiting = 0;
    for (int c = 0; c < tp; c++) {
        const double st = h->hsc[SC_STATE * IT_MAXT + c];
        k->active += st == ST_ACTIVE || st == ST_RESTART;
        k->waiting += st == ST_CANDIDATE;
    }
    return CUGP_OK;
}

// x (h->vx) = K^-1 B for the tp columns of the device block B by tp independent recurrences; the scalars stay in h->hsc
int solve_dev(cugp_iter* h, const CovFn& cf, const double* B, int tp, double tol, int max_iter, int check_every, const char* call)
{
    const int n = h->n;
    hipStream_t s = h->stream;
    int rc;
    for (Scratch* v : {&h->vx, &h->vr, &h->vp, &h->vq})
        if ((rc = v->grow((size_t)n * tp, s))) return rc;
    if ((rc = h->dpart.grow((size_t)iter_blocks(n) * IT_MAXT, s))) return rc;
    double *x = h->vx.p, *r = h->vr.p, *p = h->vp.p, *q = h->vq.p, *part = h->dpart.p, *sc = h->dsc;
    launch_iter_dot(B, B, n, tp, part, s);
    launch_iter_init(part, n, tp, tol, sc, s);
    launch_iter_start(B, x, r, p, n, tp, s);
    // the true residual of the columns that wait for it (final: of the active ones too)
    auto verify = [&](int final) {
        if (const int e = product(h, cf, h->dX, n, x, tp, q, true)) return e;
        launch_iter_resid(B, q, r, n, tp, sc, final, part, s);
        launch_iter_step_v(part, n, tp, final, sc, s);
        if (!final) launch_iter_dir(p, r, n, tp, sc, 1, s);
        return (int)CUGP_OK;
    };
    Counts k;
    int it = 0;
    for (;;) {
        if ((rc = read_status(h, tp, call, &k))) return rc;
        if (k.waiting) {
            if ((rc = verify(0))) return rc;
            continue;
        }
        if (!k.active || it >= max_iter) break;
        const int m = std::min(check_every, max_iter - it);
        for (int j = 0; j < m; j++) {
            if ((rc = product(h, cf, h->dX, n, p, tp, q, true))) return rc;
            launch_iter_dot(p, q, n, tp, part, s);
            launch_iter_step_a(part, n, tp, sc, s);
            launch_iter_update(x, r, p, q, n, tp, sc, part, s);
            launch_iter_step_b(part, n, tp, sc, s);
            launch_iter_dir(p, r, n, tp, sc, 0, s);
        }
        it += m;
    }
    if (k.active && (rc = verify(1))) return rc;
    launch_iter_poison(x, n, tp, sc, s);
    return read_status(h, tp, call, &k);
}

// rows [c0, c0 + cnt) of info from the scalars the last solve left in h->hsc
void fill_info(const cugp_iter* h, int c0, int cnt, double* info)
{
    if (!info) return;
    for (int c = 0; c < cnt; c++) {
        const double *sc = h->hsc + c, st = sc[SC_STATE * IT_MAXT], bb = sc[SC_BB * IT_MAXT];
        double* o = info + (size_t)(c0 + c) * 4;
        o[0] = sc[SC_ITERS * IT_MAXT];
        o[1] = st == ST_BROKEN ? NAN : (bb > 0.0 ? std::sqrt(sc[SC_TRUE * IT_MAXT] / bb) : 0.0);
        o[2] = st == ST_DONE ? 1.0 : 0.0;
        o[3] = st == ST_BROKEN ? 1.0 : 0.0;
    }
}

int plan_out(const char* call, int na, int nb, int t, int split, int out[4])
{
    if (!out) return invalid_arg(call, "out is NULL");
    if (na < 1 || nb < 1 || t < 1) return invalid_arg(call, "na, nb and t must be positive");
    if (na > CUGP_ITER_MAX_N || nb > CUGP_ITER_MAX_N) return invalid_arg(call, "na or nb beyond CUGP_ITER_MAX_N");
    if (split < 0 || split > CUGP_ITER_MAX_SPLIT) return invalid_arg(call, "split must lie in [0, CUGP_ITER_MAX_SPLIT]");
    const IterPlan p = iter_apply_plan(na, nb, split);
    out[0] = p.split; out[1] = p.per; out[2] = p.stages; out[3] = p.row_blocks;
    return p.split;
}

}  // namespace

int cugp_iter_apply_plan(int na, int nb, int t, int out[4]) { return plan_out("cugp_iter_apply_plan", na, nb, t, 0, out); }

int cugp_iter_apply_plan_split(int na, int nb, int t, int split, int out[4])
{
    return plan_out("cugp_iter_apply_plan_split", na, nb, t, split, out);
}

int cugp_iter_create(int n, int d, int device, int kernel, int ard, cugp_iter** out)
{
    const char* call = "cugp_iter_create";
    if (!out) return invalid_arg(call, "out is NULL");
    if (n < 1 || d < 1) return invalid_arg(call, "n and d must be positive");
    if (n > CUGP_ITER_MAX_N) return invalid_arg(call, "n beyond CUGP_ITER_MAX_N");
    if (kernel < 0 || kernel > KERNEL_RQ) return invalid_arg(call, "unknown kernel kind");
    if (ard != 0 && ard != 1) return invalid_arg(call, "ard must be 0 or 1");
    if (device < 0) return invalid_arg(call, "device must not be negative");
    int rc;
    if ((rc = need_device(call))) return rc;
    *out = nullptr;
    cugp_iter* h = new (std::nothrow) cugp_iter;
    if (!h) return fail(CUGP_ERR_NOMEM, "host allocation");
    h->n = n; h->d = d; h->device = device; h->kernel = kernel; h->ard = ard != 0;
    h->route = h->ard || kernel == KERNEL_RQ;
    h->nh = (h->ard ? d : 1) + shape_count(kernel) + 2;
    h->theta.assign(h->nh, 0.0);
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMalloc((void**)&h->dX, (size_t)n * d * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&h->dyb, (size_t)n * 16 * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&h->dhs, hs_bytes(h));
    if (e == hipSuccess) e = hipHostMalloc((void**)&h->hhs, hs_bytes(h), hipHostMallocDefault);
    if (e == hipSuccess) e = hipMalloc((void**)&h->dsc, (size_t)(SC_ROWS + 1) * IT_MAXT * sizeof(double));
    if (e == hipSuccess) e = hipHostMalloc((void**)&h->hsc, (size_t)(SC_ROWS + 1) * IT_MAXT * sizeof(double), hipHostMallocDefault);
    if (e != hipSuccess) {
        rc = fail(e == hipErrorOutOfMemory ? CUGP_ERR_NOMEM : CUGP_ERR_DEVICE, call, e);
        cugp_iter_destroy(h);
        return rc;
    }
    *out = h;
    return CUGP_OK;
}

int cugp_iter_destroy(cugp_iter* h)
{
    if (!h) return CUGP_OK;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (Scratch* v : {&h->vb, &h->vx, &h->vr, &h->vp, &h->vq, &h->vk, &h->alpha, &h->apart, &h->dpart, &h->xt, &h->res}) v->release();
    for (void* p : {(void*)h->dX, (void*)h->dyb, (void*)h->dhs, (void*)h->dsc})
        if (p) (void)hipFree(p);
    if (h->hhs) (void)hipHostFree(h->hhs);
    if (h->hsc) (void)hipHostFree(h->hsc);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return CUGP_OK;
}

int cugp_iter_num_hyper(const cugp_iter* h, int* nh)
{
    if (!h || !nh) return invalid_arg("cugp_iter_num_hyper", "null argument");
    *nh = h->nh;
    return CUGP_OK;
}

int cugp_iter_set_split(cugp_iter* h, int split)
{
    if (!h) return invalid_arg("cugp_iter_set_split", "null handle");
    if (split < 0 || split > CUGP_ITER_MAX_SPLIT) return invalid_arg("cugp_iter_set_split", "split must lie in [0, CUGP_ITER_MAX_SPLIT]");
    h->split = split;
    return CUGP_OK;
}

int cugp_iter_set_data(cugp_iter* h, const double* X, const double* y)
{
    const char* call = "cugp_iter_set_data";
    if (!h || !X || !y) return invalid_arg(call, "null argument");
    HIPCHK(hipSetDevice(h->device));
    h->fit_valid = false;
    h->have_data = false;
    HIPCHK(hipMemcpyAsync(h->dX, X, (size_t)h->n * h->d * sizeof(double), hipMemcpyHostToDevice, h->stream));
    h->host.assign((size_t)h->n * 16, 0.0);
    for (size_t i = 0; i < (size_t)h->n; i++) h->host[i * 16] = y[i];
    HIPCHK(hipMemcpyAsync(h->dyb, h->host.data(), (size_t)h->n * 16 * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->have_data = true;
    return CUGP_OK;
}

int cugp_iter_set_loghyper(cugp_iter* h, const double* theta, int nh)
{
    const char* call = "cugp_iter_set_loghyper";
    if (!h || !theta) return invalid_arg(call, "null argument");
    if (nh != h->nh) return invalid_arg(call, "nh is not the handle's (cugp_iter_num_hyper)");
    HIPCHK(hipSetDevice(h->device));
    h->fit_valid = false;
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

int cugp_iter_apply(cugp_iter* h, const double* V, int t, double* out)
{
    const char* call = "cugp_iter_apply";
    if (!h || !V || !out) return invalid_arg(call, "null argument");
    if (t < 1) return invalid_arg(call, "t must be positive");
    int rc;
    if ((rc = ready(h, call))) return rc;
    HIPCHK(hipSetDevice(h->device));
    const CovFn cf = cov_of(h);
    for (int c0 = 0; c0 < t; c0 += IT_MAXT) {
        const int cnt = std::min(IT_MAXT, t - c0), tp = iter_tp(cnt);
        if ((rc = pack(h, V, h->n, c0, cnt, tp, h->vb)) || (rc = h->vq.grow((size_t)h->n * tp, h->stream))) return rc;
        if ((rc = product(h, cf, h->dX, h->n, h->vb.p, tp, h->vq.p, true))) return rc;
        if ((rc = sync_or_fail(h->stream, call, hipGetLastError()))) return rc;
        if ((rc = unpack(h, h->vq.p, h->n, c0, cnt, tp, out))) return rc;
    }
    return CUGP_OK;
}

int cugp_iter_apply_cross(cugp_iter* h, const double* Xt, int nt, const double* V, int t, double* out)
{
    const char* call = "cugp_iter_apply_cross";
    if (!h || !Xt || !V || !out) return invalid_arg(call, "null argument");
    if (nt < 1 || t < 1) return invalid_arg(call, "nt and t must be positive");
    if (nt > CUGP_ITER_MAX_N) return invalid_arg(call, "nt beyond CUGP_ITER_MAX_N");
    int rc;
    if ((rc = ready(h, call))) return rc;
    HIPCHK(hipSetDevice(h->device));
    const CovFn cf = cov_of(h);
    if ((rc = h->xt.grow((size_t)nt * h->d, h->stream))) return rc;
    HIPCHK(hipMemcpyAsync(h->xt.p, Xt, (size_t)nt * h->d * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int c0 = 0; c0 < t; c0 += IT_MAXT) {
        const int cnt = std::min(IT_MAXT, t - c0), tp = iter_tp(cnt);
        if ((rc = pack(h, V, h->n, c0, cnt, tp, h->vb)) || (rc = h->res.grow((size_t)nt * tp, h->stream))) return rc;
        if ((rc = product(h, cf, h->xt.p, nt, h->vb.p, tp, h->res.p, false))) return rc;
        if ((rc = sync_or_fail(h->stream, call, hipGetLastError()))) return rc;
        if ((rc = unpack(h, h->res.p, nt, c0, cnt, tp, out))) return rc;
    }
    return CUGP_OK;
}

int cugp_iter_solve(cugp_iter* h, const double* B, int t, double tol, int max_iter, int check_every, double* Xout, double* info)
{
    const char* call = "cugp_iter_solve";
    if (!h || !B || !Xout) return invalid_arg(call, "null argument");
    if (t < 1) return invalid_arg(call, "t must be positive");
    int rc;
    if ((rc = solver_args(call, tol, max_iter, check_every)) || (rc = ready(h, call))) return rc;
    HIPCHK(hipSetDevice(h->device));
    const CovFn cf = cov_of(h);
    for (int c0 = 0; c0 < t; c0 += IT_MAXT) {
        const int cnt = std::min(IT_MAXT, t - c0), tp = iter_tp(cnt);
        if ((rc = pack(h, B, h->n, c0, cnt, tp, h->vb))) return rc;
        if ((rc = solve_dev(h, cf, h->vb.p, tp, tol, max_iter, check_every, call))) return rc;
        fill_info(h, c0, cnt, info);
        if ((rc = unpack(h, h->vx.p, h->n, c0, cnt, tp, Xout))) return rc;
    }
    return CUGP_OK;
}

int cugp_iter_fit(cugp_iter* h, double tol, int max_iter, int check_every, double* info)
{
    const char* call = "cugp_iter_fit";
    if (!h) return invalid_arg(call, "null handle");
    int rc;
    if ((rc = solver_args(call, tol, max_iter, check_every)) || (rc = ready(h, call))) return rc;
    HIPCHK(hipSetDevice(h->device));
    h->fit_valid = false;
    if ((rc = h->alpha.grow((size_t)h->n * 16, h->stream))) return rc;
    if ((rc = solve_dev(h, cov_of(h), h->dyb, 16, tol, max_iter, check_every, call))) return rc;
    fill_info(h, 0, 1, info);
    HIPCHK(hipMemcpyAsync(h->alpha.p, h->vx.p, (size_t)h->n * 16 * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->fit_valid = true;
    return CUGP_OK;
}

int cugp_iter_get_alpha(cugp_iter* h, double* alpha)
{
    const char* call = "cugp_iter_get_alpha";
    if (!h || !alpha) return invalid_arg(call, "null argument");
    if (!h->fit_valid) return invalid_arg(call, "no fit for the data and hyper-parameters as they stand (cugp_iter_fit)");
    HIPCHK(hipSetDevice(h->device));
    return unpack(h, h->alpha.p, h->n, 0, 1, 16, alpha);
}

int cugp_iter_predict(cugp_iter* h, const double* Xt, int nt, double* mean, double* var, double tol, int max_iter,
                      int check_every, double* info)
{
    const char* call = "cugp_iter_predict";
    if (!h || !Xt || !mean) return invalid_arg(call, "null argument");
    if (nt < 1) return invalid_arg(call, "nt must be positive");
    if (nt > CUGP_ITER_MAX_N) return invalid_arg(call, "nt beyond CUGP_ITER_MAX_N");
    int rc;
    if (var && (rc = solver_args(call, tol, max_iter, check_every))) return rc;
    if ((rc = ready(h, call))) return rc;
    if (!h->fit_valid) return invalid_arg(call, "no fit for the data and hyper-parameters as they stand (cugp_iter_fit)");
    HIPCHK(hipSetDevice(h->device));
    const CovFn cf = cov_of(h);
    hipStream_t s = h->stream;
    if ((rc = h->xt.grow((size_t)nt * h->d, s)) || (rc = h->res.grow((size_t)nt * 16, s))) return rc;
    HIPCHK(hipMemcpyAsync(h->xt.p, Xt, (size_t)nt * h->d * sizeof(double), hipMemcpyHostToDevice, s));
    if ((rc = product(h, cf, h->xt.p, nt, h->alpha.p, 16, h->res.p, false))) return rc;
    if ((rc = sync_or_fail(s, call, hipGetLastError()))) return rc;
    if ((rc = unpack(h, h->res.p, nt, 0, 1, 16, mean))) return rc;
    if (!var) return CUGP_OK;
    // var_c = sf2 + sn2 - ks_c' K^-1 ks_c, IT_MAXT test points a solve
    const double prior = h->hhs->signal_var + h->hhs->noise_var;
    double *dsum = h->dsc + (size_t)SC_ROWS * IT_MAXT, *hsum = h->hsc + (size_t)SC_ROWS * IT_MAXT;
    for (int c0 = 0; c0 < nt; c0 += IT_MAXT) {
        const int cnt = std::min(IT_MAXT, nt - c0), tp = iter_tp(cnt);
        if ((rc = h->vk.grow((size_t)h->n * tp, s))) return rc;
        launch_iter_cross_rhs(h->dX, h->n, h->d, h->xt.p + (size_t)c0 * h->d, cnt, tp, cf, h->vk.p, s);
        if ((rc = solve_dev(h, cf, h->vk.p, tp, tol, max_iter, check_every, call))) return rc;
        fill_info(h, c0, cnt, info);
        launch_iter_dot(h->vk.p, h->vx.p, h->n, tp, h->dpart.p, s);
        launch_iter_sum(h->dpart.p, h->n, tp, dsum, s);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(hsum, dsum, (size_t)IT_MAXT * sizeof(double), hipMemcpyDeviceToHost, s);
        if ((rc = sync_or_fail(s, call, e))) return rc;
        for (int c = 0; c < cnt; c++) var[c0 + c] = prior - hsum[c];
    }
    return CUGP_OK;
}
