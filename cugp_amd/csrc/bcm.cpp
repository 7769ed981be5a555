// bcm.cpp -- product-of-experts ("BCM") over the experts resident on the GPUs of one process.
//
// Mirrors class BCM (distributed_gp/BCM.h:2-27, BCM.cpp): K experts, each a full GP on its own rows,
// the objective is the plain sum of the experts' log-likelihoods / gradients (BCM.cpp:153-198) and
// the prediction is a product of experts with no prior-precision correction (BCM.cpp:45-62).
// The experts are padded to a common size and evaluated as a GROUP: one sequence of launches in which
// blockIdx.y selects the expert (group.h) -- 16 experts driven from 16 streams were bounded by the
// command processor's dispatch rate, not by the CUs.  When a group evaluation is not possible (experts
// with different hyper-parameters, profiling on) every expert is enqueued on its own stream before the
// first result is fetched.  Sums are taken in expert order on the host either way, so the result does
// not depend on completion order.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/cugp.h"
#include <hip/hip_runtime.h>

#include "group.h"

// the experts of one device: evaluated as one group of shared launches when their shapes allow it
struct DeviceSet {
    int device = 0;
    std::vector<int> idx;            // global expert indices, ascending
    cugp_group* group = nullptr;     // null: a single expert, or shapes differ
    bool grouped_now = false;        // the evaluation in flight was enqueued as a group
    // cugp_bcm_predict_grad: the set's gradient rows on its device ([local expert][(2 + 2 d) nt]) and, for the experts that
    // cannot share launches, the stream ordered behind all of theirs (created on first use)
    Scratch grad_rows;
    hipStream_t grad_stream = nullptr;
    // "rows written" per LOCAL expert whose stream wrote some (set_order_after): created on this set's device, so an
    // event only ever meets streams of the device it was created on
    std::vector<hipEvent_t> ev;
};

struct cugp_bcm {
    std::vector<DeviceSet> sets;     // one per entry of the device list (the same device may be listed twice)
    std::vector<cugp_gp*> experts;   // global order k = 0..K-1
    std::vector<int> rows;
    int d = 0;
    // ARD (cugp_bcm_create_ard; for life): every expert is an ARD handle, nh = d + 2, and the rows of an evaluation are
    // {LL, g[nh]}.  Rational quadratic (cugp_bcm_create_rq): nh-wide too, nh = d + 3, or 4 with one tied length scale.  Every body below runs at the row width 1 + nh -- 4 for the isotropic calls, whose bits it keeps.
    bool ard = false;
    int nh = 3;
    std::vector<double> hp = {0, 0, 0};
    int kernel = 0;                  // CUGP_KERNEL_* of every expert, for life
    Scratch pred_host{nullptr, 0, true};   // pinned: [expert][mean nt | variance nt] of the prediction in flight
    // cugp_bcm_predict_mode on one device set: {status, count, [K][2][nt] latent rows} (k_poe_reduce_mode's block of a
    // world of one), its output [mean nt | var nt | status, count] on the device and pinned, the stream they run on
    Scratch mode_rows, mode_out, mode_hout{nullptr, 0, true};
    hipStream_t mode_stream = nullptr;
    Scratch grad_host{nullptr, 0, true};   // pinned: cugp_bcm_predict_grad's rows, set after set
    int grad_form = 0;               // cugp_bcm_predict_grad_form: 0 no call yet, 1 expert by expert, 2 every set as a group
};

namespace {

// the argument checks of the 3-entry calls and their _ard twins, before any device call (cugp_capi.cpp: refuse_ard /
// want_ard are the handles' counterparts)
int refuse_ard_bcm(const cugp_bcm* b, const char* call, const char* use)
{
    if (!b->ard) return CUGP_OK;
    char buf[256];
    if (b->kernel == CUGP_KERNEL_RQ) snprintf(buf, sizeof buf, "%s: the BCM is rational quadratic (%d hyper-parameters); use %s", call, b->nh, use);
    else snprintf(buf, sizeof buf, "%s: the BCM is ARD (d + 2 hyper-parameters); use %s", call, use);
    return cugp_internal_fail(CUGP_ERR_INVALID, buf);
}

int want_ard_bcm(const cugp_bcm* b, int nh, const char* call, bool pointers_ok = true)
{
    char buf[256];
    if (!b || !pointers_ok || nh < 3) {
        snprintf(buf, sizeof buf, "%s: null argument or nh < 3", call);
        return cugp_internal_fail(CUGP_ERR_INVALID, buf);
    }
    if (!b->ard) {
        snprintf(buf, sizeof buf, "%s: the BCM is isotropic (3 hyper-parameters); create it with cugp_bcm_create_ard, or use %.*s",
                 call, (int)strlen(call) - 4, call);
        return cugp_internal_fail(CUGP_ERR_INVALID, buf);
    }
    if (nh != b->nh) {
        if (b->kernel == CUGP_KERNEL_RQ) snprintf(buf, sizeof buf, "%s: nh = %d, the rational quadratic BCM has %d hyper-parameters", call, nh, b->nh);
        else snprintf(buf, sizeof buf, "%s: nh = %d, the BCM has d + 2 = %d hyper-parameters", call, nh, b->nh);
        return cugp_internal_fail(CUGP_ERR_INVALID, buf);
    }
    return CUGP_OK;
}

int expert_fetch(cugp_bcm* b, cugp_gp* e, double* ll, double* g)
{
    return b->ard ? cugp_loglik_grad_fetch_ard(e, ll, g, b->nh) : cugp_loglik_grad_fetch(e, ll, g);
}

int bcm_create(int ndev, const int* devices, int nexperts, const int* rows, int d, int kernel, bool ard, cugp_bcm** out,
               bool tied = false);
int bcm_create_split(const double* X, const double* y, int N, int D, int K, int ndev, const int* devices, int kernel,
                     bool ard, cugp_bcm** out, bool tied = false);

}  // namespace

extern "C" {

// Experts k = 0..K-1 over the devices of one process: expert k lives on devices[k mod ndev] -- the reference's
// placement of chunk i on worker i mod W (cuda_scalingdist/cg_solver.cpp:93) -- and one host thread drives all
// of them: every device's experts are enqueued (one group of shared launches per device) before the first
// result is read, sums are taken in expert order on the host, so the numbers are those of the single-device
// BCM bit for bit whatever the device list (distributed_gp/BCM.cpp:153-198).
int cugp_bcm_create_multi(int ndev, const int* devices, int nexperts, const int* rows, int d, cugp_bcm** out)
{
    return cugp_bcm_create_kernel(ndev, devices, nexperts, rows, d, CUGP_KERNEL_SE, out);
}

// the same with every expert of one covariance family (cugp_create_kernel); kind 0 is the call above
int cugp_bcm_create_kernel(int ndev, const int* devices, int nexperts, const int* rows, int d, int kernel,
                           cugp_bcm** out)
{
    return bcm_create(ndev, devices, nexperts, rows, d, kernel, false, out);
}

// every expert an SE-ARD handle (cugp_create_ard): nh = d + 2 hyper-parameters, the _ard calls below
int cugp_bcm_create_ard(int ndev, const int* devices, int nexperts, const int* rows, int d, cugp_bcm** out)
{
    return bcm_create(ndev, devices, nexperts, rows, d, CUGP_KERNEL_SE, true, out);
}

// ARD experts of any covariance family (cugp_create_ard_kernel); kind 0 is the call above
int cugp_bcm_create_ard_kernel(int ndev, const int* devices, int nexperts, const int* rows, int d, int kernel,
                               cugp_bcm** out)
{
    if (kernel < CUGP_KERNEL_SE || kernel > CUGP_KERNEL_MATERN52)
        return cugp_internal_fail(CUGP_ERR_INVALID,
                                  "cugp_bcm_create_ard_kernel: unknown kernel kind (0 SE, 1 Matern 3/2, 2 Matern 5/2)");
    return bcm_create(ndev, devices, nexperts, rows, d, kernel, true, out);
}

// every expert a rational quadratic handle (cugp_create_rq): ard = 1 nh = d + 3, ard = 0 (one length scale) nh = 4; the
// _ard calls below with the BCM's nh.  The arguments are checked here, before any device call.
int cugp_bcm_create_rq(int ndev, const int* devices, int nexperts, const int* rows, int d, int ard, cugp_bcm** out)
{
    if (!out || ndev <= 0 || !devices || nexperts <= 0 || !rows || d <= 0)
        return cugp_internal_fail(CUGP_ERR_INVALID, "cugp_bcm_create_rq: null argument, or ndev, nexperts, d not positive");
    for (int k = 0; k < nexperts; k++)
        if (rows[k] <= 0) return cugp_internal_fail(CUGP_ERR_INVALID, "cugp_bcm_create_rq: an expert without rows");
    if (ard != 0 && ard != 1)
        return cugp_internal_fail(CUGP_ERR_INVALID, "cugp_bcm_create_rq: ard must be 0 (one length scale) or 1 (one per dimension)");
    return bcm_create(ndev, devices, nexperts, rows, d, CUGP_KERNEL_RQ, true, out, ard == 0);
}

int cugp_bcm_create_split_rq(const double* X, const double* y, int N, int D, int K, int ndev, const int* devices, int ard,
                             cugp_bcm** out)
{
    if (!X || !y || !out || !devices || N <= 0 || D <= 0 || K <= 0 || K > N || ndev <= 0)
        return cugp_internal_fail(CUGP_ERR_INVALID, "cugp_bcm_create_split_rq: null argument, or N, D, K, ndev not positive, or K > N");
    if (ard != 0 && ard != 1)
        return cugp_internal_fail(CUGP_ERR_INVALID, "cugp_bcm_create_split_rq: ard must be 0 (one length scale) or 1 (one per dimension)");
    return bcm_create_split(X, y, N, D, K, ndev, devices, CUGP_KERNEL_RQ, true, out, ard == 0);
}

}  // extern "C"

namespace {
// kernel == CUGP_KERNEL_RQ comes from the two calls above alone (ard set; tied: one length scale)
int bcm_create(int ndev, const int* devices, int nexperts, const int* rows, int d, int kernel, bool ard, cugp_bcm** out,
               bool tied)
{
    if (!out || ndev <= 0 || !devices || nexperts <= 0 || !rows || d <= 0) return CUGP_ERR_INVALID;
    const bool rq = kernel == CUGP_KERNEL_RQ && ard;
    if (!rq && (kernel < CUGP_KERNEL_SE || kernel > CUGP_KERNEL_MATERN52)) return CUGP_ERR_INVALID;
    cugp_bcm* b = new (std::nothrow) cugp_bcm;
    if (!b) return CUGP_ERR_NOMEM;
    b->d = d;
    b->kernel = kernel;
    b->ard = ard;
    if (ard) { b->nh = (rq && tied ? 1 : d) + (rq ? 1 : 0) + 2; b->hp.assign(b->nh, 0.0); }
    // Common padded size (identity padding) so that the experts can share launches -- unless their row counts
    // differ by more than a tile or ~6 %: then padding the small ones would cost more than it gains.
    int nmax = 0, nmin = rows[0];
    for (int k = 0; k < nexperts; k++) {
        if (rows[k] <= 0) { delete b; return CUGP_ERR_INVALID; }
        nmax = rows[k] > nmax ? rows[k] : nmax;
        nmin = rows[k] < nmin ? rows[k] : nmin;
    }
    const int tmax = (nmax + 127) / 128, tmin = (nmin + 127) / 128;
    const int pad_to = (tmax - tmin <= (tmin / 16 > 1 ? tmin / 16 : 1)) ? nmax : 0;
    const int nsets = ndev < nexperts ? ndev : nexperts;
    b->sets.resize(nsets);
    for (int s = 0; s < nsets; s++) b->sets[s].device = devices[s];
    for (int k = 0; k < nexperts; k++) {
        DeviceSet& ds = b->sets[k % nsets];
        cugp_gp* g = nullptr;
        int rc = rq    ? cugp_create_rq(rows[k], d, ds.device, pad_to, tied ? 0 : 1, &g)
                 : ard ? cugp_create_ard_kernel(rows[k], d, ds.device, pad_to, kernel, &g)
                       : cugp_create_kernel(rows[k], d, ds.device, pad_to, kernel, &g);
        if (rc) { cugp_bcm_destroy(b); return rc; }
        b->experts.push_back(g);                        // (owned by b from here on: cugp_bcm_destroy)
        rc = cugp_mark_bcm_expert(g);                   // (cugp_append refuses the experts of a BCM; no stream priorities)
        // several experts on one device already fill each other's idle time; the extra streams only cost launches
        if (!rc && nexperts > nsets) rc = cugp_set_overlap(g, 0);
        if (rc) { cugp_bcm_destroy(b); return rc; }
        b->rows.push_back(rows[k]);
        ds.idx.push_back(k);
    }
    for (DeviceSet& ds : b->sets) {
        // A set of ONE expert beside larger sets (5 experts over 3 devices: 2 + 2 + 1) is a group of one: it then takes
        // its inverse in the same hand-over blocks as the other sets' groups.  Since round 5 an accumulate-form tile
        // product adds its C tile in the epilogue, so the bits of K^-1 depend on where the block boundaries are; with
        // its overlap off (below: nexperts > nsets) the lone expert would take the whole-matrix form instead.
        if (ds.idx.size() < 2 && !(nexperts > nsets)) continue;
        std::vector<cugp_gp*> mine;
        for (int k : ds.idx) mine.push_back(b->experts[k]);
        if (cugp_group_create(mine.data(), (int)mine.size(), &ds.group) != CUGP_OK) ds.group = nullptr;
    }
    *out = b;
    return CUGP_OK;
}

// BCM.cpp:85-110 -- expert k gets rows [k*floor(N/K), ...), the last one also the remainder
int bcm_create_split(const double* X, const double* y, int N, int D, int K, int ndev, const int* devices, int kernel,
                     bool ard, cugp_bcm** out, bool tied)
{
    if (!X || !y || N <= 0 || D <= 0 || K <= 0 || K > N) return CUGP_ERR_INVALID;
    if (!(kernel == CUGP_KERNEL_RQ && ard) && (kernel < CUGP_KERNEL_SE || kernel > CUGP_KERNEL_MATERN52)) return CUGP_ERR_INVALID;
    std::vector<int> rows(K), off(K);
    const int part = N / K;
    int start = 0;
    for (int k = 0; k < K; k++) {
        off[k] = start;
        rows[k] = (k == K - 1) ? (N - start) : part;
        start += part;
    }
    int rc = bcm_create(ndev, devices, K, rows.data(), D, kernel, ard, out, tied);
    if (rc) return rc;
    for (int k = 0; k < K; k++) {
        rc = cugp_bcm_set_expert_data(*out, k, X + (size_t)off[k] * D, y + off[k]);
        if (rc) { cugp_bcm_destroy(*out); *out = nullptr; return rc; }
    }
    return CUGP_OK;
}
}  // namespace

extern "C" {

int cugp_bcm_create(int nexperts, const int* rows, int d, int device, cugp_bcm** out)
{
    return cugp_bcm_create_multi(1, &device, nexperts, rows, d, out);
}

int cugp_bcm_create_split_multi(const double* X, const double* y, int N, int D, int K, int ndev, const int* devices,
                                cugp_bcm** out)
{
    return cugp_bcm_create_split_kernel(X, y, N, D, K, ndev, devices, CUGP_KERNEL_SE, out);
}

int cugp_bcm_create_split_kernel(const double* X, const double* y, int N, int D, int K, int ndev, const int* devices,
                                 int kernel, cugp_bcm** out)
{
    return bcm_create_split(X, y, N, D, K, ndev, devices, kernel, false, out);
}

int cugp_bcm_create_split_ard(const double* X, const double* y, int N, int D, int K, int ndev, const int* devices,
                              cugp_bcm** out)
{
    return bcm_create_split(X, y, N, D, K, ndev, devices, CUGP_KERNEL_SE, true, out);
}

int cugp_bcm_create_split_ard_kernel(const double* X, const double* y, int N, int D, int K, int ndev,
                                     const int* devices, int kernel, cugp_bcm** out)
{
    if (kernel < CUGP_KERNEL_SE || kernel > CUGP_KERNEL_MATERN52)
        return cugp_internal_fail(CUGP_ERR_INVALID,
                                  "cugp_bcm_create_split_ard_kernel: unknown kernel kind (0 SE, 1 Matern 3/2, 2 Matern 5/2)");
    return bcm_create_split(X, y, N, D, K, ndev, devices, kernel, true, out);
}

int cugp_bcm_create_split(const double* X, const double* y, int N, int D, int K, int device, cugp_bcm** out)
{
    return cugp_bcm_create_split_multi(X, y, N, D, K, 1, &device, out);
}

int cugp_bcm_destroy(cugp_bcm* b)
{
    if (!b) return CUGP_OK;
    for (DeviceSet& ds : b->sets) {
        if (ds.grad_rows.p || ds.grad_stream || !ds.ev.empty()) (void)hipSetDevice(ds.device);
        for (hipEvent_t e : ds.ev) (void)hipEventDestroy(e);
        if (ds.grad_stream) { (void)hipStreamSynchronize(ds.grad_stream); (void)hipStreamDestroy(ds.grad_stream); }
        ds.grad_rows.release();
        cugp_group_destroy(ds.group);
    }
    b->grad_host.release();
    for (cugp_gp* g : b->experts) cugp_destroy(g);
    b->pred_host.release();
    if (b->mode_stream) (void)hipStreamSynchronize(b->mode_stream);
    for (Scratch* sc : {&b->mode_rows, &b->mode_out, &b->mode_hout}) sc->release();
    if (b->mode_stream) (void)hipStreamDestroy(b->mode_stream);
    delete b;
    return CUGP_OK;
}

int cugp_bcm_kernel_kind(const cugp_bcm* b, int* kernel)
{
    if (!b || !kernel) return CUGP_ERR_INVALID;
    *kernel = b->kernel;
    return CUGP_OK;
}

int cugp_bcm_num_experts(const cugp_bcm* b, int* k)
{
    if (!b || !k) return CUGP_ERR_INVALID;
    *k = (int)b->experts.size();
    return CUGP_OK;
}

int cugp_bcm_expert(cugp_bcm* b, int k, cugp_gp** gp)
{
    if (!b || !gp || k < 0 || k >= (int)b->experts.size()) return CUGP_ERR_INVALID;
    *gp = b->experts[k];
    return CUGP_OK;
}

int cugp_bcm_set_expert_data(cugp_bcm* b, int k, const double* X, const double* y)
{
    if (!b || k < 0 || k >= (int)b->experts.size()) return CUGP_ERR_INVALID;
    return cugp_set_data(b->experts[k], X, y);
}

// ---- hyper-parameters and evaluation: the 3-entry calls and their _ard twins are argument checks (refuse_ard_bcm /
// want_ard_bcm) in front of one body over the BCM's nh entries and rows of 1 + nh doubles ----
static int bcm_set_theta(cugp_bcm* b, const double* hp)
{
    b->hp.assign(hp, hp + b->nh);
    for (cugp_gp* g : b->experts) {
        int rc = b->ard ? cugp_set_loghyper_ard(g, b->hp.data(), b->nh) : cugp_set_loghyper(g, b->hp.data());
        if (rc) return rc;
    }
    return CUGP_OK;
}

int cugp_bcm_set_loghyper(cugp_bcm* b, const double hp[3])
{
    if (!b || !hp) return CUGP_ERR_INVALID;
    if (const int rc = refuse_ard_bcm(b, "cugp_bcm_set_loghyper", "cugp_bcm_set_loghyper_ard")) return rc;
    return bcm_set_theta(b, hp);
}

int cugp_bcm_get_loghyper(const cugp_bcm* b, double hp[3])
{
    if (!b || !hp) return CUGP_ERR_INVALID;
    if (const int rc = refuse_ard_bcm(b, "cugp_bcm_get_loghyper", "cugp_bcm_get_loghyper_ard")) return rc;
    for (int i = 0; i < 3; i++) hp[i] = b->hp[i];
    return CUGP_OK;
}

int cugp_bcm_num_hyper(const cugp_bcm* b, int* nh)
{
    if (!b || !nh) return cugp_internal_fail(CUGP_ERR_INVALID, "cugp_bcm_num_hyper: null argument");
    *nh = b->nh;
    return CUGP_OK;
}

int cugp_bcm_nh(const cugp_bcm* b) { return b ? b->nh : 0; }
int cugp_bcm_dim(const cugp_bcm* b) { return b ? b->d : 0; }
int cugp_bcm_is_ard(const cugp_bcm* b) { return b && b->ard ? 1 : 0; }

int cugp_bcm_set_loghyper_ard(cugp_bcm* b, const double* hp, int nh)
{
    if (const int rc = want_ard_bcm(b, nh, "cugp_bcm_set_loghyper_ard", hp != nullptr)) return rc;
    return bcm_set_theta(b, hp);
}

int cugp_bcm_get_loghyper_ard(const cugp_bcm* b, double* hp, int nh)
{
    if (const int rc = want_ard_bcm(b, nh, "cugp_bcm_get_loghyper_ard", hp != nullptr)) return rc;
    for (int i = 0; i < nh; i++) hp[i] = b->hp[i];
    return CUGP_OK;
}

// after an error half-way through an evaluation: fetch whatever is still in flight (results ignored) so that no group
// or expert keeps its "pending" flag -- the next evaluation then starts from a clean state instead of finding the
// shared-launch path "already in flight" for ever
static void bcm_drain(cugp_bcm* b)
{
    std::vector<double> lk, gk3;
    for (DeviceSet& ds : b->sets) {
        if (ds.grouped_now && ds.group) {
            lk.assign(ds.idx.size(), 0.0);
            gk3.assign((size_t)b->nh * ds.idx.size(), 0.0);
            (void)cugp_group_fetch(ds.group, lk.data(), gk3.data());
        } else {
            double l;
            for (int k : ds.idx) (void)expert_fetch(b, b->experts[k], &l, nullptr);
        }
        ds.grouped_now = false;
    }
}

// all experts of all devices in flight (a group of shared launches per device where possible, else one stream
// per expert) before anything is read back
static int bcm_enqueue_all(cugp_bcm* b)
{
    for (DeviceSet& ds : b->sets) ds.grouped_now = false;
    for (DeviceSet& ds : b->sets) {
        if (ds.group) {
            const int rc = cugp_group_enqueue(ds.group, 1);
            if (rc == CUGP_OK) { ds.grouped_now = true; continue; }
            if (rc != CUGP_ERR_INVALID) { bcm_drain(b); return rc; }   // INVALID: not possible as a group right now
        }
        for (int k : ds.idx) {
            const int rc = cugp_loglik_grad_enqueue(b->experts[k], 1);
            if (rc) { bcm_drain(b); return rc; }
        }
    }
    return CUGP_OK;
}

// rows[k] = {LL_k, g_k[0..2]} for every expert of this handle, k in global order (what a multi-process BCM
// all-reduces across ranks)
static int bcm_rows(cugp_bcm* b, double* rows)
{
    int rc = bcm_enqueue_all(b);
    if (rc) return rc;
    const size_t nh = (size_t)b->nh, w = 1 + nh;
    std::vector<double> lk, gk3;
    for (DeviceSet& ds : b->sets) {
        const size_t n = ds.idx.size();
        lk.assign(n, 0.0);
        gk3.assign(nh * n, 0.0);
        if (ds.grouped_now) {
            if ((rc = cugp_group_fetch(ds.group, lk.data(), gk3.data()))) { ds.grouped_now = false; bcm_drain(b); return rc; }
            ds.grouped_now = false;
        } else {
            for (size_t i = 0; i < n; i++)
                if ((rc = expert_fetch(b, b->experts[ds.idx[i]], &lk[i], &gk3[nh * i]))) { bcm_drain(b); return rc; }
        }
        for (size_t i = 0; i < n; i++) {
            const size_t k = (size_t)ds.idx[i];
            rows[w * k] = lk[i];
            for (size_t j = 0; j < nh; j++) rows[w * k + 1 + j] = gk3[nh * i + j];
        }
    }
    return CUGP_OK;
}

int cugp_bcm_loglik_grad_rows(cugp_bcm* b, double* rows)
{
    if (!b || !rows) return CUGP_ERR_INVALID;
    if (const int rc = refuse_ard_bcm(b, "cugp_bcm_loglik_grad_rows", "cugp_bcm_loglik_grad_rows_ard")) return rc;
    return bcm_rows(b, rows);
}

// rows[k] = {LL_k, g_k[0 .. nh - 1]}
int cugp_bcm_loglik_grad_rows_ard(cugp_bcm* b, double* rows, int nh)
{
    if (const int rc = want_ard_bcm(b, nh, "cugp_bcm_loglik_grad_rows_ard", rows != nullptr)) return rc;
    return bcm_rows(b, rows);
}

// The same payload left ON THE DEVICE for a collective that never touches the host (RCCL all-reduce over
// xGMI in cugp_amd/bcm.py): row slot[k] of dev_rows ([.][4] doubles, device memory of the handle's first device,
// e.g. a zeroed buffer with one row per expert of the WHOLE model) receives {LL_k, g_k} of local expert k.
// Returns when the rows are in place (the evaluation itself is the wait); single-device handles only.
static int bcm_rows_device(cugp_bcm* b, double* dev_rows, const int* slot)
{
    if (b->sets.size() != 1) return CUGP_ERR_INVALID;
    const size_t nh = (size_t)b->nh, w = 1 + nh, srow = b->ard ? 8 + nh : 8;
    {   // dev_rows must be device memory of the handle's device (a host pointer or another GPU's buffer would fault
        // inside the copy kernels, or silently land elsewhere)
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, dev_rows) != hipSuccess || at.type != hipMemoryTypeDevice ||
            at.device != b->sets[0].device) {
            (void)hipGetLastError();
            return CUGP_ERR_INVALID;
        }
    }
    int rc = bcm_enqueue_all(b);
    if (rc) return rc;
    DeviceSet& ds = b->sets[0];
    const size_t n = ds.idx.size();
    // (every error return drains what was enqueued and clears grouped_now, like cugp_bcm_loglik_grad_rows: the next
    //  evaluation of the handle starts clean instead of failing once with CUGP_ERR_BUSY)
    if (ds.grouped_now) {
        const double* dout = nullptr;
        void* stream = nullptr;
        if ((rc = cugp_group_device_results(ds.group, &dout, &stream))) { bcm_drain(b); return rc; }   // (the group is still in flight: drained as a group)
        for (size_t i = 0; i < n; i++)
            if ((rc = b->ard ? cugp_pack_result_rows_n(dev_rows + w * (size_t)slot[ds.idx[i]], dout + srow * i, 1, b->nh, 1, stream)
                             : cugp_copy_device_row(dev_rows + 4 * (size_t)slot[ds.idx[i]], dout + 8 * i, stream))) { bcm_drain(b); return rc; }
        std::vector<double> lk(n), gk3(nh * n);
        rc = cugp_group_fetch(ds.group, lk.data(), gk3.data());       // waits for the stream: rows are in place
        ds.grouped_now = false;
        if (rc) bcm_drain(b);
        return rc;
    }
    for (size_t i = 0; i < n; i++) {
        cugp_gp* e = b->experts[ds.idx[i]];
        if ((rc = cugp_copy_result_row(e, dev_rows + w * (size_t)slot[ds.idx[i]]))) { bcm_drain(b); return rc; }
    }
    for (size_t i = 0; i < n; i++) {
        double l;
        if ((rc = expert_fetch(b, b->experts[ds.idx[i]], &l, nullptr))) { bcm_drain(b); return rc; }
    }
    return CUGP_OK;
}

int cugp_bcm_loglik_grad_rows_device(cugp_bcm* b, double* dev_rows, const int* slot)
{
    if (!b || !dev_rows || !slot) return CUGP_ERR_INVALID;
    if (const int rc = refuse_ard_bcm(b, "cugp_bcm_loglik_grad_rows_device", "cugp_bcm_loglik_grad_rows_device_ard")) return rc;
    return bcm_rows_device(b, dev_rows, slot);
}

// dev_rows: [.][1 + nh] doubles
int cugp_bcm_loglik_grad_rows_device_ard(cugp_bcm* b, double* dev_rows, const int* slot, int nh)
{
    if (const int rc = want_ard_bcm(b, nh, "cugp_bcm_loglik_grad_rows_device_ard", dev_rows && slot)) return rc;
    return bcm_rows_device(b, dev_rows, slot);
}

// The two halves of cugp_bcm_loglik_grad_allgather (comm.cpp) on the BCM's side.  enqueue: all experts in flight, their
// rows {LL, g} packed into dsend[i][1 + nh] (local order; 4 doubles for an isotropic BCM) BEHIND the evaluation on ITS stream, which is returned -- whatever
// the caller enqueues there next (the collective, the copy to the host) needs no host wait in between.  finish: waits
// for that stream and closes the evaluation (results into the handles, status word checked).
int cugp_bcm_enqueue_rows_packed(cugp_bcm* b, double* dsend, void** stream)
{
    if (!b || !dsend || !stream) return CUGP_ERR_INVALID;
    if (b->sets.size() != 1) return CUGP_ERR_INVALID;
    int rc = bcm_enqueue_all(b);
    if (rc) return rc;
    DeviceSet& ds = b->sets[0];
    const size_t n = ds.idx.size();
    if (ds.grouped_now) {
        const double* dout = nullptr;
        if ((rc = cugp_group_device_results(ds.group, &dout, stream)) ||
            (rc = cugp_pack_result_rows_n(dsend, dout, (int)n, b->nh, b->ard ? 1 : 0, *stream))) { bcm_drain(b); return rc; }
        return CUGP_OK;
    }
    // experts on streams of their own: every row behind its expert's evaluation; all but the first are waited for
    // here, so that what follows on the first expert's stream finds every row in place
    for (size_t i = 0; i < n; i++)
        if ((rc = cugp_copy_result_row(b->experts[ds.idx[i]], dsend + (size_t)(1 + b->nh) * i))) { bcm_drain(b); return rc; }
    for (size_t i = 1; i < n; i++) {
        double l;
        if ((rc = expert_fetch(b, b->experts[ds.idx[i]], &l, nullptr))) { bcm_drain(b); return rc; }
    }
    *stream = cugp_get_stream(b->experts[ds.idx[0]]);
    return CUGP_OK;
}

int cugp_bcm_finish_rows(cugp_bcm* b)
{
    if (!b || b->sets.size() != 1) return CUGP_ERR_INVALID;
    DeviceSet& ds = b->sets[0];
    int rc;
    if (ds.grouped_now) {
        std::vector<double> lk(ds.idx.size()), gk3((size_t)b->nh * ds.idx.size());
        rc = cugp_group_fetch(ds.group, lk.data(), gk3.data());
        ds.grouped_now = false;
        if (rc) bcm_drain(b);
        return rc;
    }
    double l;
    if ((rc = expert_fetch(b, b->experts[ds.idx[0]], &l, nullptr))) bcm_drain(b);
    return rc;
}

static int bcm_sums(cugp_bcm* b, double* ll, double* g, double* per_expert_ll)
{
    const size_t K = b->experts.size(), nh = (size_t)b->nh, w = 1 + nh;
    std::vector<double> rows(w * K), sg(nh, 0.0);
    int rc = bcm_rows(b, rows.data());
    if (rc) return rc;
    double sll = 0.0;
    for (size_t k = 0; k < K; k++) {
        const double l = rows[w * k];
        const double* gk = &rows[w * k + 1];
        sll = sll + l;                                   // BCM.cpp:190-194
        for (size_t i = 0; i < nh; i++) sg[i] = (k == 0) ? gk[i] : sg[i] + gk[i];   // BCM.cpp:161-173
        if (per_expert_ll) per_expert_ll[k] = l;
    }
    if (ll) *ll = sll;
    if (g)
        for (size_t i = 0; i < nh; i++) g[i] = sg[i];
    return CUGP_OK;
}

int cugp_bcm_loglik_grad(cugp_bcm* b, double* ll, double g[3], double* per_expert_ll)
{
    if (!b) return CUGP_ERR_INVALID;
    if (const int rc = refuse_ard_bcm(b, "cugp_bcm_loglik_grad", "cugp_bcm_loglik_grad_ard")) return rc;
    return bcm_sums(b, ll, g, per_expert_ll);
}

int cugp_bcm_loglik_grad_ard(cugp_bcm* b, double* ll, double* g, int nh, double* per_expert_ll)
{
    if (const int rc = want_ard_bcm(b, nh, "cugp_bcm_loglik_grad_ard")) return rc;
    return bcm_sums(b, ll, g, per_expert_ll);
}

// Round 5: experts whose inverse quantities are not valid for the current hyper-parameters (a prediction right after
// set_BCM_log_hyperparam, BCM.cpp:64-83 after :123-130) are brought up to date by ONE evaluation of the whole model -- the
// groups of shared launches -- instead of one by one inside cugp_predict (16 x 1500 rows: 18 ms -> one 2 ms evaluation),
// and every prediction then sees the experts in the state a BCM evaluation leaves them in, whatever came before.
static int bcm_refresh(cugp_bcm* b)
{
    for (cugp_gp* e : b->experts)
        if (!cugp_has_inverse(e)) {
            double ll;
            return bcm_sums(b, &ll, nullptr, nullptr);   // (at the BCM's own row width: an ARD BCM's nh-wide evaluation)
        }
    return CUGP_OK;
}

int cugp_bcm_predict_partial(cugp_bcm* b, const double* Xt, int nt, double* sum_prec, double* sum_prec_mean)
{
    if (!b || !Xt || nt <= 0 || !sum_prec || !sum_prec_mean) return CUGP_ERR_INVALID;
    // Stale experts first (bcm_refresh).  Then all experts' predictions are in flight before the first is read: each on
    // its own stream, results into one pinned buffer; the two product-of-experts sums are taken in expert order
    // (BCM.cpp:45-62).
    const size_t K = b->experts.size();
    int rc;
    if ((rc = bcm_refresh(b)) || (rc = b->pred_host.grow(K * 2 * (size_t)nt, nullptr))) return rc;
    size_t enq = 0;
    for (; enq < K && rc == CUGP_OK; enq++) rc = cugp_predict_enqueue(b->experts[enq], Xt, nt, b->pred_host.p + enq * 2 * nt);
    if (rc) enq--;                                          // (the failing one enqueued nothing that needs a fetch)
    for (size_t k = 0; k < enq; k++) {
        const int rf = cugp_predict_fetch(b->experts[k]);
        if (rf && rc == CUGP_OK) rc = rf;
    }
    if (rc) return rc;
    for (int i = 0; i < nt; i++) sum_prec[i] = sum_prec_mean[i] = 0.0;
    for (size_t k = 0; k < K; k++) {
        const double* m = b->pred_host.p + k * 2 * nt;
        const double* v = m + nt;
        for (int i = 0; i < nt; i++) {                   // BCM.cpp:51-55
            const double inv = 1.0 / v[i];
            sum_prec[i] += inv;
            sum_prec_mean[i] += inv * m[i];
        }
    }
    return CUGP_OK;
}

// "rows written" on `stream` -> `wait_stream` waits for it.  Event `local` of the device set (its local expert index),
// created on first use with the SET's device current -- the caller's state -- so it is only ever recorded on streams of
// the device it belongs to, whatever the device list.  Shared by every row producer of the BCM.
static int set_order_after(DeviceSet& ds, size_t local, void* stream, void* wait_stream)
{
    while (ds.ev.size() <= local) {
        hipEvent_t ev = nullptr;
        if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess)
            return cugp_internal_fail(CUGP_ERR_DEVICE, "hipEventCreateWithFlags");
        ds.ev.push_back(ev);
    }
    if (hipEventRecord(ds.ev[local], (hipStream_t)stream) != hipSuccess ||
        hipStreamWaitEvent((hipStream_t)wait_stream, ds.ev[local], 0) != hipSuccess)
        return cugp_internal_fail(CUGP_ERR_DEVICE, "hipEventRecord / hipStreamWaitEvent (prediction rows)");
    return CUGP_OK;
}

// The rows of cugp_bcm_predict_allgather (comm.cpp) for the experts of this handle, local order = global order of the
// handle.  As cugp_bcm_predict_partial: stale experts first brought up to date by ONE evaluation of the whole model.
// Then the experts of the device predict as ONE group of batched launches where they can, else each on its own stream
// (the cugp_bcm_enqueue_rows_packed pattern); wait_stream is ordered behind every stream that writes rows by events.
int cugp_bcm_predict_rows_enqueue(cugp_bcm* b, int device, const double* Xt, int nt, double* dsend, size_t slot_stride,
                                  void* wait_stream)
{
    return cugp_bcm_predict_rows_enqueue_form(b, device, Xt, nt, dsend, slot_stride, wait_stream, 0);
}

int cugp_bcm_predict_rows_enqueue_form(cugp_bcm* b, int device, const double* Xt, int nt, double* dsend,
                                       size_t slot_stride, void* wait_stream, int latent)
{
    if (!b || !Xt || nt <= 0 || !dsend || !wait_stream) return CUGP_ERR_INVALID;
    if (b->sets.size() != 1 || b->sets[0].device != device)
        return cugp_internal_fail(CUGP_ERR_INVALID, "cugp_bcm_predict_allgather: the BCM's experts are not all on the communicator's device");
    int rc;
    if ((rc = bcm_refresh(b))) return rc;
    DeviceSet& ds = b->sets[0];
    const size_t n = ds.idx.size();
    if (hipSetDevice(device) != hipSuccess) return cugp_internal_fail(CUGP_ERR_DEVICE, "hipSetDevice");
    if (ds.group) {
        void* s = nullptr;
        rc = cugp_group_predict_enqueue_form(ds.group, Xt, nt, dsend, slot_stride, &s, latent);
        if (rc == CUGP_OK) return set_order_after(ds, 0, s, wait_stream);
        if (rc != CUGP_ERR_INVALID) return rc;               // INVALID: not possible as a group right now
    }
    for (size_t i = 0; i < n; i++) {
        void* s = nullptr;
        if ((rc = cugp_predict_rows_enqueue_form(b->experts[ds.idx[i]], Xt, nt, dsend + i * slot_stride, &s, latent)))
            return rc;
        if ((rc = set_order_after(ds, i, s, wait_stream))) return rc;
    }
    return CUGP_OK;
}

int cugp_bcm_predict_rows_finish(cugp_bcm* b)
{
    if (!b) return CUGP_ERR_INVALID;
    int rc = CUGP_OK;
    for (cugp_gp* e : b->experts) {
        const int r = cugp_predict_fetch(e);
        if (r && rc == CUGP_OK) rc = r;
    }
    return rc;
}

int cugp_poe_finish(const double* sum_prec, const double* sum_prec_mean, int nt, double* mean, double* var)
{
    if (!sum_prec || !sum_prec_mean || !mean || !var || nt <= 0) return CUGP_ERR_INVALID;
    for (int i = 0; i < nt; i++) {                       // BCM.cpp:56-60
        const double tv = 1.0 / sum_prec[i];
        var[i] = tv;
        mean[i] = tv * sum_prec_mean[i];
    }
    return CUGP_OK;
}

int cugp_bcm_predict(cugp_bcm* b, const double* Xt, int nt, double* mean, double* var)
{
    if (!b || nt <= 0) return CUGP_ERR_INVALID;
    std::vector<double> sp(nt), spm(nt);
    int rc = cugp_bcm_predict_partial(b, Xt, nt, sp.data(), spm.data());
    if (rc) return rc;
    return cugp_poe_finish(sp.data(), spm.data(), nt, mean, var);
}

// ---- combination rules on latent expert distributions (include/cugp.h: CUGP_COMBINE_*) ----
// Host twin of k_poe_reduce_mode (predict_gfx950.h): the same operations in the same order, every one rounded on its own.
int cugp_poe_combine(const double* rows, int K, int nt, int mode, double sf2, double sn2, int with_noise, double* mean,
                     double* var)
{
#pragma clang fp contract(off)
    if (!rows || !mean || !var || K <= 0 || nt <= 0 || mode < CUGP_COMBINE_POE || mode > CUGP_COMBINE_RBCM)
        return cugp_internal_fail(CUGP_ERR_INVALID, "cugp_poe_combine: null argument, K <= 0, nt <= 0 or an unknown mode");
    const double bg = 1.0 / (double)K;
    for (int t = 0; t < nt; t++) {
        double sp = 0.0, spm = 0.0, sb = 0.0;
        for (int k = 0; k < K; k++) {
            const double* r = rows + (size_t)k * 2 * nt;
            const double p = r[t], pm = r[nt + t];
            double beta = 1.0;
            if (mode == CUGP_COMBINE_GPOE) beta = bg;
            else if (mode == CUGP_COMBINE_RBCM) beta = 0.5 * std::log(sf2 * p);
            sp = sp + beta * p;
            spm = spm + beta * pm;
            sb = sb + beta;
        }
        double prec = sp;
        if (mode >= CUGP_COMBINE_BCM) prec = sp + (1.0 - sb) / sf2;
        const double tv = 1.0 / prec;
        mean[t] = tv * spm;
        var[t] = with_noise ? tv + sn2 : tv;
    }
    return CUGP_OK;
}

int cugp_bcm_prior_scalars(const cugp_bcm* b, double* sf2, double* sn2)
{
    if (!b || !sf2 || !sn2) return CUGP_ERR_INVALID;
    *sf2 = std::exp(b->hp[b->nh - 2] * 2);          // (cugp_capi.cpp: scalars)
    *sn2 = std::exp(b->hp[b->nh - 1] * 2);
    return CUGP_OK;
}

// One device set: the experts' latent rows as one group of batched launches (else expert by expert) into the BCM's own
// buffer, laid out as the block of a world of one, k_poe_reduce_mode behind them on the BCM's stream, one copy, one host
// wait.  Several device sets: every expert's latent mean and variance into pinned host memory, all in flight before the
// first is read (cugp_bcm_predict_partial's pattern), the rows formed as poe_row forms them, then cugp_poe_combine.
int cugp_bcm_predict_mode(cugp_bcm* b, const double* Xt, int nt, int mode, int with_noise, double* mean, double* var)
{
    if (!b || !Xt || nt <= 0 || !mean || !var || mode < CUGP_COMBINE_POE || mode > CUGP_COMBINE_RBCM)
        return cugp_internal_fail(CUGP_ERR_INVALID, "cugp_bcm_predict_mode: null argument, nt <= 0 or an unknown mode");
    const size_t K = b->experts.size();
    double sf2, sn2;
    int rc;
    if ((rc = cugp_bcm_prior_scalars(b, &sf2, &sn2)) || (rc = bcm_refresh(b))) return rc;
    if (b->sets.size() == 1) {
        const int device = b->sets[0].device;
        if (hipSetDevice(device) != hipSuccess) return cugp_internal_fail(CUGP_ERR_DEVICE, "hipSetDevice");
        if (!b->mode_stream && hipStreamCreateWithFlags(&b->mode_stream, hipStreamNonBlocking) != hipSuccess)
            return cugp_internal_fail(CUGP_ERR_DEVICE, "hipStreamCreateWithFlags (cugp_bcm_predict_mode)");
        const size_t rstride = 2 + K * 2 * (size_t)nt, nout = 2 * (size_t)nt + 2;
        if ((rc = b->mode_rows.grow(rstride, b->mode_stream)) || (rc = b->mode_out.grow(nout, b->mode_stream)) ||
            (rc = b->mode_hout.grow(nout, b->mode_stream)))
            return rc;
        // the block's header {status, count}: zeros -- nothing reads them here, but the kernel copies them to its output
        if (hipMemsetAsync(b->mode_rows.p, 0, 2 * sizeof(double), b->mode_stream) != hipSuccess)
            return cugp_internal_fail(CUGP_ERR_DEVICE, "hipMemsetAsync (cugp_bcm_predict_mode)");
        rc = cugp_bcm_predict_rows_enqueue_form(b, device, Xt, nt, b->mode_rows.p + 2, 2 * (size_t)nt, b->mode_stream, 1);
        if (rc == CUGP_OK)
            rc = cugp_poe_reduce_mode_enqueue(b->mode_rows.p, rstride, 1, (int)K, nt, mode, sf2, sn2, with_noise ? 1 : 0,
                                              b->mode_out.p, b->mode_stream);
        if (rc == CUGP_OK && hipMemcpyAsync(b->mode_hout.p, b->mode_out.p, nout * sizeof(double), hipMemcpyDeviceToHost,
                                            b->mode_stream) != hipSuccess)
            rc = cugp_internal_fail(CUGP_ERR_DEVICE, "hipMemcpyAsync (cugp_bcm_predict_mode)");
        if (hipStreamSynchronize(b->mode_stream) != hipSuccess && rc == CUGP_OK)     // the one host wait
            rc = cugp_internal_fail(CUGP_ERR_DEVICE, "hipStreamSynchronize (cugp_bcm_predict_mode)");
        const int rf = cugp_bcm_predict_rows_finish(b);        // (streams already done: closes them)
        if (rc == CUGP_OK) rc = rf;
        if (rc) return rc;
        memcpy(mean, b->mode_hout.p, (size_t)nt * sizeof(double));
        memcpy(var, b->mode_hout.p + nt, (size_t)nt * sizeof(double));
        return CUGP_OK;
    }
    if ((rc = b->pred_host.grow(K * 2 * (size_t)nt, nullptr))) return rc;
    size_t enq = 0;
    for (; enq < K && rc == CUGP_OK; enq++)
        rc = cugp_predict_enqueue_form(b->experts[enq], Xt, nt, b->pred_host.p + enq * 2 * nt, 1);
    if (rc) enq--;                                          // (the failing one enqueued nothing that needs a fetch)
    for (size_t k = 0; k < enq; k++) {
        const int rf = cugp_predict_fetch(b->experts[k]);
        if (rf && rc == CUGP_OK) rc = rf;
    }
    if (rc) return rc;
    for (size_t k = 0; k < K; k++) {                        // (m, var_f) -> (1/var_f, m/var_f) in place: poe_row's operations
#pragma clang fp contract(off)
        double* m = b->pred_host.p + k * 2 * nt;
        double* v = m + nt;
        for (int i = 0; i < nt; i++) {
            const double inv = 1.0 / v[i], pm = inv * m[i];
            m[i] = inv;
            v[i] = pm;
        }
    }
    return cugp_poe_combine(b->pred_host.p, (int)K, nt, mode, sf2, sn2, with_noise, mean, var);
}

// ---- gradients of the combined prediction with respect to the test inputs (include/cugp.h: cugp_poe_combine_grad) ----
// The chain rule of the rules above on the experts' (mean, variance) and their gradients, experts in order, every operation
// rounded on its own.  Per test point: p_k = 1 / v_k, beta_k and prec as cugp_poe_combine forms them (from v_k here, not from
// rows); then per input dimension
//   dp = -dv / v^2,  dbeta = 0 | -1/2 dv / v (rbcm),  a_k = dbeta p + beta dp,  dprec = sum a_k - [bcm, rbcm] (sum dbeta) / sf2
//   dvar = -dprec / prec^2
//   dmean = dvar S + dS / prec,  S = sum beta p m,  dS = sum (a_k m_k + beta p dm_k), evaluated as
//         = sum w_k dm_k + (sum a_k (m_k - mean)) / prec + [bcm, rbcm] mean ((sum dbeta) / sf2) / prec,
//     w_k = (beta_k p_k) / prec,  mean = sum w_k m_k
// -- the same expression (dS - mean dprec) / prec with the DIFFERENCE m_k - mean formed first: dvar S and dS / prec are each
// of the size of |dv p m| and cancel to the size of dm where the experts agree (one expert: w = 1, mean = m and dmean = dm
// exactly).  CUGP_COMBINE_REFERENCE takes POE's arithmetic: the caller passes the experts' NOISY variances (their gradients
// are the latent ones').
int cugp_poe_combine_grad(const double* mean, const double* var, const double* dmean, const double* dvar, int K, int nt,
                          int d, int mode, double sf2, double* out_dmean, double* out_dvar)
{
#pragma clang fp contract(off)
    if (!mean || !var || !dmean || !dvar || !out_dmean || !out_dvar || K <= 0 || nt <= 0 || d <= 0 ||
        mode < CUGP_COMBINE_REFERENCE || mode > CUGP_COMBINE_RBCM)
        return cugp_internal_fail(CUGP_ERR_INVALID,
                                  "cugp_poe_combine_grad: null argument, K <= 0, nt <= 0, d <= 0 or an unknown mode");
    const double bg = 1.0 / (double)K;
    const bool prior = mode >= CUGP_COMBINE_BCM;
    std::vector<double> pk(K), bk(K), wk(K);
    for (int t = 0; t < nt; t++) {
        double sp = 0.0, sb = 0.0;
        for (int k = 0; k < K; k++) {
            const double p = 1.0 / var[(size_t)k * nt + t];
            double beta = 1.0;
            if (mode == CUGP_COMBINE_GPOE) beta = bg;
            else if (mode == CUGP_COMBINE_RBCM) beta = 0.5 * std::log(sf2 * p);
            pk[k] = p;
            bk[k] = beta;
            wk[k] = beta * p;
            sp = sp + wk[k];
            sb = sb + beta;
        }
        double prec = sp;
        if (prior) prec = sp + (1.0 - sb) / sf2;
        double mu = 0.0;
        for (int k = 0; k < K; k++) {
            wk[k] = wk[k] / prec;
            mu = mu + wk[k] * mean[(size_t)k * nt + t];
        }
        for (int c = 0; c < d; c++) {
            double dprec = 0.0, sdm = 0.0, sam = 0.0, sdb = 0.0;
            for (int k = 0; k < K; k++) {
                const size_t e = ((size_t)k * nt + t) * d + c;
                const double v = var[(size_t)k * nt + t], dv = dvar[e];
                double a = bk[k] * -(dv / (v * v));
                if (mode == CUGP_COMBINE_RBCM) {
                    const double db = -0.5 * (dv / v);
                    a = db * pk[k] + a;
                    sdb = sdb + db;
                }
                dprec = dprec + a;
                sdm = sdm + wk[k] * dmean[e];
                sam = sam + a * (mean[(size_t)k * nt + t] - mu);
            }
            double dmo = sdm + sam / prec;
            if (prior) {
                const double pr = sdb / sf2;
                dprec = dprec - pr;
                dmo = dmo + (mu * pr) / prec;
            }
            out_dvar[(size_t)t * d + c] = -(dprec / (prec * prec));
            out_dmean[(size_t)t * d + c] = dmo;
        }
    }
    return CUGP_OK;
}

// The gradient rows of one device set (its device current), local expert i's at drows + i * slot_stride: ONE group of
// batched launches where the experts can run as one (*grouped), else each expert on its own stream.  *done: the stream
// behind which every row is written -- wait_stream, ordered behind the writers by events; wait_stream null: the group's
// own stream, or (expert by expert) the set's grad_stream, created here.  No host wait.
static int set_grad_rows_enqueue(cugp_bcm* b, DeviceSet& ds, const double* Xt, int nt, double* drows, size_t slot_stride,
                                 int latent, int want_dvar, void* wait_stream, void** done, bool* grouped)
{
    int rc;
    *grouped = false;
    if (ds.group) {
        void* s = nullptr;
        rc = cugp_group_predict_grad_enqueue(ds.group, Xt, nt, drows, slot_stride, &s, latent, want_dvar);
        if (rc == CUGP_OK) {
            *grouped = true;
            *done = wait_stream ? wait_stream : s;
            return wait_stream ? set_order_after(ds, 0, s, wait_stream) : CUGP_OK;
        }
        if (rc != CUGP_ERR_INVALID) return rc;               // INVALID: not possible as a group right now
    }
    if (!wait_stream) {
        if (!ds.grad_stream && hipStreamCreateWithFlags(&ds.grad_stream, hipStreamNonBlocking) != hipSuccess)
            return cugp_internal_fail(CUGP_ERR_DEVICE, "hipStreamCreateWithFlags (cugp_bcm_predict_grad)");
        wait_stream = ds.grad_stream;
    }
    *done = wait_stream;
    for (size_t i = 0; i < ds.idx.size(); i++) {
        void* s = nullptr;
        if ((rc = cugp_predict_grad_rows_enqueue(b->experts[ds.idx[i]], Xt, nt, drows + i * slot_stride, &s, latent, want_dvar)))
            return rc;
        if ((rc = set_order_after(ds, i, s, wait_stream))) return rc;
    }
    return CUGP_OK;
}

// cugp_bcm_predict_rows_enqueue_form with gradient rows ([m nt | v nt | dmean nt d | dvar nt d] per slot): the BCM's side of
// cugp_bcm_predict_grad_allgather (comm.cpp).  cugp_bcm_predict_rows_finish waits for the experts' streams.
int cugp_bcm_predict_grad_rows_enqueue(cugp_bcm* b, int device, const double* Xt, int nt, double* dsend,
                                       size_t slot_stride, void* wait_stream, int latent, int want_dvar)
{
    if (!b || !Xt || nt <= 0 || !dsend || !wait_stream) return CUGP_ERR_INVALID;
    if (b->sets.size() != 1 || b->sets[0].device != device)
        return cugp_internal_fail(CUGP_ERR_INVALID, "cugp_bcm_predict_grad_allgather: the BCM's experts are not all on the communicator's device");
    int rc;
    if ((rc = bcm_refresh(b))) return rc;
    if (hipSetDevice(device) != hipSuccess) return cugp_internal_fail(CUGP_ERR_DEVICE, "hipSetDevice");
    void* done = nullptr;
    bool grouped = false;
    rc = set_grad_rows_enqueue(b, b->sets[0], Xt, nt, dsend, slot_stride, latent, want_dvar, wait_stream, &done, &grouped);
    if (rc == CUGP_OK) b->grad_form = grouped ? 2 : 1;
    return rc;
}

int cugp_bcm_predict_grad_form(const cugp_bcm* b, int* form)
{
    if (!b || !form) return cugp_internal_fail(CUGP_ERR_INVALID, "cugp_bcm_predict_grad_form: null argument");
    *form = b->grad_form;
    return CUGP_OK;
}

// Every expert's gradient rows [m nt | v nt | dmean nt d | dvar nt d] in flight before the first wait: per device set ONE
// group of batched launches (cugp_group_predict_grad_enqueue) where its experts can run as one, else expert by expert on
// their own streams (cugp_predict_grad_rows_enqueue), and one copy per set into pinned host memory behind them -- a BCM
// over several devices of one process works.  Then the rule on the host, exactly as before the batched path: mode >= 0:
// the experts' latent distributions through rows made as poe_row makes them and cugp_poe_combine;
// CUGP_COMBINE_REFERENCE: their noisy predictions through the two sums of cugp_bcm_predict_partial and cugp_poe_finish
// (with_noise is then not read); cugp_poe_combine_grad for the gradients -- which reads every expert's dvar for the
// mean's gradient too, so the experts' V = W L^-1 is always computed.  Stale experts are refreshed first, as every BCM
// prediction does.
int cugp_bcm_predict_grad(cugp_bcm* b, const double* Xt, int nt, int mode, int with_noise, double* mean, double* var,
                          double* dmean, double* dvar)
{
    if (!b || !Xt || nt <= 0 || (!dmean && !dvar) || mode < CUGP_COMBINE_REFERENCE || mode > CUGP_COMBINE_RBCM)
        return cugp_internal_fail(CUGP_ERR_INVALID,
                                  "cugp_bcm_predict_grad: null BCM or Xt, nt <= 0, neither dmean nor dvar given, or an unknown mode");
    const size_t K = b->experts.size(), d = (size_t)b->d, n1 = (size_t)nt, nd = n1 * d, slot = 2 * n1 + 2 * nd;
    const bool reference = mode == CUGP_COMBINE_REFERENCE;
    double sf2, sn2;
    int rc;
    if ((rc = cugp_bcm_prior_scalars(b, &sf2, &sn2)) || (rc = bcm_refresh(b)) || (rc = b->grad_host.grow(K * slot, nullptr)))
        return rc;
    const size_t nsets = b->sets.size();
    std::vector<void*> done(nsets, nullptr);
    std::vector<size_t> first(nsets, 0);                   // the set's first slot in the pinned buffer
    bool all_grouped = true;
    size_t enq = 0, off = 0;
    for (; enq < nsets && rc == CUGP_OK; enq++) {
        DeviceSet& ds = b->sets[enq];
        first[enq] = off;
        off += ds.idx.size();
        if (hipSetDevice(ds.device) != hipSuccess) { rc = cugp_internal_fail(CUGP_ERR_DEVICE, "hipSetDevice"); break; }
        if ((rc = ds.grad_rows.grow(ds.idx.size() * slot, nullptr))) break;
        bool grouped = false;
        rc = set_grad_rows_enqueue(b, ds, Xt, nt, ds.grad_rows.p, slot, reference ? 0 : 1, 1, nullptr, &done[enq], &grouped);
        all_grouped = all_grouped && grouped;
        if (rc == CUGP_OK && hipMemcpyAsync(b->grad_host.p + first[enq] * slot, ds.grad_rows.p, ds.idx.size() * slot * sizeof(double),
                                            hipMemcpyDeviceToHost, (hipStream_t)done[enq]) != hipSuccess)
            rc = cugp_internal_fail(CUGP_ERR_DEVICE, "hipMemcpyAsync (cugp_bcm_predict_grad)");
    }
    // the waits: every set's copy, then every expert's own stream (already done: closes its profiling events) -- after a
    // failure too, so that nothing enqueued still writes rows when the call returns
    for (size_t si = 0; si < nsets; si++)
        if (done[si] && (hipSetDevice(b->sets[si].device) != hipSuccess || hipStreamSynchronize((hipStream_t)done[si]) != hipSuccess) &&
            rc == CUGP_OK)
            rc = cugp_internal_fail(CUGP_ERR_DEVICE, "hipStreamSynchronize (cugp_bcm_predict_grad)");
    for (cugp_gp* e : b->experts) {
        const int rf = cugp_predict_fetch(e);
        if (rf && rc == CUGP_OK) rc = rf;
    }
    if (rc) return rc;
    b->grad_form = all_grouped ? 2 : 1;
    std::vector<double> m(K * n1), v(K * n1), dm(K * nd), dv(K * nd), rows(K * 2 * n1), om(n1), ov(n1), odm(nd), odv(nd);
    for (size_t si = 0; si < nsets; si++)
        for (size_t i = 0; i < b->sets[si].idx.size(); i++) {  // expert order for the host sums
            const size_t k = (size_t)b->sets[si].idx[i];
            const double* r = b->grad_host.p + (first[si] + i) * slot;
            memcpy(m.data() + k * n1, r, n1 * sizeof(double));
            memcpy(v.data() + k * n1, r + n1, n1 * sizeof(double));
            memcpy(dm.data() + k * nd, r + 2 * n1, nd * sizeof(double));
            memcpy(dv.data() + k * nd, r + 2 * n1 + nd, nd * sizeof(double));
        }
    if (reference) {
        std::vector<double> sp(n1, 0.0), spm(n1, 0.0);
        for (size_t k = 0; k < K; k++)
            for (size_t i = 0; i < n1; i++) {                  // BCM.cpp:51-55, as cugp_bcm_predict_partial
                const double inv = 1.0 / v[k * n1 + i];
                sp[i] += inv;
                spm[i] += inv * m[k * n1 + i];
            }
        if ((rc = cugp_poe_finish(sp.data(), spm.data(), nt, om.data(), ov.data()))) return rc;
    } else {
        for (size_t k = 0; k < K; k++)
            for (size_t i = 0; i < n1; i++) {                  // poe_row's operations
#pragma clang fp contract(off)
                const double inv = 1.0 / v[k * n1 + i], pm = inv * m[k * n1 + i];
                rows[k * 2 * n1 + i] = inv;
                rows[k * 2 * n1 + n1 + i] = pm;
            }
        if ((rc = cugp_poe_combine(rows.data(), (int)K, nt, mode, sf2, sn2, with_noise, om.data(), ov.data()))) return rc;
    }
    if ((rc = cugp_poe_combine_grad(m.data(), v.data(), dm.data(), dv.data(), (int)K, nt, (int)d, mode, sf2, odm.data(),
                                    odv.data())))
        return rc;
    if (mean) memcpy(mean, om.data(), n1 * sizeof(double));
    if (var) memcpy(var, ov.data(), n1 * sizeof(double));
    if (dmean) memcpy(dmean, odm.data(), nd * sizeof(double));
    if (dvar) memcpy(dvar, odv.data(), nd * sizeof(double));
    return CUGP_OK;
}

namespace {
void bcm_objective(void* ctx, const double th[3], double* f, double g[3])
{
    cugp_bcm* b = (cugp_bcm*)ctx;
    double ll = NAN;
    cugp_bcm_set_loghyper(b, th);
    if (cugp_bcm_loglik_grad(b, &ll, g, nullptr) != CUGP_OK) { ll = NAN; g[0] = g[1] = g[2] = NAN; }
    *f = -1.0 * ll;
}
void bcm_objective_n(void* ctx, const double* th, int nh, double* f, double* g)
{
    cugp_bcm* b = (cugp_bcm*)ctx;
    double ll = NAN;
    if (bcm_set_theta(b, th) != CUGP_OK || bcm_sums(b, &ll, g, nullptr) != CUGP_OK) {
        ll = NAN;
        for (int i = 0; i < nh; i++) g[i] = NAN;
    }
    *f = -1.0 * ll;
}
}  // namespace

// conjugate gradients over the nh entries of an ARD BCM from its current hyper-parameters; the end point stays set.
// trace (may be NULL): rows of nh + 1 doubles [theta_0 .. theta_{nh-1}, f]
int cugp_bcm_cg_solve_ard(cugp_bcm* b, int budget, double* trace, int trace_cap, int* nevals)
{
    if (!b) return cugp_internal_fail(CUGP_ERR_INVALID, "cugp_bcm_cg_solve_ard: null handle");
    if (const int rc = want_ard_bcm(b, b->ard ? b->nh : 3, "cugp_bcm_cg_solve_ard")) return rc;
    std::vector<double> th(b->hp);
    if (const int rc = cugp_cg_minimize_n(bcm_objective_n, b, th.data(), b->nh, budget, trace, trace_cap, nevals)) return rc;
    return bcm_set_theta(b, th.data());
}

int cugp_bcm_cg_solve(cugp_bcm* b, int budget, double* trace, int trace_cap, int* nevals)
{
    if (!b) return CUGP_ERR_INVALID;
    if (const int rc = refuse_ard_bcm(b, "cugp_bcm_cg_solve", "cugp_bcm_cg_solve_ard")) return rc;
    double th[3] = {b->hp[0], b->hp[1], b->hp[2]};
    int rc = cugp_cg_minimize(bcm_objective, b, th, budget, trace, trace_cap, nevals);
    if (rc) return rc;
    return cugp_bcm_set_loghyper(b, th);
}

}  // extern "C"
