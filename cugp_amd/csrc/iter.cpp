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
    // the solver's precision (cugp_iter_set_precision): mixed runs the sweeps on k_cov_apply32
    bool mixed = false;
    double cycle_drop = CUGP_ITER_CYCLE_DROP;
    int stats[4] = {0, 0, 0, 0};   // fp32 products, fp64 products, verifications, fell back: the last solving call's
    Scratch vb, vx, vr, vp, vq, vk, alpha, apart, dpart, xt, res;
    Scratch xpart, xout;           // the test-input gradients: k_cov_xgrad's partial sums; dmean, dvar [nt][d]
    Scratch gpart, gout, ghost;    // the gradient forms: k_cov_grad's partial rows; their sums and the
                                   // columns' u'v behind them; the pinned copy of those
    Scratch fom, fb, forg, fw, fout;   // the pathwise draws: Omega [m][d], b [m], the origin [d], W [m][tp];
                                   // Phi W [nq][tp]
    std::vector<double> host;      // packing: [t][n] target-major <-> [n][tp]
    // the preconditioner (cugp_iter_set_precond): M = L L' + sn2 I from a pivoted Cholesky factor of Kf
    int pc_rank = 0, pc_got = 0, pc_rp = 0;       // asked for, achieved, padded (pc_plan)
    bool pc_built = false;         // L, Q hold for (data, theta, pc_rank); a rank of 0 is built as it stands
    Scratch pL, pQ, pdres, pshv, pint, ppart, pT, vz;   // L, Q [n][rp]; residual diagonal; argmax shares; piv, ctl and the
                                   // shares' rows (ints); partial blocks of Q'R; T = Q'R; z = M^-1 r
    cugp_gp* pf = nullptr;         // the r x r side: an ordinary handle whose A receives C = sn2 I + L'L (as sparse.cpp's B)
    int pf_n = 0;                  // ... the size it was created for
    std::vector<int> hpiv;         // the pivots and ctl as read back: [rp + 2]
    // the Lanczos quadrature (cugp_iter_loglik): a solve's log of (a_j, b_j) with its lengths and start
    // weights, k_slq_quad's scratch, the probes' quadratures [t], the call's three sums, their pinned copy, G1 [r][tp]
    Scratch lrec, lmeta, lwork, lquad, lout, lhost, pg1;
    // the variance cache (cugp_iter_varcache_build): Q, R [n][rp]; the working blocks W, W2, P [n][16];
    // C = Q'W [rp][16] and its partial blocks; both passes' coefficients Hc [rp][16]; H, its factor S [rp][rp]; the small side
    // (Ti [16][16], the columns' norms [16], a unit HyperScalars for k_pc_correct's division, ctl); k_cov_var's sums
    bool vc_valid = false;         // Q, R, H hold for (data, theta); dropped by set_data, set_loghyper and a new build
    int vc_rank = 0, vc_got = 0, vc_rp = 0, vc_products = 0, vc_reason = 0, vc_bw = 1;
    Scratch vcQ, vcR, vcW, vcW2, vcP, vcC, vcpart, vcHc, vcH, vcS, vcsm, vcg;
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

// out [na][tp] = k(A, X) V (+ sn2 V: square, A == X) on the handle's stream; f32: the mixed mode's product
int product(cugp_iter* h, const CovFn& cf, const double* A, int na, const double* V, int tp, double* out, bool square,
            bool f32 = false)
{
    const IterPlan pl = iter_apply_plan(na, h->n, h->split);
    int rc;
    if (pl.split > 1 && (rc = h->apart.grow((size_t)pl.split * na * tp, h->stream))) return rc;
    if (f32) launch_cov_apply32(A, na, h->dX, h->n, h->d, cf, V, tp, out, h->apart.p, pl, square, h->stream);
    else launch_cov_apply(A, na, h->dX, h->n, h->d, cf, V, tp, out, h->apart.p, pl, square, h->stream);
    return CUGP_OK;
}

struct Counts { int active, waiting, stalled; };
// rows: SC_ROWS, or SC_ALLOC while the mixed mode's sweeps run (the stall flags lie behind the rows of the fp64 mode)
int read_status(cugp_iter* h, int tp, const char* call, Counts* k, int rows = SC_ROWS)
{
    hipError_t e = hipGetLastError();
    if (e == hipSuccess)
        e = hipMemcpyAsync(h->hsc, h->dsc, (size_t)rows * IT_MAXT * sizeof(double), hipMemcpyDeviceToHost, h->stream);
    if (const int rc = sync_or_fail(h->stream, call, e)) return rc;
    k->active = k->waiting = k->stalled = 0;
    for (int c = 0; c < tp; c++) {
        const double st = h->hsc[SC_STATE * IT_MAXT + c];
        k->active += st == ST_ACTIVE || st == ST_RESTART;
        k->waiting += st == ST_CANDIDATE;
        if (rows > SC_STALL) k->stalled += h->hsc[SC_STALL * IT_MAXT + c] != 0.0;
    }
    return CUGP_OK;
}

// The factor and the r x r side for the handle's data, theta and rank as they stand; one wait behind the factor's launches
// (the device decides where it ends), one around the small factorisation.
int precond_build(cugp_iter* h, const char* call)
{
    if (h->pc_built) return CUGP_OK;
    const int n = h->n, rank = h->pc_rank;
    h->pc_got = h->pc_rp = 0;
    if (rank == 0) { h->pc_built = true; return CUGP_OK; }
    const CovFn cf = cov_of(h);
    hipStream_t s = h->stream;
    const PcPlan pl = pc_plan(n, rank);
    const int rp = pl.rp, nwg = pchol_blocks(n);
    int rc;
    if ((rc = h->pL.grow((size_t)n * rp, s)) || (rc = h->pQ.grow((size_t)n * rp, s)) || (rc = h->pdres.grow(n, s)) ||
        (rc = h->pshv.grow((size_t)2 * nwg, s)) || (rc = h->pint.grow(((size_t)rp + 2 + 2 * (size_t)nwg + 1) / 2, s)) ||
        (rc = h->ppart.grow((size_t)pl.blocks * rp * IT_MAXT, s)) || (rc = h->pT.grow((size_t)rp * IT_MAXT, s)))
        return rc;
    int *piv = (int*)h->pint.p, *ctl = piv + rp, *shi = ctl + 2;
    double* L = h->pL.p;
    launch_pchol_init(cf, h->d, n, rp, L, h->pdres.p, piv, ctl, s);
    for (int k = 0; k <= rank; k++) launch_pchol_step(h->dX, n, h->d, cf, L, rp, h->pdres.p, piv, ctl, h->pshv.p, shi, k, rank, s);
    h->hpiv.assign(rp + 2, -1);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(h->hpiv.data(), piv, (size_t)(rp + 2) * sizeof(int), hipMemcpyDeviceToHost, s);
    if ((rc = sync_or_fail(s, call, e))) return rc;
    int got = std::max(0, std::min(h->hpiv[rp], rank));
    if (h->hpiv[rp + 1]) {                                // a NaN residual: no factor at all, the recurrences run plain
        got = 0;
        HIPCHK(hipMemsetAsync(L, 0, (size_t)n * rp * sizeof(double), s));
        HIPCHK(hipStreamSynchronize(s));
    }
    h->pc_got = got;
    h->pc_rp = rp;
    if (got == 0) { h->pc_built = true; return CUGP_OK; }
    if (!h->pf || h->pf_n != rp) {
        if (h->pf) cugp_destroy(h->pf);
        h->pf = nullptr;
        if ((rc = cugp_create(rp, 1, h->device, &h->pf))) return rc;
        h->pf_n = rp;
        if ((rc = ensure_factor_bufs(h->pf)) || (rc = ensure_inverse_bufs(h->pf))) return rc;
    }
    cugp_gp* f = h->pf;
    launch_pc_eye(f->dA, f->npad, s);
    for (int c0 = 0; c0 < rp; c0 += 64) {                 // C = sn2 I + L'L, a 64-column group at a time
        launch_pc_project(L, L + c0, rp, IT_MAXT, n, pl, h->ppart.p, s);
        launch_pc_gram_finish(h->ppart.p, pl.blocks, rp, cf.hd, f->dA, f->npad, c0, s);
    }
    if ((rc = sync_or_fail(s, call, hipGetLastError()))) return rc;
    if ((rc = la_factor_inverse(f, true))) return rc;    // Lc, Lc^-1, Lc^-T (its own stream, waited for)
    for (int c0 = 0; c0 < rp; c0 += 64) launch_pc_correct(L, rp, f->dU, f->npad, c0, nullptr, cf.hd, n, IT_MAXT, h->pQ.p, rp, s);
    if ((rc = sync_or_fail(s, call, hipGetLastError()))) return rc;
    h->pc_built = true;
    return CUGP_OK;
}

// Z [n][tp] = M^-1 R = (R - Q (Q'R)) / sn2 on the handle's stream (built, achieved rank > 0)
int precond_apply_dev(cugp_iter* h, const double* R, int tp, double* Z)
{
    const PcPlan pl = pc_plan(h->n, h->pc_rank);
    launch_pc_project(h->pQ.p, R, tp, tp, h->n, pl, h->ppart.p, h->stream);
    launch_pc_project_finish(h->ppart.p, pl.blocks, (size_t)pl.rp * tp, h->pT.p, h->stream);
    launch_pc_correct(h->pQ.p, pl.rp, h->pT.p, tp, 0, R, h->dhs, h->n, tp, Z, tp, h->stream);
    return CUGP_OK;
}

// x (h->vx) = K^-1 B for the tp columns of the device block B by tp independent recurrences; the scalars stay in h->hsc
// record: every column's (a_j, b_j) go into h->lrec, max_iter rows (k_iter_record behind each sweep's last scalar kernel; fp64
// mode only); off, the launches are exactly the ones without it
int solve_dev(cugp_iter* h, const CovFn& cf, const double* B, int tp, double tol, int max_iter, int check_every, const char* call,
              bool record = false)
{
    const int n = h->n;
    hipStream_t s = h->stream;
    int rc;
    if ((rc = precond_build(h, call))) return rc;
    const bool pc = h->pc_got > 0;                     // else: the plain recurrence, launch for launch
    for (Scratch* v : {&h->vx, &h->vr, &h->vp, &h->vq})
        if ((rc = v->grow((size_t)n * tp, s))) return rc;
    if (pc && (rc = h->vz.grow((size_t)n * tp, s))) return rc;
    if ((rc = h->dpart.grow((size_t)iter_blocks(n) * IT_MAXT, s))) return rc;
    if (record && ((rc = h->lrec.grow((size_t)2 * max_iter * IT_MAXT, s)) || (rc = h->lmeta.grow((size_t)ML_ROWS * IT_MAXT, s)))) return rc;
    double *x = h->vx.p, *r = h->vr.p, *p = h->vp.p, *q = h->vq.p, *z = h->vz.p, *part = h->dpart.p, *sc = h->dsc;
    // z = M^-1 r and r'z behind it; fresh: the start and a restart (r'z alone), else a sweep (the ratio too)
    auto precondition = [&](int fresh) {
        precond_apply_dev(h, r, tp, z);
        launch_iter_dot(r, z, n, tp, part, s);
        launch_iter_step_z(part, n, tp, fresh, sc, s);
    };
    launch_iter_dot(B, B, n, tp, part, s);
    launch_iter_init(part, n, tp, tol, sc, s);
    launch_iter_start(B, x, r, p, n, tp, s);
    // mixed: the sweeps' product in fp32 and cycle goals, until a verification finds a column stalled (then, and in the
    // fp64 mode from the start, the launches below are the fp64 mode's)
    bool f32 = h->mixed;
    const double rho2 = h->cycle_drop * h->cycle_drop;
    if (f32) launch_iter_goal_init(tp, rho2, sc, s);
    if (pc) {
        precondition(1);
        launch_iter_dir(p, z, n, tp, sc, 0, s);        // (the ratio is 0 from k_iter_init: p = z)
    }
    if (record) launch_iter_record(sc, tp, 1, pc ? SC_RZ : SC_BB, max_iter, h->lrec.p, h->lmeta.p, s);
    // the true residual of the columns that wait for it (final: of the active ones too)
    auto verify = [&](int final) {
        if (const int e = product(h, cf, h->dX, n, x, tp, q, true)) return e;
        h->stats[1]++;
        h->stats[2]++;
        launch_iter_resid(B, q, r, n, tp, sc, final, part, s);
        if (f32) launch_iter_step_v_mx(part, n, tp, final, rho2, sc, s);
        else launch_iter_step_v(part, n, tp, final, sc, s);
        if (!final && pc) precondition(1);
        if (!final) launch_iter_dir(p, pc ? z : r, n, tp, sc, 1, s);
        return (int)CUGP_OK;
    };
    Counts k;
    int it = 0;
    for (;;) {
        if ((rc = read_status(h, tp, call, &k, f32 ? SC_ALLOC : SC_ROWS))) return rc;
        if (f32 && k.stalled) {                        // fp32 cannot refine this K: the rest of the call in fp64,
            f32 = false;                               // the unfinished columns again from x = 0 (k_iter_again)
            h->stats[3] = 1;
            launch_iter_again(B, x, r, n, tp, sc, s);
            if (pc) precondition(1);
            launch_iter_dir(p, pc ? z : r, n, tp, sc, 1, s);
            continue;
        }
        if (k.waiting) {
            if ((rc = verify(0))) return rc;
            continue;
        }
        if (!k.active || it >= max_iter) break;
        const int m = std::min(check_every, max_iter - it);
        for (int j = 0; j < m; j++) {
            if ((rc = product(h, cf, h->dX, n, p, tp, q, true, f32))) return rc;
            h->stats[f32 ? 0 : 1]++;
            launch_iter_dot(p, q, n, tp, part, s);
            if (pc) launch_iter_step_a_pc(part, n, tp, sc, s);
            else launch_iter_step_a(part, n, tp, sc, s);
            launch_iter_update(x, r, p, q, n, tp, sc, part, s);
            if (f32) launch_iter_step_b_mx(part, n, tp, sc, s);
            else launch_iter_step_b(part, n, tp, sc, s);
            if (pc) precondition(0);
            if (record) launch_iter_record(sc, tp, 0, 0, max_iter, h->lrec.p, h->lmeta.p, s);
            launch_iter_dir(p, pc ? z : r, n, tp, sc, 0, s);
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

// alpha = K^-1 y into h->alpha: what cugp_iter_fit runs behind its checks
int fit_run(cugp_iter* h, double tol, int max_iter, int check_every, double* info, const char* call)
{
    int rc;
    h->fit_valid = false;
    if ((rc = h->alpha.grow((size_t)h->n * 16, h->stream))) return rc;
    if ((rc = solve_dev(h, cov_of(h), h->dyb, 16, tol, max_iter, check_every, call))) return rc;
    fill_info(h, 0, 1, info);
    HIPCHK(hipMemcpyAsync(h->alpha.p, h->vx.p, (size_t)h->n * 16 * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->fit_valid = true;
    return CUGP_OK;
}

// The raw sums of one pair of device blocks U, V [n][tp] with cnt live columns: raw[c] for the cov_grad_columns of
// k_cov_grad, raw[nc] = sum_c u_c'v_c (k_iter_dot / k_iter_sum per column, the columns added in ascending order on the
// host).  first: copied, else raw = raw + the block's.  One wait.
int forms_dev(cugp_iter* h, const CovFn& cf, const double* U, const double* V, int cnt, int tp, bool first,
              std::vector<double>& raw, const char* call)
{
    const int n = h->n, nc = cov_grad_columns(cf, h->d);
    const IterPlan pl = iter_apply_plan(n, n, h->split);
    hipStream_t s = h->stream;
    int rc;
    if ((rc = h->gpart.grow((size_t)pl.row_blocks * pl.split * nc, s)) || (rc = h->gout.grow((size_t)nc + IT_MAXT, s)) ||
        (rc = h->ghost.grow((size_t)nc + IT_MAXT, s)) || (rc = h->dpart.grow((size_t)iter_blocks(n) * IT_MAXT, s)))
        return rc;
    launch_cov_grad(h->dX, n, h->d, cf, U, V, tp, h->gpart.p, h->gout.p, pl, s);
    launch_iter_dot(U, V, n, tp, h->dpart.p, s);
    launch_iter_sum(h->dpart.p, n, tp, h->gout.p + nc, s);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(h->ghost.p, h->gout.p, (size_t)(nc + tp) * sizeof(double), hipMemcpyDeviceToHost, s);
    if ((rc = sync_or_fail(s, call, e))) return rc;
    const double* got = h->ghost.p;
    double dot = got[nc];
    for (int c = 1; c < cnt; c++) dot = dot + got[nc + c];
    raw.resize(nc + 1);
    for (int c = 0; c < nc; c++) raw[c] = first ? got[c] : raw[c] + got[c];
    raw[nc] = first ? dot : raw[nc] + dot;
    return CUGP_OK;
}

// out[nh] = sum W o dK/dtheta_h from the raw sums: the length scales (a tied handle: the d columns added in index order, as
// k_finalize_ard_tied does), the shape columns, 2 sum W o Kf, 2 sn2 tr W
void forms_out(const cugp_iter* h, const std::vector<double>& raw, double* out)
{
    const int nc = (int)raw.size() - 1, nl = h->route ? h->d : 1;
    int o = 0;
    if (h->route && !h->ard) {
        double g0 = raw[0];
        for (int c = 1; c < nl; c++) g0 = g0 + raw[c];
        out[o++] = g0;
    } else {
        for (int c = 0; c < nl; c++) out[o++] = raw[c];
    }
    for (int c = nl; c < nc - 1; c++) out[o++] = raw[c];
    out[o++] = 2.0 * raw[nc - 1];
    out[o] = 2.0 * h->hhs->noise_var * raw[nc];
}

// the launch grid's third dimension is the feature chunk of k_cov_grad's per-dimension sums
int grad_dims(const cugp_iter* h, const char* call)
{
    if (h->route && (h->d + 15) / 16 > 65535) return invalid_arg(call, "more than 65535 * 16 input dimensions on the ARD route");
    return CUGP_OK;
}

// the launch grid's third dimension is the feature chunk of k_cov_xgrad's sums, for every family
int xgrad_dims(const cugp_iter* h, const char* call)
{
    if ((h->d + 15) / 16 > 65535) return invalid_arg(call, "more than 65535 * 16 input dimensions");
    return CUGP_OK;
}

// Xt [nt][d] into h->xt, and h->xout grown to `blocks` result blocks of nt * d
int xgrad_inputs(cugp_iter* h, const double* Xt, int nt, int blocks)
{
    int rc;
    if ((rc = h->xt.grow((size_t)nt * h->d, h->stream)) || (rc = h->xout.grow((size_t)blocks * nt * h->d, h->stream))) return rc;
    HIPCHK(hipMemcpyAsync(h->xt.p, Xt, (size_t)nt * h->d * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return CUGP_OK;
}

// One k_cov_xgrad launch with its finish on the handle's stream, for the cnt test rows from row c0 of h->xt.  Wv null: the
// mean form over wm into outm, any cnt; else cnt <= tp rows against the columns of Wv [n][tp] into outv (and wm into outm)
int xgrad_dev(cugp_iter* h, const CovFn& cf, int c0, int cnt, const double* wm, const double* Wv, int tp, double* outm,
              double* outv, double fv)
{
    const IterPlan pl = iter_apply_plan(cnt, h->n, h->split);
    if (const int rc = h->xpart.grow((size_t)pl.split * (Wv ? 2 : 1) * cnt * h->d, h->stream)) return rc;
    launch_cov_xgrad(h->xt.p + (size_t)c0 * h->d, cnt, h->dX, h->n, h->d, cf, wm, Wv, tp, h->xpart.p, outm, outv, fv, pl, h->stream);
    return CUGP_OK;
}

// the device block src [nt][d] -> the caller's array (null: nothing); the stream is waited for
int xgrad_fetch(cugp_iter* h, const double* src, int nt, double* dst)
{
    if (dst) HIPCHK(hipMemcpyAsync(dst, src, (size_t)nt * h->d * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return CUGP_OK;
}

// the refusals the three calls of the pathwise draws share (before any device work)
int features_args(const cugp_iter* h, const char* call, const double* Omega, const double* b, int m, const double* W, int s)
{
    if (!h || !Omega || !b || !W) return invalid_arg(call, "null argument");
    if (s < 1 || s > IT_MAXT) return invalid_arg(call, "s must lie in [1, 64]");
    if (m < 1) return invalid_arg(call, "m must be positive");
    if (m > CUGP_ITER_MAX_N) return invalid_arg(call, "m beyond CUGP_ITER_MAX_N");
    return ready(h, call);
}

// Omega [m][d], b [m], the origin [d] (null: zeros) and W [s][m] as [m][tp] into the handle's feature buffers
int features_stage(cugp_iter* h, const double* Omega, const double* b, int m, const double* W, int s, int tp, const double* origin)
{
    hipStream_t st = h->stream;
    const size_t d = h->d;
    int rc;
    if ((rc = h->fom.grow((size_t)m * d, st)) || (rc = h->fb.grow(m, st)) || (rc = h->forg.grow(d, st))) return rc;
    HIPCHK(hipMemcpyAsync(h->fom.p, Omega, (size_t)m * d * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(h->fb.p, b, (size_t)m * sizeof(double), hipMemcpyHostToDevice, st));
    const std::vector<double> zero(origin ? 0 : d, 0.0);
    HIPCHK(hipMemcpyAsync(h->forg.p, origin ? origin : zero.data(), d * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    return pack(h, W, m, 0, s, tp, h->fw);
}

// h->fout [nq][tp] = Phi(A) W for the staged features on the handle's stream; always fp64
int features_dev(cugp_iter* h, const CovFn& cf, const double* A, int nq, int m, int tp)
{
    const IterPlan pl = rff_apply_plan(nq, m, h->split);
    int rc;
    if ((rc = h->fout.grow((size_t)nq * tp, h->stream))) return rc;
    if (pl.split > 1 && (rc = h->apart.grow((size_t)pl.split * nq * tp, h->stream))) return rc;
    const double amp = std::sqrt(2.0 * h->hhs->signal_var / (double)m);
    launch_rff_apply(A, nq, h->d, cf, h->fom.p, h->fb.p, m, h->forg.p, h->fw.p, tp, amp, h->fout.p, h->apart.p, pl, h->stream);
    return CUGP_OK;
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
    h->ghost.pinned = true;
    h->lhost.pinned = true;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMalloc((void**)&h->dX, (size_t)n * d * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&h->dyb, (size_t)n * 16 * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&h->dhs, hs_bytes(h));
    if (e == hipSuccess) e = hipHostMalloc((void**)&h->hhs, hs_bytes(h), hipHostMallocDefault);
    if (e == hipSuccess) e = hipMalloc((void**)&h->dsc, (size_t)SC_ALLOC * IT_MAXT * sizeof(double));
    if (e == hipSuccess) e = hipHostMalloc((void**)&h->hsc, (size_t)SC_ALLOC * IT_MAXT * sizeof(double), hipHostMallocDefault);
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
    for (Scratch* v : {&h->vb, &h->vx, &h->vr, &h->vp, &h->vq, &h->vk, &h->alpha, &h->apart, &h->dpart, &h->xt, &h->res, &h->pL,
                       &h->pQ, &h->pdres, &h->pshv, &h->pint, &h->ppart, &h->pT, &h->vz, &h->gpart, &h->gout, &h->ghost, &h->xpart, &h->xout,
                       &h->fom, &h->fb, &h->forg, &h->fw, &h->fout, &h->lrec, &h->lmeta, &h->lwork, &h->lquad, &h->lout, &h->lhost, &h->pg1,
                       &h->vcQ, &h->vcR, &h->vcW, &h->vcW2, &h->vcP, &h->vcC, &h->vcpart, &h->vcHc, &h->vcH, &h->vcS, &h->vcsm, &h->vcg})
        v->release();
    if (h->pf) cugp_destroy(h->pf);
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
    h->pc_built = false;
    h->vc_valid = false;
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
    h->pc_built = false;
    h->vc_valid = false;
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

int cugp_iter_set_precond(cugp_iter* h, int rank)
{
    const char* call = "cugp_iter_set_precond";
    if (!h) return invalid_arg(call, "null handle");
    if (rank < 0 || rank > std::min(h->n, CUGP_ITER_MAX_RANK)) return invalid_arg(call, "rank must lie in [0, min(n, CUGP_ITER_MAX_RANK)]");
    h->pc_rank = rank;
    h->pc_built = false;
    return CUGP_OK;
}

int cugp_iter_precond_plan(int n, int rank, int out[4])
{
    const char* call = "cugp_iter_precond_plan";
    if (!out) return invalid_arg(call, "out is NULL");
    if (n < 1 || n > CUGP_ITER_MAX_N) return invalid_arg(call, "n must lie in [1, CUGP_ITER_MAX_N]");
    if (rank < 0 || rank > std::min(n, CUGP_ITER_MAX_RANK)) return invalid_arg(call, "rank must lie in [0, min(n, CUGP_ITER_MAX_RANK)]");
    const PcPlan p = pc_plan(n, rank);
    out[0] = p.rp; out[1] = p.per; out[2] = p.blocks; out[3] = p.per / 4;
    return p.blocks;
}

// the factor for the handle as it stands (a rank of 0 needs neither data nor theta)
static int precond_ready(cugp_iter* h, const char* call)
{
    int rc;
    if (h->pc_rank > 0 && (rc = ready(h, call))) return rc;
    HIPCHK(hipSetDevice(h->device));
    return precond_build(h, call);
}

int cugp_iter_precond_info(cugp_iter* h, int out[4])
{
    const char* call = "cugp_iter_precond_info";
    if (!h || !out) return invalid_arg(call, "null argument");
    if (const int rc = precond_ready(h, call)) return rc;
    out[0] = h->pc_rank; out[1] = h->pc_got; out[2] = h->pc_rp; out[3] = h->pc_built ? 1 : 0;
    return CUGP_OK;
}

int cugp_iter_get_precond(cugp_iter* h, double* L, int* piv)
{
    const char* call = "cugp_iter_get_precond";
    if (!h || !L || !piv) return invalid_arg(call, "null argument");
    if (const int rc = precond_ready(h, call)) return rc;
    const size_t n = h->n, rp = h->pc_rp, got = h->pc_got;
    if (got == 0) return CUGP_OK;
    h->host.resize(n * rp);
    HIPCHK(hipMemcpyAsync(h->host.data(), h->pL.p, n * rp * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (size_t i = 0; i < n; i++)
        for (size_t m = 0; m < got; m++) L[i * got + m] = h->host[i * rp + m];
    for (size_t m = 0; m < got; m++) piv[m] = h->hpiv[m];
    return CUGP_OK;
}

int cugp_iter_precond_apply(cugp_iter* h, const double* V, int t, double* out)
{
    const char* call = "cugp_iter_precond_apply";
    if (!h || !V || !out) return invalid_arg(call, "null argument");
    if (t < 1) return invalid_arg(call, "t must be positive");
    if (h->pc_rank == 0) return invalid_arg(call, "no preconditioner asked for (cugp_iter_set_precond)");
    int rc;
    if ((rc = precond_ready(h, call))) return rc;
    if (h->pc_got == 0) return invalid_arg(call, "the factor ended at rank 0: there is no preconditioner to apply");
    for (int c0 = 0; c0 < t; c0 += IT_MAXT) {
        const int cnt = std::min(IT_MAXT, t - c0), tp = iter_tp(cnt);
        if ((rc = pack(h, V, h->n, c0, cnt, tp, h->vb)) || (rc = h->vz.grow((size_t)h->n * tp, h->stream))) return rc;
        precond_apply_dev(h, h->vb.p, tp, h->vz.p);
        if ((rc = sync_or_fail(h->stream, call, hipGetLastError()))) return rc;
        if ((rc = unpack(h, h->vz.p, h->n, c0, cnt, tp, out))) return rc;
    }
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

int cugp_iter_apply32(cugp_iter* h, const double* V, int t, double* out)
{
    const char* call = "cugp_iter_apply32";
    if (!h || !V || !out) return invalid_arg(call, "null argument");
    if (t < 1) return invalid_arg(call, "t must be positive");
    int rc;
    if ((rc = ready(h, call))) return rc;
    HIPCHK(hipSetDevice(h->device));
    const CovFn cf = cov_of(h);
    for (int c0 = 0; c0 < t; c0 += IT_MAXT) {
        const int cnt = std::min(IT_MAXT, t - c0), tp = iter_tp(cnt);
        if ((rc = pack(h, V, h->n, c0, cnt, tp, h->vb)) || (rc = h->vq.grow((size_t)h->n * tp, h->stream))) return rc;
        if ((rc = product(h, cf, h->dX, h->n, h->vb.p, tp, h->vq.p, true, true))) return rc;
        if ((rc = sync_or_fail(h->stream, call, hipGetLastError()))) return rc;
        if ((rc = unpack(h, h->vq.p, h->n, c0, cnt, tp, out))) return rc;
    }
    return CUGP_OK;
}

int cugp_iter_set_precision(cugp_iter* h, int mode, double cycle_drop)
{
    const char* call = "cugp_iter_set_precision";
    if (mode != CUGP_ITER_FP64 && mode != CUGP_ITER_MIXED) return invalid_arg(call, "mode must be CUGP_ITER_FP64 or CUGP_ITER_MIXED");
    if (!(cycle_drop == 0.0 || (cycle_drop > 0.0 && cycle_drop < 1.0))) return invalid_arg(call, "cycle_drop must lie in (0, 1), or be 0");
    if (!h) return invalid_arg(call, "null handle");
    h->mixed = mode == CUGP_ITER_MIXED;
    h->cycle_drop = cycle_drop == 0.0 ? CUGP_ITER_CYCLE_DROP : cycle_drop;
    return CUGP_OK;
}

int cugp_iter_solve_stats(const cugp_iter* h, int out[4])
{
    if (!h || !out) return invalid_arg("cugp_iter_solve_stats", "null argument");
    std::copy(h->stats, h->stats + 4, out);
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
    std::fill(h->stats, h->stats + 4, 0);
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
    std::fill(h->stats, h->stats + 4, 0);
    return fit_run(h, tol, max_iter, check_every, info, call);
}

int cugp_iter_grad_forms(cugp_iter* h, const double* U, const double* V, int t, double* out)
{
    const char* call = "cugp_iter_grad_forms";
    if (!h || !U || !V || !out) return invalid_arg(call, "null argument");
    if (t < 1) return invalid_arg(call, "t must be positive");
    int rc;
    if ((rc = ready(h, call)) || (rc = grad_dims(h, call))) return rc;
    HIPCHK(hipSetDevice(h->device));
    const CovFn cf = cov_of(h);
    std::vector<double> raw;
    for (int c0 = 0; c0 < t; c0 += IT_MAXT) {
        const int cnt = std::min(IT_MAXT, t - c0), tp = iter_tp(cnt);
        if ((rc = pack(h, U, h->n, c0, cnt, tp, h->vb)) || (rc = pack(h, V, h->n, c0, cnt, tp, h->vk))) return rc;
        if ((rc = forms_dev(h, cf, h->vb.p, h->vk.p, cnt, tp, c0 == 0, raw, call))) return rc;
    }
    forms_out(h, raw, out);
    return CUGP_OK;
}

int cugp_iter_loglik_grad(cugp_iter* h, const double* Z, int t, double tol, int max_iter, int check_every, double* g,
                          double* quad, double* info)
{
    const char* call = "cugp_iter_loglik_grad";
    if (!h || !Z || !g) return invalid_arg(call, "null argument");
    if (t < 1) return invalid_arg(call, "t must be positive");
    int rc;
    if ((rc = solver_args(call, tol, max_iter, check_every)) || (rc = ready(h, call)) || (rc = grad_dims(h, call))) return rc;
    HIPCHK(hipSetDevice(h->device));
    std::fill(h->stats, h->stats + 4, 0);
    if (!h->fit_valid && (rc = fit_run(h, tol, max_iter, check_every, nullptr, call))) return rc;
    const CovFn cf = cov_of(h);
    hipStream_t s = h->stream;
    // the probes: u_p = K^-1 z_p, 64 a solve; both blocks stay on the device for their forms
    std::vector<double> raw, rawa;
    for (int c0 = 0; c0 < t; c0 += IT_MAXT) {
        const int cnt = std::min(IT_MAXT, t - c0), tp = iter_tp(cnt);
        if ((rc = pack(h, Z, h->n, c0, cnt, tp, h->vb))) return rc;
        if ((rc = solve_dev(h, cf, h->vb.p, tp, tol, max_iter, check_every, call))) return rc;
        fill_info(h, c0, cnt, info);
        if ((rc = forms_dev(h, cf, h->vx.p, h->vb.p, cnt, tp, c0 == 0, raw, call))) return rc;
    }
    if ((rc = forms_dev(h, cf, h->alpha.p, h->alpha.p, 1, 16, true, rawa, call))) return rc;
    std::vector<double> fp(h->nh), fa(h->nh);
    forms_out(h, raw, fp.data());
    forms_out(h, rawa, fa.data());
    for (int k = 0; k < h->nh; k++) g[k] = 0.5 * (fp[k] / (double)t - fa[k]);
    if (quad) {
        launch_iter_dot(h->dyb, h->alpha.p, h->n, 16, h->dpart.p, s);
        launch_iter_sum(h->dpart.p, h->n, 16, h->gout.p, s);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(h->ghost.p, h->gout.p, sizeof(double), hipMemcpyDeviceToHost, s);
        if ((rc = sync_or_fail(s, call, e))) return rc;
        *quad = h->ghost.p[0];
    }
    return CUGP_OK;
}

int cugp_iter_loglik(cugp_iter* h, const double* Z, const double* G1, int t, double tol, int max_iter, int check_every, double* ll,
                     double* g, double* quad, double* logdet_precond, double* y_alpha, double* info)
{
    const char* call = "cugp_iter_loglik";
    if (!h || !Z || !ll) return invalid_arg(call, "null argument");
    if (t < 1) return invalid_arg(call, "t must be positive");
    int rc;
    if ((rc = solver_args(call, tol, max_iter, check_every))) return rc;
    if (max_iter > CUGP_ITER_MAX_LOG) return invalid_arg(call, "max_iter beyond CUGP_ITER_MAX_LOG (the recurrence's log)");
    if ((rc = ready(h, call)) || (g && (rc = grad_dims(h, call)))) return rc;
    if (h->mixed) return invalid_arg(call, "refused in the mixed mode: fp32 sweeps and cycle restarts are not one Lanczos process");
    HIPCHK(hipSetDevice(h->device));
    std::fill(h->stats, h->stats + 4, 0);
    if (!h->fit_valid && (rc = fit_run(h, tol, max_iter, check_every, nullptr, call))) return rc;
    if ((rc = precond_build(h, call))) return rc;
    const int n = h->n, r = h->pc_got;
    if (r > 0 && !G1) return invalid_arg(call, "a preconditioned handle needs G1 [t][achieved rank] beside the probes");
    const CovFn cf = cov_of(h);
    hipStream_t s = h->stream;
    if ((rc = h->lquad.grow(t, s)) || (rc = h->lout.grow(3, s)) || (rc = h->lhost.grow((size_t)t + 3, s)) ||
        (rc = h->lwork.grow((size_t)3 * max_iter * IT_MAXT, s)))
        return rc;
    // the probes: z_p (preconditioned L g1 + sn g2), u_p = K^-1 z_p with the recurrence logged, its quadrature, and for the
    // gradient v_p = M^-1 z_p: E[u v'] = K^-1
    std::vector<double> raw, rawa;
    for (int c0 = 0; c0 < t; c0 += IT_MAXT) {
        const int cnt = std::min(IT_MAXT, t - c0), tp = iter_tp(cnt);
        if ((rc = pack(h, Z, n, c0, cnt, tp, h->vb))) return rc;
        const double* B = h->vb.p;
        if (r > 0) {
            if ((rc = pack(h, G1, r, c0, cnt, tp, h->pg1)) || (rc = h->vk.grow((size_t)n * tp, s))) return rc;
            launch_pc_sample(h->pL.p, h->pc_rp, h->pg1.p, r, h->vb.p, h->dhs, n, tp, h->vk.p, s);
            B = h->vk.p;
        }
        if ((rc = solve_dev(h, cf, B, tp, tol, max_iter, check_every, call, true))) return rc;
        fill_info(h, c0, cnt, info);
        launch_slq_quad(h->lrec.p, h->lmeta.p, cnt, max_iter, h->lwork.p, h->lquad.p + c0, s);
        if (g) {
            if (r > 0) precond_apply_dev(h, B, tp, h->vz.p);
            if ((rc = forms_dev(h, cf, h->vx.p, r > 0 ? h->vz.p : B, cnt, tp, c0 == 0, raw, call))) return rc;
        }
    }
    if (g) {
        if ((rc = forms_dev(h, cf, h->alpha.p, h->alpha.p, 1, 16, true, rawa, call))) return rc;
        std::vector<double> fp(h->nh), fa(h->nh);
        forms_out(h, raw, fp.data());
        forms_out(h, rawa, fa.data());
        for (int k = 0; k < h->nh; k++) g[k] = 0.5 * (fp[k] / (double)t - fa[k]);
    }
    // the call's one wait of its own: y'alpha, the probes' mean and the factor's diagonal in one launch, read back with quad
    if ((rc = h->dpart.grow((size_t)iter_blocks(n) * IT_MAXT, s))) return rc;
    launch_iter_dot(h->dyb, h->alpha.p, n, 16, h->dpart.p, s);
    launch_slq_finish(h->dpart.p, n, h->lquad.p, t, r > 0 ? h->pf->dU : nullptr, r > 0 ? h->pf->npad : 0, r, h->lout.p, s);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(h->lhost.p, h->lout.p, 3 * sizeof(double), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipMemcpyAsync(h->lhost.p + 3, h->lquad.p, (size_t)t * sizeof(double), hipMemcpyDeviceToHost, s);
    if ((rc = sync_or_fail(s, call, e))) return rc;
    const double ya = h->lhost.p[0], mean = h->lhost.p[1];
    const double ldm = r > 0 ? (double)(n - r) * std::log(h->hhs->noise_var) + h->lhost.p[2] : 0.0;
    *ll = -0.5 * (ya + (ldm + mean) + (double)n * 1.83787);
    if (quad) std::copy(h->lhost.p + 3, h->lhost.p + 3 + t, quad);
    if (logdet_precond) *logdet_precond = ldm;
    if (y_alpha) *y_alpha = ya;
    return CUGP_OK;
}

int cugp_iter_precond_sample(cugp_iter* h, const double* G1, const double* G2, int t, double* out)
{
    const char* call = "cugp_iter_precond_sample";
    if (!h || !G1 || !G2 || !out) return invalid_arg(call, "null argument");
    if (t < 1) return invalid_arg(call, "t must be positive");
    if (h->pc_rank == 0) return invalid_arg(call, "no preconditioner asked for (cugp_iter_set_precond)");
    int rc;
    if ((rc = precond_ready(h, call))) return rc;
    const int n = h->n, r = h->pc_got;
    if (r == 0) return invalid_arg(call, "the factor ended at rank 0: there is no preconditioner to sample from");
    for (int c0 = 0; c0 < t; c0 += IT_MAXT) {
        const int cnt = std::min(IT_MAXT, t - c0), tp = iter_tp(cnt);
        if ((rc = pack(h, G2, n, c0, cnt, tp, h->vb)) || (rc = pack(h, G1, r, c0, cnt, tp, h->pg1)) ||
            (rc = h->vk.grow((size_t)n * tp, h->stream)))
            return rc;
        launch_pc_sample(h->pL.p, h->pc_rp, h->pg1.p, r, h->vb.p, h->dhs, n, tp, h->vk.p, h->stream);
        if ((rc = sync_or_fail(h->stream, call, hipGetLastError()))) return rc;
        if ((rc = unpack(h, h->vk.p, n, c0, cnt, tp, out))) return rc;
    }
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
    std::fill(h->stats, h->stats + 4, 0);
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

int cugp_iter_input_grad(cugp_iter* h, const double* Xt, int nt, const double* W, int t, double* out)
{
    const char* call = "cugp_iter_input_grad";
    if (!h || !Xt || !W || !out) return invalid_arg(call, "null argument");
    if (nt < 1) return invalid_arg(call, "nt must be positive");
    if (nt > CUGP_ITER_MAX_N) return invalid_arg(call, "nt beyond CUGP_ITER_MAX_N");
    if (t != 1 && t != nt) return invalid_arg(call, "t must be 1 (one weight vector for every test point) or nt (one per test point)");
    int rc;
    if ((rc = ready(h, call)) || (rc = xgrad_dims(h, call))) return rc;
    HIPCHK(hipSetDevice(h->device));
    const CovFn cf = cov_of(h);
    if ((rc = xgrad_inputs(h, Xt, nt, 1))) return rc;
    if (t == 1) {
        if ((rc = pack(h, W, h->n, 0, 1, 16, h->vb)) || (rc = xgrad_dev(h, cf, 0, nt, h->vb.p, nullptr, 16, h->xout.p, nullptr, 0.0)))
            return rc;
    } else {
        // test point c0 + c takes column c of the batch's block: IT_MAXT points a launch, the form's sign by fv = -1
        for (int c0 = 0; c0 < nt; c0 += IT_MAXT) {
            const int cnt = std::min(IT_MAXT, nt - c0), tp = iter_tp(cnt);
            if ((rc = pack(h, W, h->n, c0, cnt, tp, h->vb))) return rc;
            if ((rc = xgrad_dev(h, cf, c0, cnt, nullptr, h->vb.p, tp, nullptr, h->xout.p + (size_t)c0 * h->d, -1.0))) return rc;
        }
    }
    if ((rc = sync_or_fail(h->stream, call, hipGetLastError()))) return rc;
    return xgrad_fetch(h, h->xout.p, nt, out);
}

int cugp_iter_predict_grad(cugp_iter* h, const double* Xt, int nt, int with_noise, double* mean, double* var, double* dmean,
                           double* dvar, double tol, int max_iter, int check_every, double* info)
{
    const char* call = "cugp_iter_predict_grad";
    if (!h || !Xt) return invalid_arg(call, "null argument");
    if (!dmean && !dvar) return invalid_arg(call, "dmean and dvar are both NULL (cugp_iter_predict gives the mean and the variance alone)");
    if (nt < 1) return invalid_arg(call, "nt must be positive");
    if (nt > CUGP_ITER_MAX_N) return invalid_arg(call, "nt beyond CUGP_ITER_MAX_N");
    const bool solve = var || dvar;
    int rc;
    if (solve && (rc = solver_args(call, tol, max_iter, check_every))) return rc;
    if ((rc = ready(h, call)) || (rc = xgrad_dims(h, call))) return rc;
    if (!h->fit_valid) return invalid_arg(call, "no fit for the data and hyper-parameters as they stand (cugp_iter_fit)");
    HIPCHK(hipSetDevice(h->device));
    const CovFn cf = cov_of(h);
    hipStream_t s = h->stream;
    const size_t nd = (size_t)nt * h->d;
    if ((rc = xgrad_inputs(h, Xt, nt, 2))) return rc;
    double *dm = h->xout.p, *dv = h->xout.p + nd;
    if (mean) {                                         // cugp_iter_predict's own launches: its bits
        if ((rc = h->res.grow((size_t)nt * 16, s))) return rc;
        if ((rc = product(h, cf, h->xt.p, nt, h->alpha.p, 16, h->res.p, false))) return rc;
        if ((rc = sync_or_fail(s, call, hipGetLastError()))) return rc;
        if ((rc = unpack(h, h->res.p, nt, 0, 1, 16, mean))) return rc;
    }
    if (!solve) {                                       // the mean's gradient alone: one launch over all nt rows, no solve
        if ((rc = xgrad_dev(h, cf, 0, nt, h->alpha.p, nullptr, 16, dm, nullptr, 0.0))) return rc;
        if ((rc = sync_or_fail(s, call, hipGetLastError()))) return rc;
        return xgrad_fetch(h, dm, nt, dmean);
    }
    std::fill(h->stats, h->stats + 4, 0);
    // cugp_iter_predict's variance loop; the batch's v = K^-1 ks stay in h->vx for the gradients' one launch
    const double prior = h->hhs->signal_var + h->hhs->noise_var;
    double *dsum = h->dsc + (size_t)SC_ROWS * IT_MAXT, *hsum = h->hsc + (size_t)SC_ROWS * IT_MAXT;
    for (int c0 = 0; c0 < nt; c0 += IT_MAXT) {
        const int cnt = std::min(IT_MAXT, nt - c0), tp = iter_tp(cnt);
        if ((rc = h->vk.grow((size_t)h->n * tp, s))) return rc;
        launch_iter_cross_rhs(h->dX, h->n, h->d, h->xt.p + (size_t)c0 * h->d, cnt, tp, cf, h->vk.p, s);
        if ((rc = solve_dev(h, cf, h->vk.p, tp, tol, max_iter, check_every, call))) return rc;
        fill_info(h, c0, cnt, info);
        if (var) {
            launch_iter_dot(h->vk.p, h->vx.p, h->n, tp, h->dpart.p, s);
            launch_iter_sum(h->dpart.p, h->n, tp, dsum, s);
            hipError_t e = hipGetLastError();
            if (e == hipSuccess) e = hipMemcpyAsync(hsum, dsum, (size_t)IT_MAXT * sizeof(double), hipMemcpyDeviceToHost, s);
            if ((rc = sync_or_fail(s, call, e))) return rc;
            for (int c = 0; c < cnt; c++) {
                const double v = prior - hsum[c];
                var[c0 + c] = with_noise ? v : v - h->hhs->noise_var;
            }
        }
        const size_t o = (size_t)c0 * h->d;
        if ((rc = xgrad_dev(h, cf, c0, cnt, h->alpha.p, h->vx.p, tp, dmean ? dm + o : nullptr, dvar ? dv + o : nullptr, 2.0))) return rc;
    }
    if ((rc = sync_or_fail(s, call, hipGetLastError()))) return rc;
    if ((rc = xgrad_fetch(h, dm, nt, dmean))) return rc;
    return xgrad_fetch(h, dv, nt, dvar);
}

int cugp_iter_features_apply(cugp_iter* h, const double* Xq, int nq, const double* Omega, const double* b, int m, const double* W,
                             int s, const double* origin, double* out)
{
    const char* call = "cugp_iter_features_apply";
    int rc;
    if ((rc = features_args(h, call, Omega, b, m, W, s))) return rc;
    if (!out) return invalid_arg(call, "null argument");
    if (nq < 1) return invalid_arg(call, "nq must be positive");
    if (nq > CUGP_ITER_MAX_N) return invalid_arg(call, "nq beyond CUGP_ITER_MAX_N");
    if (!Xq && nq != h->n) return invalid_arg(call, "Xq is NULL (the training rows): nq must be the handle's n");
    HIPCHK(hipSetDevice(h->device));
    const CovFn cf = cov_of(h);
    const int tp = iter_tp(s);
    if ((rc = features_stage(h, Omega, b, m, W, s, tp, origin))) return rc;
    const double* A = h->dX;
    if (Xq) {
        if ((rc = h->xt.grow((size_t)nq * h->d, h->stream))) return rc;
        HIPCHK(hipMemcpyAsync(h->xt.p, Xq, (size_t)nq * h->d * sizeof(double), hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        A = h->xt.p;
    }
    if ((rc = features_dev(h, cf, A, nq, m, tp))) return rc;
    if ((rc = sync_or_fail(h->stream, call, hipGetLastError()))) return rc;
    return unpack(h, h->fout.p, nq, 0, s, tp, out);
}

int cugp_iter_paths_fit(cugp_iter* h, const double* Omega, const double* b, int m, const double* W, const double* Eps, int s,
                        const double* origin, double tol, int max_iter, int check_every, double* V, double* info)
{
    const char* call = "cugp_iter_paths_fit";
    int rc;
    if ((rc = features_args(h, call, Omega, b, m, W, s))) return rc;
    if (!V) return invalid_arg(call, "null argument");
    if ((rc = solver_args(call, tol, max_iter, check_every))) return rc;
    HIPCHK(hipSetDevice(h->device));
    std::fill(h->stats, h->stats + 4, 0);
    const CovFn cf = cov_of(h);
    const int n = h->n, tp = iter_tp(s);
    if ((rc = features_stage(h, Omega, b, m, W, s, tp, origin))) return rc;
    if (Eps && (rc = pack(h, Eps, n, 0, s, tp, h->vk))) return rc;
    if ((rc = h->vb.grow((size_t)n * tp, h->stream)) || (rc = features_dev(h, cf, h->dX, n, m, tp))) return rc;
    launch_iter_paths_rhs(h->dyb, h->fout.p, Eps ? h->vk.p : nullptr, std::exp(h->theta[h->nh - 1]), s, n, tp, h->vb.p, h->stream);
    if ((rc = solve_dev(h, cf, h->vb.p, tp, tol, max_iter, check_every, call))) return rc;
    fill_info(h, 0, s, info);
    return unpack(h, h->vx.p, n, 0, s, tp, V);
}

int cugp_iter_paths_eval(cugp_iter* h, const double* Xt, int nt, const double* Omega, const double* b, int m, const double* W,
                         const double* V, int s, const double* origin, double* out)
{
    const char* call = "cugp_iter_paths_eval";
    int rc;
    if ((rc = features_args(h, call, Omega, b, m, W, s))) return rc;
    if (!Xt || !V || !out) return invalid_arg(call, "null argument");
    if (nt < 1) return invalid_arg(call, "nt must be positive");
    if (nt > CUGP_ITER_MAX_N) return invalid_arg(call, "nt beyond CUGP_ITER_MAX_N");
    HIPCHK(hipSetDevice(h->device));
    const CovFn cf = cov_of(h);
    hipStream_t st = h->stream;
    const int tp = iter_tp(s);
    if ((rc = features_stage(h, Omega, b, m, W, s, tp, origin)) || (rc = pack(h, V, h->n, 0, s, tp, h->vb))) return rc;
    if ((rc = h->xt.grow((size_t)nt * h->d, st)) || (rc = h->res.grow((size_t)nt * tp, st))) return rc;
    HIPCHK(hipMemcpyAsync(h->xt.p, Xt, (size_t)nt * h->d * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    if ((rc = features_dev(h, cf, h->xt.p, nt, m, tp)) || (rc = product(h, cf, h->xt.p, nt, h->vb.p, tp, h->res.p, false))) return rc;
    launch_iter_paths_add(h->fout.p, h->res.p, (size_t)nt * tp, st);
    if ((rc = sync_or_fail(st, call, hipGetLastError()))) return rc;
    return unpack(h, h->res.p, nt, 0, s, tp, out);
}

int cugp_iter_paths_grad(cugp_iter* h, const double* Xt, int nt, const double* Omega, const double* b, int m, const double* W,
                         const double* V, int s, const double* origin, double* out)
{
    const char* call = "cugp_iter_paths_grad";
    if (!W && !V) return invalid_arg(call, "W and V are both NULL (neither term is asked for)");
    if (s < 1 || s > IT_MAXT) return invalid_arg(call, "s must lie in [1, 64]");
    if (nt < 1) return invalid_arg(call, "nt must be positive");
    if (nt > CUGP_ITER_MAX_N) return invalid_arg(call, "nt beyond CUGP_ITER_MAX_N");
    if (!h || !Xt || !out) return invalid_arg(call, "null argument");
    int rc;
    if ((rc = W ? features_args(h, call, Omega, b, m, W, s) : ready(h, call)) || (rc = xgrad_dims(h, call))) return rc;
    HIPCHK(hipSetDevice(h->device));
    const CovFn cf = cov_of(h);
    hipStream_t st = h->stream;
    const int tp = iter_tp(s), d = h->d;
    const IterPlan pd = iter_apply_plan(nt, h->n, h->split), pf = rff_apply_plan(nt, W ? m : 1, h->split);
    if (W && (rc = features_stage(h, Omega, b, m, W, s, tp, origin))) return rc;
    if (V && (rc = pack(h, V, h->n, 0, s, tp, h->vb))) return rc;
    const size_t cnt = (size_t)nt * d * tp;
    if ((rc = h->xt.grow((size_t)nt * d, st)) || (rc = h->xout.grow(cnt, st))) return rc;
    if (V && (rc = h->xpart.grow(pd.split * cnt, st))) return rc;
    if (W && (rc = h->apart.grow(pf.split * cnt, st))) return rc;
    HIPCHK(hipMemcpyAsync(h->xt.p, Xt, (size_t)nt * d * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    const double amp = W ? std::sqrt(2.0 * h->hhs->signal_var / (double)m) : 0.0;
    launch_paths_grad(h->xt.p, nt, d, cf, h->dX, h->n, V ? h->vb.p : nullptr, pd, h->xpart.p, h->fom.p, h->fb.p, m, h->forg.p,
                      W ? h->fw.p : nullptr, amp, pf, h->apart.p, tp, h->xout.p, st);
    if ((rc = sync_or_fail(st, call, hipGetLastError()))) return rc;
    // the device block is [tp][nt][d]: its first s slabs are the caller's array
    HIPCHK(hipMemcpyAsync(out, h->xout.p, (size_t)s * nt * d * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return CUGP_OK;
}

// ---- the variance cache ----

int cugp_iter_varcache_build(cugp_iter* h, const double* B, int tb, int rank, int out[4])
{
    const char* call = "cugp_iter_varcache_build";
    if (!h || !B || !out) return invalid_arg(call, "null argument");
    if (tb < 1 || tb > 16) return invalid_arg(call, "tb must lie in [1, 16]");
    if (rank < 1 || rank > CUGP_ITER_MAX_RANK) return invalid_arg(call, "rank must lie in [1, CUGP_ITER_MAX_RANK]");
    if (rank > h->n) return invalid_arg(call, "rank beyond n");
    int rc;
    if ((rc = ready(h, call))) return rc;
    HIPCHK(hipSetDevice(h->device));
    h->vc_valid = false;
    const CovFn cf = cov_of(h);
    hipStream_t s = h->stream;
    const int n = h->n, bw = tb, nblk = (rank + bw - 1) / bw;
    const PcPlan pl = pc_plan(n, rank);
    const int rp = pl.rp;
    const size_t nb16 = (size_t)n * 16, small = 256 + 16 + 4 + 2;
    if ((rc = h->vcQ.grow((size_t)n * rp, s)) || (rc = h->vcR.grow((size_t)n * rp, s)) || (rc = h->vcW2.grow(nb16, s)) ||
        (rc = h->vcP.grow(nb16, s)) || (rc = h->vcC.grow((size_t)rp * 16, s)) || (rc = h->vcpart.grow((size_t)pl.blocks * rp * 16, s)) ||
        (rc = h->vcHc.grow((size_t)rp * 16, s)) || (rc = h->vcH.grow((size_t)rp * rp, s)) || (rc = h->vcS.grow((size_t)rp * rp, s)) ||
        (rc = h->vcsm.grow(small, s)) || (rc = h->dpart.grow((size_t)iter_blocks(n) * IT_MAXT, s)))
        return rc;
    if ((rc = pack(h, B, n, 0, tb, 16, h->vcW))) return rc;          // the start block: [n][16], zero beyond tb
    double *Q = h->vcQ.p, *W = h->vcW.p, *W2 = h->vcW2.p, *P = h->vcP.p, *C = h->vcC.p, *Hc = h->vcHc.p, *H = h->vcH.p;
    double *Ti = h->vcsm.p, *nrm0 = Ti + 256;
    HyperScalars* unit = (HyperScalars*)(nrm0 + 16);
    int* ctl = (int*)(nrm0 + 16 + 4);
    const HyperScalars one{1.0, 1.0, 1.0};
    HIPCHK(hipMemcpyAsync(unit, &one, sizeof one, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(Q, 0, (size_t)n * rp * sizeof(double), s));
    HIPCHK(hipMemsetAsync(H, 0, (size_t)rp * rp * sizeof(double), s));
    launch_vc_init(ctl, s);
    // C = Q'V over all rp columns (those not yet filled are zeros)
    auto project = [&](const double* V) {
        launch_pc_project(Q, V, 16, 16, n, pl, h->vcpart.p, s);
        launch_pc_project_finish(h->vcpart.p, pl.blocks, (size_t)rp * 16, C, s);
    };
    auto norms = [&](const double* V) {
        launch_iter_dot(V, V, n, 16, h->dpart.p, s);
        launch_iter_sum(h->dpart.p, n, 16, nrm0, s);
    };
    // CholQR twice on the cw columns of src at slot c0: -> P, and Q's slot; the second round records block column c0p of H
    auto orthonormalise = [&](double* src, double* tmp, int c0, int cw, int record, int c0p) {
        launch_vc_place(src, Q, rp, c0, cw, n, s);
        project(src);
        launch_vc_factor(C, c0, cw, 0, 0, nrm0, Ti, Hc, H, rp, c0p, ctl, s);
        launch_vc_scale(src, Ti, tmp, Q, rp, c0, cw, n, s);
        project(tmp);
        launch_vc_factor(C, c0, cw, 1, record, nrm0, Ti, Hc, H, rp, c0p, ctl, s);
        launch_vc_scale(tmp, Ti, P, Q, rp, c0, cw, n, s);
    };
    norms(W);
    orthonormalise(W, W2, 0, std::min(bw, rank), 0, 0);
    const IterPlan ap = iter_apply_plan(n, n, h->split);
    if (ap.split > 1 && (rc = h->apart.grow((size_t)ap.split * n * 16, s))) return rc;
    for (int j = 0; j < nblk; j++) {
        const int c0p = j * bw, c0 = std::min(rank, c0p + bw);       // the block multiplied; where the next one starts
        launch_cov_apply(h->dX, n, h->dX, n, h->d, cf, P, 16, W, h->apart.p, ap, true, s);
        norms(W);
        project(W);
        launch_vc_hacc(C, Hc, rp, 1, ctl, s);
        if (j == nblk - 1) {                                         // the last block column of H: nothing to orthonormalise
            launch_vc_factor(C, c0, 0, 2, 1, nrm0, Ti, Hc, H, rp, c0p, ctl, s);
            break;
        }
        launch_pc_correct(Q, rp, C, 16, 0, W, unit, n, 16, W2, 16, s);
        project(W2);
        launch_vc_hacc(C, Hc, rp, 0, ctl, s);
        launch_pc_correct(Q, rp, C, 16, 0, W2, unit, n, 16, W, 16, s);
        orthonormalise(W, W2, c0, std::min(bw, rank - c0), 1, c0p);
    }
    launch_vc_finish(H, h->vcS.p, Q, h->vcR.p, rp, bw, n, ctl, s);
    int hctl[VC_CTL] = {0, 0, 0, 0};
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(hctl, ctl, sizeof hctl, hipMemcpyDeviceToHost, s);
    if ((rc = sync_or_fail(s, call, e))) return rc;
    h->vc_rank = rank;
    h->vc_got = std::max(0, std::min(hctl[VC_GOT], rank));
    h->vc_rp = rp;
    h->vc_bw = bw;
    h->vc_products = hctl[VC_PRODUCTS];
    h->vc_reason = hctl[VC_REASON];
    h->vc_valid = true;
    out[0] = h->vc_got; out[1] = rp; out[2] = h->vc_products; out[3] = h->vc_reason;
    return CUGP_OK;
}

int cugp_iter_varcache_info(cugp_iter* h, int out[4])
{
    if (!h || !out) return invalid_arg("cugp_iter_varcache_info", "null argument");
    out[0] = h->vc_valid ? h->vc_got : 0;
    out[1] = h->vc_valid ? h->vc_rp : 0;
    out[2] = h->vc_valid ? h->vc_products : 0;
    out[3] = h->vc_valid ? h->vc_reason : 0;
    return CUGP_OK;
}

int cugp_iter_varcache_get(cugp_iter* h, double* Q, double* R, double* H)
{
    const char* call = "cugp_iter_varcache_get";
    if (!h) return invalid_arg(call, "null handle");
    if (!h->vc_valid) return invalid_arg(call, "no cache for the data and hyper-parameters as they stand (cugp_iter_varcache_build)");
    HIPCHK(hipSetDevice(h->device));
    const size_t n = h->n, rp = h->vc_rp, got = h->vc_got;
    if (got == 0) return CUGP_OK;
    for (int which = 0; which < 2; which++) {
        double* dst = which ? R : Q;
        if (!dst) continue;
        h->host.resize(n * rp);
        HIPCHK(hipMemcpyAsync(h->host.data(), which ? h->vcR.p : h->vcQ.p, n * rp * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        for (size_t m = 0; m < got; m++)
            for (size_t i = 0; i < n; i++) dst[m * n + i] = h->host[i * rp + m];
    }
    if (H) {                                            // what was factored: k_vc_hsym's arithmetic on the coefficients
        h->host.resize(rp * rp);
        HIPCHK(hipMemcpyAsync(h->host.data(), h->vcH.p, rp * rp * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        const size_t bw = h->vc_bw;
        for (size_t i = 0; i < got; i++)
            for (size_t j = 0; j < got; j++) {
                const double hij = h->host[i * rp + j], hji = h->host[j * rp + i];
                H[i * got + j] = i / bw == j / bw ? (hij + hji) * 0.5 : i / bw < j / bw ? hij : hji;
            }
    }
    return CUGP_OK;
}

int cugp_iter_predict_cached(cugp_iter* h, const double* Xt, int nt, int with_noise, double* mean, double* var)
{
    const char* call = "cugp_iter_predict_cached";
    if (!h || !Xt || !var) return invalid_arg(call, "null argument");
    if (nt < 1) return invalid_arg(call, "nt must be positive");
    if (nt > CUGP_ITER_MAX_N) return invalid_arg(call, "nt beyond CUGP_ITER_MAX_N");
    if (!h->vc_valid) return invalid_arg(call, "no cache for the data and hyper-parameters as they stand (cugp_iter_varcache_build)");
    if (mean && !h->fit_valid) return invalid_arg(call, "the mean needs a fit for the data and hyper-parameters as they stand (cugp_iter_fit)");
    int rc;
    if ((rc = ready(h, call))) return rc;
    HIPCHK(hipSetDevice(h->device));
    const CovFn cf = cov_of(h);
    hipStream_t s = h->stream;
    if ((rc = h->xt.grow((size_t)nt * h->d, s))) return rc;
    HIPCHK(hipMemcpyAsync(h->xt.p, Xt, (size_t)nt * h->d * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    if (mean) {                                         // cugp_iter_predict's own launches: its bits
        if ((rc = h->res.grow((size_t)nt * 16, s))) return rc;
        if ((rc = product(h, cf, h->xt.p, nt, h->alpha.p, 16, h->res.p, false))) return rc;
        if ((rc = sync_or_fail(s, call, hipGetLastError()))) return rc;
        if ((rc = unpack(h, h->res.p, nt, 0, 1, 16, mean))) return rc;
    }
    const double prior = h->hhs->signal_var + (with_noise ? h->hhs->noise_var : 0.0);
    if (h->vc_got == 0) {                               // an empty basis: the prior, no launch
        std::fill(var, var + nt, prior);
        return CUGP_OK;
    }
    const IterPlan pl = iter_apply_plan(nt, h->n, h->split);
    const int rp = h->vc_rp, nz = (rp + VC_NCT * 16 - 1) / (VC_NCT * 16);
    if ((rc = h->vcg.grow((size_t)(nz + 1) * nt, s))) return rc;
    if (pl.split > 1 && (rc = h->vcpart.grow((size_t)pl.split * nt * rp, s))) return rc;
    double* sq = h->vcg.p + (size_t)nz * nt;
    launch_cov_var(h->xt.p, nt, h->dX, h->n, h->d, cf, h->vcR.p, rp, h->vcpart.p, h->vcg.p, sq, pl, s);
    h->host.resize(nt);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(h->host.data(), sq, (size_t)nt * sizeof(double), hipMemcpyDeviceToHost, s);
    if ((rc = sync_or_fail(s, call, e))) return rc;
    for (int i = 0; i < nt; i++) var[i] = prior - h->host[i];
    return CUGP_OK;
}
