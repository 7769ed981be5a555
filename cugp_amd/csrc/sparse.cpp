// sparse.cpp -- cugp_sparse: sparse variational GP regression on inducing points, a client of the dense handle.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "handle.h"

using namespace cugp;

// ---------------------------------------------------------------- sparse variational GP regression on inducing points
// include/cugp.h and DESIGN.md section 25.  The M x M side is two ordinary handles: `u` over Z with the noise slot holding
// the jitter (its own evaluation: Lu, Lu^-1, Lu^-T) and `b`, a factor handle whose A receives B = I + P / s2 and goes the
// way cugp_potri's does (LB, LB^-1, LB^-T, B^-1).  The N side streams the data in chunks through u's cross-covariance and
// triangular-product launches on u's stream; the new passes are kernels.h's launch_sparse_* / launch_trace_cross.
// One side of the model: a set of p label vectors over the handle's rows -- the handle's own y (p = 1 from creation on), or
// the targets (cugp_sparse_set_targets) -- with everything that depends on them and the results of
// that side's last evaluation.  Both sides share P and the factor handle b, so evaluating one clears the other's `valid`.
struct SparseSide {
    // The route of three steps: the three small solves (true: launch_trmv_lower / _upper on one vector; false: products on
    // the tile over the rows of a matrix), the rank-p term of the weights (true: yv, bv in k_trace_cross's registers;
    // false: k_sparse_weights_targets into G first) and the mean of a prediction (true: k_sparse_predict_finish's; false:
    // launch_targets_mean).  Everything else is one kernel family that the own y runs with p = 1.  The routes stay apart
    // because each is another summation order -- other bits -- for no shared benefit; the flag is the side's, not p == 1's:
    // one target keeps the matrix route and its bits.
    bool vector = false;
    int p = 0, rows = 0;                            // label vectors (0: none set); rows of each of the five vectors: 1, or p rounded up to 128
    size_t ystride = 0;                             // the row stride of y: n rounded up to 128
    double *y = nullptr, *yy = nullptr;             // [p][ystride], zero padded to the chunks' 128-row tiles, and y_t'y_t
    double *vec = nullptr;                          // q, c', gamma', beta', beta' / s2^2: [rows][mpad] each
    double *part = nullptr;                         // the slabs' shares of q: [p][chunk pad / 128][mpad]
    bool valid = false, pd = false;                 // b, c' hold for (data, Z, theta, labels); ... and both matrices were positive definite
    bool row_grad = false, row_z = false;           // the row holds the gradient; gz holds the gradient in Z
    std::vector<double> row, gz;                    // [F, g (nh), F_t (p)] and gZ [m][d]
    double *dout = nullptr, *hout = nullptr;        // results row, device and pinned
    Scratch pred;
    double* v(int k, int mpad) const { return vec + (size_t)k * rows * mpad; }     // vector k of the five
};

// What the local shards of one sharded evaluation share: who the lead is and whether the global M
// side it holds still stands.  Any set_ call on, or the end of, one of the shards clears `valid`.
struct ShardGroup {
    const cugp_sparse* lead = nullptr;
    bool valid = false;
};

struct cugp_sparse {
    int n = 0, m = 0, d = 0, mpad = 0, device = 0, kernel = KERNEL_SE, nh = 3, chunk_rows = 0;
    bool ard = false;
    double jitter = 1e-6;
    cugp_gp *u = nullptr, *b = nullptr;
    double *dX = nullptr;                           // [n][d]
    bool have_data = false, have_z = false;
    std::vector<double> theta;
    SparseSide own, tg;                             // the handle's own y; the targets (cugp_sparse_set_targets)
    // scratch, created on first use
    double *dS = nullptr, *dW = nullptr, *dG = nullptr;      // one chunk: k(X_c, Z), W_c, G_c^T ([chunk pad][mpad])
    double *dP = nullptr, *dscr = nullptr;                   // P and the Gram launch's partial tiles
    double *dM[4] = {nullptr, nullptr, nullptr, nullptr};    // H, H2, a product, R (mpad^2 each): the gradient's
    double *dpart = nullptr;                                 // trace partials: the rectangle's, then the square's
    // the gradient with respect to Z (cugp_sparse_bound_grad_z): created on its first use
    std::vector<double> z;                                   // Z as set, [m][d] (the host copy cugp_sparse_get_inducing returns)
    double *dzpart = nullptr, *dzacc = nullptr, *dzout = nullptr, *hz = nullptr;   // partial blocks, running sums, result, its pinned copy
    // a member of a model whose rows are sharded over ranks (cugp_sparse_create_shard; nshards 0: an ordinary handle)
    int shard = -1, nshards = 0;
    long long rows_total = 0;                                // N of the last sharded evaluation
    std::shared_ptr<ShardGroup> grp;                         // the last sharded evaluation this handle took part in
    double *dglob = nullptr;                                 // the lead's: {y'y, N} and S_uf [nh - 1], summed over the shards
};

namespace {
int sp_chunk_max(const cugp_sparse* s)
{
    const int rows = s->chunk_rows > 0 ? s->chunk_rows : SPARSE_CHUNK_DEFAULT;
    return ((s->n < rows ? s->n : rows) + TILE - 1) / TILE * TILE;
}

size_t sp_blocks_uf(const cugp_sparse* s)
{
    size_t nb = 0;
    const int chunks = sparse_shape(s->n, s->mpad, s->chunk_rows, 0).chunks;
    for (int c = 0; c < chunks; c++) nb += (size_t)(sparse_shape(s->n, s->mpad, s->chunk_rows, c).cpad / 64) * (s->mpad / 64);
    return nb;
}

int sp_ensure(cugp_sparse* s, bool want_grad)
{
    int rc;
    const size_t cm = (size_t)sp_chunk_max(s) * s->mpad, mm = (size_t)s->mpad * s->mpad;
    int split = 1;
    const int chunks = sparse_shape(s->n, s->mpad, s->chunk_rows, 0).chunks;
    for (int c = 0; c < chunks; c++) split = std::max(split, sparse_shape(s->n, s->mpad, s->chunk_rows, c).split);
    if ((rc = ensure(&s->dS, cm)) || (rc = ensure(&s->dW, cm)) || (rc = ensure(&s->dP, mm)) ||
        (rc = ensure(&s->dscr, (size_t)split * mm)))
        return rc;
    if (want_grad) {
        if ((rc = ensure(&s->dG, cm))) return rc;
        for (double*& p : s->dM)
            if ((rc = ensure(&p, mm))) return rc;
        const size_t nb = sp_blocks_uf(s) + (size_t)(s->mpad / 64) * (s->mpad / 64);
        if ((rc = ensure(&s->dpart, (size_t)(s->nh - 1) * nb))) return rc;
    }
    return CUGP_OK;
}

// the buffers of the Z gradient, all or none: a failed allocation leaves the handle as it was
int sp_ensure_z(cugp_sparse* s)
{
    if (s->hz) return CUGP_OK;
    const size_t md = (size_t)s->m * s->d;
    int slots = sparse_z_shape(s->mpad, s->mpad, s->d).ranges;                    // the square's pass
    const int chunks = sparse_shape(s->n, s->mpad, s->chunk_rows, 0).chunks;
    for (int c = 0; c < chunks; c++)
        slots = std::max(slots, sparse_z_shape(sparse_shape(s->n, s->mpad, s->chunk_rows, c).cpad, s->mpad, s->d).ranges);
    double *part = nullptr, *acc = nullptr, *out = nullptr, *h = nullptr;
    hipError_t e = hipMalloc((void**)&part, (size_t)slots * md * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&acc, md * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&out, md * sizeof(double));
    if (e == hipSuccess) e = hipHostMalloc((void**)&h, md * sizeof(double), hipHostMallocDefault);
    if (e != hipSuccess) {
        for (double* p : {part, acc, out})
            if (p) (void)hipFree(p);
        return fail(e == hipErrorOutOfMemory ? CUGP_ERR_NOMEM : CUGP_ERR_DEVICE, "the inducing-input gradient's partial blocks", e);
    }
    s->dzpart = part; s->dzacc = acc; s->dzout = out; s->hz = h;
    return CUGP_OK;
}

// S_c = k(X_c, Z) and W_c = S_c Lu^-T of one chunk on u's stream: the launches of a prediction with the chunk as test rows
void sp_chunk_w(cugp_sparse* s, const CovFn& cf, const SparseShape& c)
{
    cugp_gp* u = s->u;
    launch_kcross(u->dX, s->m, s->d, s->mpad, s->dX + (size_t)c.r0 * s->d, c.count, c.cpad, cf, s->dS, u->stream);
    launch_predict_gemm(s->dS, u->dT, s->dW, s->mpad, c.cpad / TILE, u->nt, u->stream);
}

void sp_side_free(SparseSide& r)
{
    for (double** q : {&r.y, &r.yy, &r.vec, &r.part, &r.dout}) {
        if (*q) (void)hipFree(*q);
        *q = nullptr;
    }
    if (r.hout) (void)hipHostFree(r.hout);
    r.hout = nullptr;
    r.p = r.rows = 0;
    r.valid = false;
}

// a side's buffers for p label vectors, all or none: a failed allocation leaves the side without labels
int sp_side_alloc(cugp_sparse* s, SparseSide& r, int p)
{
    sp_side_free(r);
    const int rows = r.vector ? 1 : (p + TILE - 1) / TILE * TILE;
    const size_t ypad = ((size_t)s->n + TILE - 1) / TILE * TILE, nrow = (size_t)1 + s->nh + p;
    int rc = ensure(&r.y, (size_t)p * ypad);
    if (!rc) rc = ensure(&r.yy, (size_t)p);
    if (!rc) rc = ensure(&r.vec, (size_t)5 * rows * s->mpad);
    if (!rc) rc = ensure(&r.part, (size_t)p * (sp_chunk_max(s) / TILE) * s->mpad);
    if (!rc) rc = ensure(&r.dout, nrow);
    if (!rc && hipHostMalloc((void**)&r.hout, nrow * sizeof(double), hipHostMallocDefault) != hipSuccess)
        rc = fail(CUGP_ERR_NOMEM, "cugp_sparse: the pinned results row");
    if (rc) { sp_side_free(r); return rc; }
    r.p = p;
    r.rows = rows;
    r.ystride = ypad;
    return CUGP_OK;
}

// the checks every evaluating call shares, behind its own argument checks and in front of any device work
int sp_ready(const cugp_sparse* s, const SparseSide& r, const char* call)
{
    if (!s->have_data) return invalid_arg(call, "no data set (cugp_sparse_set_data)");
    if (r.p <= 0) return invalid_arg(call, "no targets set (cugp_sparse_set_targets)");
    if (!s->have_z) return invalid_arg(call, "no inducing inputs set (cugp_sparse_set_inducing)");
    return CUGP_OK;
}

// a shard handle in a call that would evaluate its own rows alone
int sp_shard_refuse(const char* call)
{
    return invalid_arg(call, "the handle is a shard of a sharded model (cugp_sparse_create_shard): its rows alone are another "
                             "model; evaluate with cugp_sparse_sharded_bound_grad");
}

void sp_touch(cugp_sparse* s)                                          // (data, Z or theta of a shard changed)
{
    if (s->grp) s->grp->valid = false;
}

// The bound (and its gradient) of one side at the current hyper-parameters: F = sum_t F_t over the side's p label vectors,
// with the F_t behind the gradient's slots.  The results land in that side's row and gz: NaN where Kuu or B is not
// positive definite (the header's convention).  Two host waits beyond the inner evaluation's: in front of B's
// factorisation, which runs on the factor handle's own stream, and at the end.
// One sequence and one kernel family for both sides; a side's `vector` picks the route of the small solves and of the
// weights' rank-p term (SparseSide).
// want_z (with want_grad): the same sequence with the Z pass behind every k_trace_cross, on the weights that launch read
// -- no launch of the sequence changes, so F and the hyper-parameter components keep their bits -- and no further host wait.
int sp_eval(cugp_sparse* s, SparseSide& r, bool want_grad, const char* call, bool want_z = false)
{
    int rc;
    if (s->nshards > 0) return sp_shard_refuse(call);
    if ((rc = sp_ready(s, r, call))) return rc;
    SparseSide& other = &r == &s->own ? s->tg : s->own;
    if (r.valid && (r.row_grad || !want_grad) && (r.row_z || !want_z)) return CUGP_OK;
    cugp_gp *u = s->u, *b = s->b;
    if (want_z) {
        if ((rc = use_device(u))) return rc;
        if ((rc = sp_ensure_z(s))) return rc;
    }
    const int p = r.p, nrow = 1 + s->nh + p;
    r.valid = r.pd = false;
    other.valid = false;                                               // (b and P are about to be rewritten)
    r.row.assign((size_t)nrow, NAN);
    r.row_grad = want_grad;
    r.row_z = want_z;
    if (want_z) r.gz.assign((size_t)s->m * s->d, NAN);
    std::vector<double> th(s->theta);
    th[s->nh - 1] = 0.5 * std::log(s->jitter);                        // the noise slot of the inner handle: Kuu = k(Z, Z) + eps I
    if ((rc = set_theta(u, th.data()))) return rc;
    if ((rc = cugp_loglik_grad(u, nullptr, nullptr))) return rc;       // Lu, Lu^-1, Lu^-T
    if ((rc = use_device(u))) return rc;
    if ((rc = sp_ensure(s, want_grad))) return rc;
    if (!std::isfinite(u->last_ll)) { r.valid = true; return CUGP_OK; }       // Kuu is not positive definite: NaN results
    if (const int pe = prepare_kernels())
        return fail(CUGP_ERR_DEVICE, "hipFuncSetAttribute(MaxDynamicSharedMemorySize)", (hipError_t)pe);
    hipStream_t st = u->stream;
    const int mp = s->mpad, nl = s->nh - 2;
    const double sf2 = std::exp(s->theta[s->nh - 2] * 2), s2 = std::exp(s->theta[s->nh - 1] * 2);
    double *q = r.v(0, mp), *cp = r.v(1, mp), *gp = r.v(2, mp), *bp = r.v(3, mp), *bsc = r.v(4, mp);
    const int chunks = sparse_shape(s->n, mp, s->chunk_rows, 0).chunks;
    CovFn cf;
    {
        TuneScope ts(u);
        if ((rc = cov_fn(u, st, nullptr, &cf))) return rc;
        for (int c = 0; c < chunks; c++) {
            const SparseShape sh = sparse_shape(s->n, mp, s->chunk_rows, c);
            sp_chunk_w(s, cf, sh);
            launch_sparse_gram(s->dW, mp, sh, s->dP, s->dscr, c == 0, st);
            launch_sparse_wty_targets(s->dW, mp, sh.cpad, r.y + sh.r0, r.ystride, p, r.part, q, c == 0, st);
        }
        launch_sparse_form_b(s->dP, mp, s2, b->dA, st);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(st));
    }
    if ((rc = la_factor_inverse(b, true))) return rc;                  // LB, LB^-1, LB^-T, B^-1 (cugp_potri's route)
    if ((rc = use_device(u))) return rc;
    TuneScope ts(u);
    if (r.vector) launch_trmv_lower(b->dT, mp, mp, q, cp, st);         // c' = LB^-1 q
    else launch_predict_gemm(q, b->dT, cp, mp, r.rows / TILE, b->nt, st);      // C' = Q LB^-T: row t = LB^-1 q_t
    const size_t nb_uf = sp_blocks_uf(s), nb_uu = (size_t)(mp / 64) * (mp / 64);
    double *part_uf = s->dpart, *part_uu = want_grad ? s->dpart + (size_t)(nl + 1) * nb_uf : nullptr;
    if (want_grad) {
        double *H = s->dM[0], *H2 = s->dM[1], *X1 = s->dM[2], *R = s->dM[3];
        if (r.vector) {
            launch_trmv_upper(b->dU, mp, mp, cp, gp, st);              // gamma' = LB^-T c'
            launch_trmv_upper(u->dU, mp, mp, gp, bp, st);              // beta' = Lu^-T gamma'
        } else {
            launch_targets_alpha(cp, b->dU, gp, mp, p, st);            // Gamma' = C' LB^-1: row t = LB^-T c'_t
            launch_targets_alpha(gp, u->dU, bp, mp, p, st);            // Beta' = Gamma' Lu^-1: row t = Lu^-T gamma'_t
        }
        launch_sparse_h_targets(b->dKinv, s->dP, gp, bp, p, s->m, mp, s2, H, H2, bsc, st);
        launch_targets_alpha(H, u->dU, X1, mp, mp, st);                // H Lu^-1
        launch_sparse_transpose(X1, R, mp, 1.0 / s2, st);              // R = Lu^-T H / s2
        launch_targets_alpha(H2, u->dU, X1, mp, mp, st);               // H2 Lu^-1
        launch_sparse_transpose(X1, H, mp, 1.0, st);                   // Lu^-T H2
        launch_targets_alpha(H, u->dU, H2, mp, mp, st);                // 2 G_uu = Lu^-T H2 Lu^-1
        size_t pofs = 0;
        for (int c = 0; c < chunks; c++) {
            const SparseShape sh = sparse_shape(s->n, mp, s->chunk_rows, c);
            if (chunks > 1) sp_chunk_w(s, cf, sh);                     // (one chunk: W is still there)
            launch_sparse_weights(s->dW, R, s->dG, sh.cpad, mp, st);
            if (!r.vector)                                             // (the rank-p part goes into G: the traces get no yv, bv)
                launch_sparse_weights_targets(s->dG, sh.cpad, mp, r.y + sh.r0, r.ystride, bsc, p, sh.count, s->m, st);
            const double *yv = r.vector ? r.y + sh.r0 : nullptr, *bv = r.vector ? bsc : nullptr;
            launch_trace_cross(s->dX + (size_t)sh.r0 * s->d, sh.count, sh.cpad, u->dX, s->m, s->d, mp, cf, s->dG, yv, bv,
                               part_uf, nb_uf, pofs, st);
            if (want_z)
                launch_trace_cross_z(s->dX + (size_t)sh.r0 * s->d, sh.count, sh.cpad, u->dX, s->m, s->d, mp, cf, s->dG, yv, bv,
                                     s->dzpart, s->dzacc, c == 0, false, s->dzout, s->hz, st);
            pofs += (size_t)(sh.cpad / 64) * (mp / 64);
        }
        launch_trace_cross(u->dX, s->m, mp, u->dX, s->m, s->d, mp, cf, H2, nullptr, nullptr, part_uu, nb_uu, 0, st);
        if (want_z) {
            for (size_t i = 0; i < (size_t)s->m * s->d; i++) s->hz[i] = NAN;
            launch_trace_cross_z(u->dX, s->m, mp, u->dX, s->m, s->d, mp, cf, H2, nullptr, nullptr, s->dzpart, s->dzacc, false,
                                 true, s->dzout, s->hz, st);
        }
    }
    for (int i = 0; i < nrow; i++) r.hout[i] = NAN;
    const double* puf = want_grad ? part_uf : nullptr;
    const double ls2 = s->theta[s->nh - 1] * 2;
    const SparseFinalTargets fin{s->dP, b->dKinv, cp, gp, b->dlogdet, r.yy, s->m, mp, b->nt, p, (double)s->n, sf2, s2, ls2};
    launch_sparse_finalize_targets(fin, puf, nb_uf, part_uu, nb_uu, nl, r.dout, r.hout, st);
    if ((rc = sync_or_fail(st, call, hipGetLastError()))) return rc;
    r.pd = std::isfinite(r.hout[0]);
    if (r.pd) {                                                        // (B is not positive definite: NaN results)
        r.row[0] = r.hout[0];
        if (want_grad) std::copy(r.hout + 1, r.hout + 1 + s->nh, r.row.begin() + 1);
        std::copy(r.hout + 1 + s->nh, r.hout + nrow, r.row.begin() + 1 + s->nh);      // the F_t
        if (want_z) std::copy(s->hz, s->hz + (size_t)s->m * s->d, r.gz.begin());
    }
    r.valid = true;
    return CUGP_OK;
}

// The state a prediction reads: an ordinary handle is evaluated where stale (sp_eval); a shard handle is never evaluated
// -- the lead of the last sharded evaluation answers from the global M side it holds while that stands, every other
// shard handle and a stale lead refuse.
int sp_state(cugp_sparse* s, SparseSide& r, const char* call)
{
    if (s->nshards == 0) return sp_eval(s, r, false, call);
    if (&r != &s->own) return sp_shard_refuse(call);
    if (!s->grp || s->grp->lead != s)
        return invalid_arg(call, "the handle is a shard that does not hold the model: predict from the first local shard of "
                                 "cugp_sparse_sharded_bound_grad");
    if (!s->grp->valid || !r.valid)
        return invalid_arg(call, "the sharded model is stale (hyper-parameters, Z or data changed since): evaluate with "
                                 "cugp_sparse_sharded_bound_grad first");
    return CUGP_OK;
}

int sp_set_theta(cugp_sparse* s, const double* th)
{
    bool changed = false;
    for (int i = 0; i < s->nh; i++) changed = changed || th[i] != s->theta[i] || std::isnan(th[i]);
    if (!changed) return CUGP_OK;
    sp_touch(s);
    s->theta.assign(th, th + s->nh);
    s->own.valid = s->tg.valid = false;
    return CUGP_OK;
}

// [F, g, F_t] of a side's last evaluation to wherever the caller wants them
void sp_copy_row(const SparseSide& r, int nh, double* F, double* g, double* F_each)
{
    *F = r.row[0];
    if (g) std::copy(r.row.begin() + 1, r.row.begin() + 1 + nh, g);
    if (F_each) std::copy(r.row.begin() + 1 + nh, r.row.end(), F_each);
}

bool sp_z_moved(const cugp_sparse* s, const double* zv)                // (a NaN counts as moved)
{
    for (size_t i = 0; i < s->z.size(); i++)
        if (zv[i] != s->z[i]) return true;
    return false;
}

struct SpObjective {                                                    // what the two callbacks below are handed
    cugp_sparse* s;
    SparseSide* side;
    const char* call;
};

// f = -F of the side and its gradient at th (NaN where the evaluation fails)
void sp_objective(void* ctx, const double* th, int nh, double* f, double* gr)
{
    const SpObjective* o = (const SpObjective*)ctx;
    SparseSide& r = *o->side;
    const bool ok = sp_set_theta(o->s, th) == CUGP_OK && sp_eval(o->s, r, true, o->call) == CUGP_OK;
    objective_result(ok, ok ? r.row[0] : NAN, r.row.data() + 1, nh, f, gr);
}

// the same at v = [theta, vec Z]; a Z that differs goes to the handle
void sp_objective_z(void* ctx, const double* v, int nv, double* f, double* gr)
{
    const SpObjective* o = (const SpObjective*)ctx;
    cugp_sparse* s = o->s;
    SparseSide& r = *o->side;
    if ((!sp_z_moved(s, v + s->nh) || cugp_sparse_set_inducing(s, v + s->nh) == CUGP_OK) && sp_set_theta(s, v) == CUGP_OK &&
        sp_eval(s, r, true, o->call, true) == CUGP_OK) {
        *f = -1.0 * r.row[0];
        std::copy(r.row.begin() + 1, r.row.begin() + 1 + s->nh, gr);
        std::copy(r.gz.begin(), r.gz.end(), gr + s->nh);
    } else {
        *f = NAN;
        std::fill(gr, gr + nv, NAN);
    }
}

// Conjugate gradients on -F of a side from the current hyper-parameters: cugp_cg_minimize_n's loop over the handle's nh
// entries with the iterates as its record, as cugp_cg_solve_loo keeps it; the end point stays set
int sp_cg_theta(cugp_sparse* s, SpObjective* o, int budget, double* trace, int trace_cap, int* nevals)
{
    std::vector<double> th(s->theta);
    if (const int rc = cg_iterates(sp_objective, o, th.data(), s->nh, budget, trace, trace_cap, nevals)) return rc;
    return sp_set_theta(s, th.data());
}

// the same loop over the nh + m d variables [theta, vec Z]; the record keeps [theta, f] of the iterates
int sp_cg_theta_z(cugp_sparse* s, SpObjective* o, int budget, double* trace, int trace_cap, int* nevals)
{
    int rc, nrows = 0;
    if ((rc = use_device(s->u)) || (rc = sp_ensure_z(s))) return rc;
    const int nv = s->nh + s->m * s->d, cap = trace ? std::max(trace_cap, 0) : 0;
    std::vector<double> v(s->theta), rows((size_t)cap * (nv + 1), NAN);
    v.insert(v.end(), s->z.begin(), s->z.end());
    if ((rc = cg_iterates(sp_objective_z, o, v.data(), nv, budget, cap ? rows.data() : nullptr, cap, nevals, &nrows))) return rc;
    for (int r = 0; r < nrows + (nrows < cap); r++) {                  // (with the NaN row behind the last iterate)
        std::copy(rows.begin() + (size_t)r * (nv + 1), rows.begin() + (size_t)r * (nv + 1) + s->nh, trace + (size_t)r * (s->nh + 1));
        trace[(size_t)r * (s->nh + 1) + s->nh] = rows[(size_t)r * (nv + 1) + nv];
    }
    if (sp_z_moved(s, v.data() + s->nh) && (rc = cugp_sparse_set_inducing(s, v.data() + s->nh))) return rc;
    return sp_set_theta(s, v.data());
}

// the three cg calls: the argument checks, then the driver of the side
int sp_cg(cugp_sparse* s, SparseSide cugp_sparse::*side, bool inducing, const char* call, int budget, double* trace, int trace_cap,
          int* nevals)
{
    if (!s) return invalid_arg(call, "null handle");
    if (budget <= 0) return invalid_arg(call, "budget must be positive");
    if (s->nshards > 0) return sp_shard_refuse(call);
    if (const int rc = sp_ready(s, s->*side, call)) return rc;
    SpObjective o{s, &(s->*side), call};
    return inducing ? sp_cg_theta_z(s, &o, budget, trace, trace_cap, nevals) : sp_cg_theta(s, &o, budget, trace, trace_cap, nevals);
}
}  // namespace

int cugp_sparse_plan(int n, int m, int chunk_rows, int pass, int out[5])
{
    const char* call = "cugp_sparse_plan";
    if (!out) return invalid_arg(call, "out is NULL");
    if (n < 1 || m < 1 || m > CUGP_SPARSE_MAX_M) return invalid_arg(call, "n < 1, m < 1 or m beyond CUGP_SPARSE_MAX_M");
    if (chunk_rows < 0 || chunk_rows % TILE) return invalid_arg(call, "chunk_rows must be 0 or a multiple of 128");
    const SparseShape c = sparse_shape(n, (m + TILE - 1) / TILE * TILE, chunk_rows, pass < 0 ? 0 : pass);
    if (pass < 0 || pass >= c.chunks) return invalid_arg(call, "pass beyond the last one");
    out[0] = c.r0; out[1] = c.count; out[2] = c.cpad; out[3] = c.split; out[4] = c.kstep;
    return c.chunks;
}

// test rows per prediction pass: whole 128-row tiles whose Ks, Wt and Vt ([rows][mpad] each) stay within 1 GiB, at most 2^20
static int sparse_predict_rows(int mpad)
{
    const int rows = (int)std::min<size_t>(((size_t)1 << 30) / ((size_t)3 * mpad * sizeof(double)) / TILE * TILE, (size_t)1 << 20);
    return rows < TILE ? TILE : rows;
}

int cugp_sparse_predict_plan(int m, int nt, int pass, int out[2])
{
    const char* call = "cugp_sparse_predict_plan";
    if (!out) return invalid_arg(call, "out is NULL");
    if (m < 1 || m > CUGP_SPARSE_MAX_M) return invalid_arg(call, "m < 1 or m beyond CUGP_SPARSE_MAX_M");
    if (nt <= 0) return invalid_arg(call, "nt must be positive");
    const int rows = sparse_predict_rows((m + TILE - 1) / TILE * TILE);
    const int passes = (int)(((long long)nt + rows - 1) / rows);
    if (pass < 0 || pass >= passes) return invalid_arg(call, "pass beyond the last one");
    out[0] = pass * rows;                                               // (< nt: no overflow)
    out[1] = nt - out[0] < rows ? nt - out[0] : rows;
    return passes;
}

int cugp_sparse_create(int n, int m, int d, int device, int kernel, int ard, double jitter, int chunk_rows, cugp_sparse** out)
{
    const char* call = "cugp_sparse_create";
    if (!out) return invalid_arg(call, "out is NULL");
    if (n < 1 || d < 1) return invalid_arg(call, "n and d must be positive");
    if (m < 1) return invalid_arg(call, "m < 1: at least one inducing input");
    if (m > CUGP_SPARSE_MAX_M) return invalid_arg(call, "m beyond CUGP_SPARSE_MAX_M");
    if (kernel < 0 || kernel >= KERNEL_COUNT) return invalid_arg(call, "unknown kernel kind");
    if (chunk_rows < 0 || chunk_rows % TILE) return invalid_arg(call, "chunk_rows must be 0 or a multiple of 128");
    if (!(jitter > 0.0) || !std::isfinite(jitter)) return invalid_arg(call, "jitter must be positive and finite");
    int rc;
    if ((rc = need_device(call))) return rc;
    cugp_sparse* s = new (std::nothrow) cugp_sparse;
    if (!s) return fail(CUGP_ERR_NOMEM, "host allocation");
    *out = nullptr;
    s->n = n; s->m = m; s->d = d; s->device = device; s->kernel = kernel; s->ard = ard != 0;
    s->nh = s->ard ? d + 2 : 3;
    s->jitter = jitter; s->chunk_rows = chunk_rows;
    s->mpad = (m + TILE - 1) / TILE * TILE;
    s->theta.assign(s->nh, 0.0);
    s->own.vector = true;
    s->own.row.assign((size_t)2 + s->nh, NAN);
    if ((rc = create_handle(m, d, device, 0, s->ard, &s->u, kernel)) || (rc = cugp_create(m, 1, device, &s->b)) ||
        (rc = ensure_factor_bufs(s->b)) || (rc = ensure_inverse_bufs(s->b))) { cugp_sparse_destroy(s); return rc; }
    if ((rc = sp_side_alloc(s, s->own, 1))) { cugp_sparse_destroy(s); return rc; }
    hipError_t e = hipMalloc((void**)&s->dX, (size_t)n * d * sizeof(double));
    if (e == hipSuccess) e = hipMemset(s->b->dy, 0, (size_t)s->b->npad * sizeof(double));
    if (e != hipSuccess) {
        rc = fail(e == hipErrorOutOfMemory ? CUGP_ERR_NOMEM : CUGP_ERR_DEVICE, call, e);
        cugp_sparse_destroy(s);
        return rc;
    }
    *out = s;
    return CUGP_OK;
}

int cugp_sparse_destroy(cugp_sparse* s)
{
    if (!s) return CUGP_OK;
    sp_touch(s);
    (void)hipSetDevice(s->device);
    if (s->u && s->u->stream) (void)hipStreamSynchronize(s->u->stream);
    if (s->u) (void)cugp_destroy(s->u);
    if (s->b) (void)cugp_destroy(s->b);
    for (double* p : {s->dX, s->dS, s->dW, s->dG, s->dP, s->dscr, s->dM[0], s->dM[1], s->dM[2], s->dM[3], s->dpart, s->dzpart,
                      s->dzacc, s->dzout, s->dglob})
        if (p) (void)hipFree(p);
    for (SparseSide* r : {&s->own, &s->tg}) {
        sp_side_free(*r);
        r->pred.release();
    }
    if (s->hz) (void)hipHostFree(s->hz);
    delete s;
    return CUGP_OK;
}

int cugp_sparse_dims(const cugp_sparse* s, int* n, int* m, int* d, int* mpad, int* chunk_rows)
{
    if (!s) return invalid_arg("cugp_sparse_dims", "null handle");
    if (n) *n = s->n;
    if (m) *m = s->m;
    if (d) *d = s->d;
    if (mpad) *mpad = s->mpad;
    if (chunk_rows) *chunk_rows = s->chunk_rows > 0 ? s->chunk_rows : SPARSE_CHUNK_DEFAULT;
    return CUGP_OK;
}

int cugp_sparse_num_hyper(const cugp_sparse* s, int* nh)
{
    if (!s || !nh) return invalid_arg("cugp_sparse_num_hyper", "null argument");
    *nh = s->nh;
    return CUGP_OK;
}

int cugp_sparse_set_data(cugp_sparse* s, const double* X, const double* y)
{
    const char* call = "cugp_sparse_set_data";
    if (!s || !X || !y) return invalid_arg(call, "null argument");
    int rc;
    if ((rc = use_device(s->u))) return rc;
    hipStream_t st = s->u->stream;
    SparseSide& r = s->own;
    HIPCHK(hipMemcpyAsync(s->dX, X, (size_t)s->n * s->d * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(r.y, 0, r.ystride * sizeof(double), st));
    HIPCHK(hipMemcpyAsync(r.y, y, (size_t)s->n * sizeof(double), hipMemcpyHostToDevice, st));
    launch_sparse_yy_targets(r.y, r.ystride, s->n, 1, r.yy, st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    s->have_data = true;
    sp_touch(s);
    s->own.valid = s->tg.valid = false;
    return CUGP_OK;
}

int cugp_sparse_set_inducing(cugp_sparse* s, const double* Z)
{
    if (!s || !Z) return invalid_arg("cugp_sparse_set_inducing", "null argument");
    const std::vector<double> zero((size_t)s->m, 0.0);                 // (the inner handle's labels are never read by this model)
    if (const int rc = cugp_set_data(s->u, Z, zero.data())) return rc;
    s->z.assign(Z, Z + (size_t)s->m * s->d);
    s->have_z = true;
    sp_touch(s);
    s->own.valid = s->tg.valid = false;
    return CUGP_OK;
}

int cugp_sparse_set_loghyper(cugp_sparse* s, const double* hp, int nh)
{
    const char* call = "cugp_sparse_set_loghyper";
    if (!s || !hp) return invalid_arg(call, "null argument");
    if (nh != s->nh) return invalid_arg(call, "nh is not the handle's (cugp_sparse_num_hyper)");
    return sp_set_theta(s, hp);
}

int cugp_sparse_get_loghyper(const cugp_sparse* s, double* hp, int nh)
{
    const char* call = "cugp_sparse_get_loghyper";
    if (!s || !hp) return invalid_arg(call, "null argument");
    if (nh != s->nh) return invalid_arg(call, "nh is not the handle's (cugp_sparse_num_hyper)");
    std::copy(s->theta.begin(), s->theta.end(), hp);
    return CUGP_OK;
}

int cugp_sparse_bound(cugp_sparse* s, double* F)
{
    const char* call = "cugp_sparse_bound";
    if (!s || !F) return invalid_arg(call, "null argument");
    if (const int rc = sp_eval(s, s->own, false, call)) return rc;
    sp_copy_row(s->own, s->nh, F, nullptr, nullptr);
    return CUGP_OK;
}

int cugp_sparse_bound_grad(cugp_sparse* s, double* F, double* g, int nh)
{
    const char* call = "cugp_sparse_bound_grad";
    if (!s || !F || !g) return invalid_arg(call, "null argument");
    if (nh != s->nh) return invalid_arg(call, "nh is not the handle's (cugp_sparse_num_hyper)");
    if (const int rc = sp_eval(s, s->own, true, call)) return rc;
    sp_copy_row(s->own, s->nh, F, g, nullptr);
    return CUGP_OK;
}

namespace {
// The prediction of one side, behind the call's own argument checks.  Per pass of cugp_sparse_predict_plan Ks, Wt and Vt;
// the variance, which no y enters, by k_sparse_predict_finish.  A vector side's mean comes from that launch too; a matrix
// side's means are (C' / s2) Vt^T (launch_targets_mean), each pass's rows copied to their place in the target-major
// result, and its `var` may be NULL (then the launch is left out).
int sp_predict(cugp_sparse* s, SparseSide& r, const char* call, const double* Xt, int nt, int with_noise, double* mean, double* var)
{
    int rc;
    if ((rc = sp_state(s, r, call))) return rc;                        // (answers from the last evaluation's state when it holds)
    const int p = r.p;
    const bool matrix = !r.vector;
    if (!r.pd) {
        std::fill(mean, mean + (size_t)p * nt, NAN);
        if (var) std::fill(var, var + nt, NAN);
        return CUGP_OK;
    }
    cugp_gp *u = s->u, *b = s->b;
    if ((rc = use_device(u))) return rc;
    TuneScope ts(u);
    hipStream_t st = u->stream;
    const int mp = s->mpad, p64 = (p + 63) / 64 * 64;
    int pr[2];                                                         // the passes of cugp_sparse_predict_plan: the first is the largest
    const int passes = cugp_sparse_predict_plan(s->m, nt, 0, pr);
    if (passes < 1) return passes;
    const int cmax = (pr[1] + TILE - 1) / TILE * TILE;
    const size_t nxt = (((size_t)nt * s->d + 15) / 16) * 16, nks = (size_t)cmax * mp;
    // the matrix route's own: C' / s2, launch_targets_mean's partial sums, a pass's means [p][rows]; its dm is one pass's, unread
    const size_t ncs = matrix ? (size_t)p64 * mp : 0, npp = matrix ? (size_t)targets_mean_split(mp) * p64 * cmax : 0;
    const size_t nm = matrix ? (size_t)p * pr[1] : 0, ndm = matrix ? (size_t)cmax : (size_t)nt;
    if ((rc = r.pred.grow(nxt + 3 * nks + ncs + npp + nm + ndm + nt, st))) return rc;
    double *dXt = r.pred.p, *dKs = dXt + nxt, *dWt = dKs + nks, *dVt = dWt + nks, *dCs = dVt + nks, *dPp = dCs + ncs;
    double *dM = dPp + npp, *dm = dM + nm, *dv = dm + ndm;
    HIPCHK(hipMemcpyAsync(dXt, Xt, (size_t)nt * s->d * sizeof(double), hipMemcpyHostToDevice, st));
    CovFn cf;
    if ((rc = cov_fn(u, st, nullptr, &cf))) return rc;
    const double sf2 = std::exp(s->theta[s->nh - 2] * 2), s2 = std::exp(s->theta[s->nh - 1] * 2);
    const double* cp = r.v(1, mp);                                     // c', or C'
    if (matrix) launch_sparse_scale_targets(cp, p, p64, s->m, mp, s2, dCs, st);
    hipError_t e = hipGetLastError();
    for (int ps = 0; ps < passes && e == hipSuccess; ps++) {
        (void)cugp_sparse_predict_plan(s->m, nt, ps, pr);
        const int t0 = pr[0], c = pr[1], cpad = (c + TILE - 1) / TILE * TILE;
        launch_kcross(u->dX, s->m, s->d, mp, dXt + (size_t)t0 * s->d, c, cpad, cf, dKs, st);
        launch_predict_gemm(dKs, u->dT, dWt, mp, cpad / TILE, u->nt, st);      // Wt = Ks Lu^-T
        launch_predict_gemm(dWt, b->dT, dVt, mp, cpad / TILE, b->nt, st);      // Vt = Wt LB^-T
        if (var) launch_sparse_predict_finish(dWt, dVt, cp, mp, c, sf2, s2, with_noise ? s2 : 0.0, matrix ? dm : dm + t0, dv + t0, st);
        if (matrix) launch_targets_mean(dCs, dVt, dPp, mp, p, c, cpad, dM, st);       // [p][c], packed
        e = hipGetLastError();
        if (e == hipSuccess && matrix)                                         // row t of the pass to mean[t * nt + t0 ..]
            e = hipMemcpy2DAsync(mean + t0, (size_t)nt * sizeof(double), dM, (size_t)c * sizeof(double),
                                 (size_t)c * sizeof(double), p, hipMemcpyDeviceToHost, st);
    }
    if (e == hipSuccess && !matrix) e = hipMemcpyAsync(mean, dm, (size_t)nt * sizeof(double), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && var) e = hipMemcpyAsync(var, dv, (size_t)nt * sizeof(double), hipMemcpyDeviceToHost, st);
    return sync_or_fail(st, call, e);
}
}  // namespace

int cugp_sparse_predict(cugp_sparse* s, const double* Xt, int nt, int with_noise, double* mean, double* var)
{
    const char* call = "cugp_sparse_predict";
    if (!s || !Xt || !mean || !var) return invalid_arg(call, "null argument");
    if (nt <= 0) return invalid_arg(call, "nt must be positive");
    return sp_predict(s, s->own, call, Xt, nt, with_noise, mean, var);
}

// ---- joint covariance, draws and input gradients of the prediction (include/cugp.h)
// The product launch of cugp_sparse_predict_cov at the process's current tuning, and where it refuses: pure arithmetic
int cugp_sparse_predict_cov_plan(int m, int nt, int out[4])
{
    const char* call = "cugp_sparse_predict_cov_plan";
    if (!out) return invalid_arg(call, "out is NULL");
    if (m < 1 || m > CUGP_SPARSE_MAX_M) return invalid_arg(call, "m < 1 or m beyond CUGP_SPARSE_MAX_M");
    if (nt <= 0) return invalid_arg(call, "nt must be positive");
    if (nt > CUGP_SPARSE_MAX_M) return invalid_arg(call, "nt beyond CUGP_SPARSE_MAX_M: the padded nt^2 must fit an int in the factor handle's kernels");
    const int mpad = (m + TILE - 1) / TILE * TILE, ntpad = (nt + TILE - 1) / TILE * TILE;
    if (nt > sparse_predict_rows(mpad))
        return invalid_arg(call, "nt beyond the first pass of cugp_sparse_predict_plan: Wt and Vt must be whole");
    int tn[TUNE_COUNT];                                                // the process defaults: what a handle without keys of its own takes over
    tune_defaults(tn);
    const int* prev = t_tune;
    t_tune = tn;
    const CovShape cs = predict_cov_shape(ntpad, mpad);
    t_tune = prev;
    out[0] = ntpad; out[1] = 32 * cs.wm; out[2] = cs.split; out[3] = cs.kstep;
    return CUGP_OK;
}

namespace {
// The shared half of cugp_sparse_predict_cov and cugp_sparse_predict_sample, behind their argument checks: the own side's
// state (evaluated first when stale), Ks, Wt and Vt of all nt points in ONE pass, the marginal prediction by
// cugp_sparse_predict's launch (the mean's bits), then into the lower tiles of the factor handle of the inner handle u
//   Sigma = k(Xt,Xt) (+ s2 I) + jitter I - (Wt Wt^T - Vt Vt^T)
// by k_sparse_predict_cov (both products on one set of accumulators, split over k as k_predict_cov's) and
// k_predict_cov_finish as it stands.  The inner handle keeps eps in its noise slot -- an ARD handle's scalars are read from
// the device, where that slot cannot be replaced for one launch --, so the finish is told there is no noise and s2 rides in
// its jitter argument: the same single addition to the diagonal, and nothing of eps reaches Sigma.
// *pd false: Kuu or B is not positive definite (nothing was enqueued; the caller writes NaN).
int sp_predict_cov_device(cugp_sparse* s, const char* call, const double* Xt, int nt, bool with_noise, double jitter,
                          double** dmean, cugp_gp** fout, bool* pd)
{
    int rc;
    if ((rc = sp_state(s, s->own, call))) return rc;
    *pd = s->own.pd;
    if (!*pd) return CUGP_OK;
    cugp_gp *u = s->u, *b = s->b;
    if ((rc = use_device(u))) return rc;
    TuneScope ts(u);
    hipStream_t st = u->stream;
    const int mp = s->mpad, tiles = (nt + TILE - 1) / TILE, ntpad = tiles * TILE;
    if ((rc = cov_factor_handle(u, tiles))) return rc;
    if (!u->cov.ev) HIPCHK(hipEventCreateWithFlags(&u->cov.ev, hipEventDisableTiming));
    cugp_gp* f = u->cov.f;
    f->n = nt;                                                         // (a smaller problem in the handle's buffers)
    f->nt = tiles;
    f->npad = ntpad;
    const size_t nxt = (((size_t)nt * s->d + 15) / 16) * 16, nks = (size_t)ntpad * mp;
    if ((rc = s->own.pred.grow(nxt + 3 * nks + 2 * (size_t)ntpad, st))) return rc;
    double *dXt = s->own.pred.p, *dKs = dXt + nxt, *dWt = dKs + nks, *dVt = dWt + nks, *dm = dVt + nks, *dv = dm + ntpad;
    HIPCHK(hipMemcpyAsync(dXt, Xt, (size_t)nt * s->d * sizeof(double), hipMemcpyHostToDevice, st));
    CovFn cf;
    if ((rc = cov_fn(u, st, nullptr, &cf))) return rc;
    const double sf2 = std::exp(s->theta[s->nh - 2] * 2), s2 = std::exp(s->theta[s->nh - 1] * 2);
    launch_kcross(u->dX, s->m, s->d, mp, dXt, nt, ntpad, cf, dKs, st);
    launch_predict_gemm(dKs, u->dT, dWt, mp, tiles, u->nt, st);        // Wt = Ks Lu^-T
    launch_predict_gemm(dWt, b->dT, dVt, mp, tiles, b->nt, st);        // Vt = Wt LB^-T
    launch_sparse_predict_finish(dWt, dVt, s->own.v(1, mp), mp, nt, sf2, s2, with_noise ? s2 : 0.0, dm, dv, st);
    const CovShape cs = predict_cov_shape(ntpad, mp);
    if ((rc = u->cov.scr.grow((size_t)(cs.split - 1) * ntpad * ntpad, st))) return rc;
    launch_sparse_predict_cov(dWt, dVt, mp, ntpad, cs, f->dA, u->cov.scr.p, st);
    cf.h.noise_var = s2;                                               // (by value; unread: with_noise is off, see above)
    launch_predict_cov_finish(dXt, nt, s->d, ntpad, cf, false, with_noise ? s2 + jitter : jitter, f->dA, u->cov.scr.p,
                              cs.split - 1, f->dtickets, st);
    HIPCHK(hipGetLastError());
    *dmean = dm;
    *fout = f;
    return CUGP_OK;
}

// the refusals the covariance and the draws share, in front of any device work: cugp_sparse_predict_cov_plan's
int sp_cov_refuse(const cugp_sparse* s, const char* call, int nt)
{
    if (nt <= 0) return invalid_arg(call, "nt must be positive");
    if (nt > CUGP_SPARSE_MAX_M) return invalid_arg(call, "nt beyond CUGP_SPARSE_MAX_M (cugp_sparse_predict_cov_plan)");
    if (nt > sparse_predict_rows(s->mpad))
        return invalid_arg(call, "nt beyond the first pass of cugp_sparse_predict_plan (cugp_sparse_predict_cov_plan)");
    return sp_ready(s, s->own, call);
}
}  // namespace

int cugp_sparse_predict_cov(cugp_sparse* s, const double* Xt, int nt, int with_noise, double* mean, double* cov)
{
    const char* call = "cugp_sparse_predict_cov";
    if (!s || !Xt || !cov) return invalid_arg(call, "null argument");
    int rc;
    if ((rc = sp_cov_refuse(s, call, nt))) return rc;
    double* dm = nullptr;
    cugp_gp* f = nullptr;
    bool pd = false;
    hipStream_t st = s->u->stream;
    if ((rc = sp_predict_cov_device(s, call, Xt, nt, with_noise != 0, 0.0, &dm, &f, &pd))) { (void)hipStreamSynchronize(st); return rc; }
    if (!pd) {
        if (mean) std::fill(mean, mean + nt, NAN);
        std::fill(cov, cov + (size_t)nt * nt, NAN);
        return CUGP_OK;
    }
    hipError_t e = hipSuccess;
    if (mean) e = hipMemcpyAsync(mean, dm, (size_t)nt * sizeof(double), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess)
        e = hipMemcpy2DAsync(cov, (size_t)nt * sizeof(double), f->dA, (size_t)f->npad * sizeof(double),
                             (size_t)nt * sizeof(double), nt, hipMemcpyDeviceToHost, st);
    if ((rc = sync_or_fail(st, call, e))) return rc;
    // lower triangle, mirrored (cugp_predict_cov's result), in 32 x 32 blocks read along their rows: a column walk over the
    // whole matrix lands on a few cache sets where nt is a multiple of 512 (measured: 530 ms of 535 at nt = 4096)
    constexpr int MB = 32;
    for (int i0 = 0; i0 < nt; i0 += MB)
        for (int j0 = i0; j0 < nt; j0 += MB)
            for (int j = j0; j < j0 + MB && j < nt; j++) {
                const double* lo = cov + (size_t)j * nt;
                for (int i = i0; i < i0 + MB && i < j; i++) cov[(size_t)i * nt + j] = lo[i];
            }
    return CUGP_OK;
}

int cugp_sparse_predict_sample(cugp_sparse* s, const double* Xt, int nt, int with_noise, double jitter, int nsamples,
                               const double* normals, double* samples)
{
    const char* call = "cugp_sparse_predict_sample";
    if (!s || !Xt || !normals || !samples) return invalid_arg(call, "null argument");
    if (nsamples <= 0) return invalid_arg(call, "nsamples must be positive");
    if (!std::isfinite(jitter) || !(jitter >= 0.0)) return invalid_arg(call, "jitter must be finite and not negative");
    int rc;
    if ((rc = sp_cov_refuse(s, call, nt))) return rc;
    double* dm = nullptr;
    cugp_gp* f = nullptr;
    bool pd = false;
    if ((rc = sp_predict_cov_device(s, call, Xt, nt, with_noise != 0, jitter, &dm, &f, &pd))) {
        (void)hipStreamSynchronize(s->u->stream);
        return rc;
    }
    if (!pd) {
        std::fill(samples, samples + (size_t)nsamples * nt, NAN);
        return CUGP_OK;
    }
    return sample_tail(s->u, f, dm, nt, nsamples, normals, samples, call);
}

// Mean, variance and their gradients with respect to the test inputs, in cugp_sparse_predict's passes.  Per pass Ks, Wt, Vt
// and the marginal prediction by cugp_sparse_predict's launches, then -- dvar asked for -- T = Vt LB^-1, D = Wt - T
// (k_sparse_predict_diff, into Vt's place: the prediction has read it) and U = D Lu^-1, both products
// launch_targets_alpha's; then k_predict_grad and its finish, the exact model's instantiations, with (X, n, npad) :=
// (Z, m, mpad), a = beta' / s2 for alpha and U for V.  gamma' and beta' are formed here, by the evaluation's own two
// launches, into this call's scratch whether or not the last evaluation was a gradient one: the same kernels on the same
// inputs give the bits bound_grad's hold, and bound_grad's are not written.
int cugp_sparse_predict_grad(cugp_sparse* s, const double* Xt, int nt, int with_noise, double* mean, double* var, double* dmean,
                             double* dvar)
{
    const char* call = "cugp_sparse_predict_grad";
    if (!s || !Xt) return invalid_arg(call, "null argument");
    if (!dmean && !dvar) return invalid_arg(call, "dmean and dvar are both NULL");
    if (nt <= 0) return invalid_arg(call, "nt must be positive");
    int rc;
    if ((rc = sp_state(s, s->own, call))) return rc;
    const size_t nout = (size_t)nt * s->d;
    if (!s->own.pd) {
        if (mean) std::fill(mean, mean + nt, NAN);
        if (var) std::fill(var, var + nt, NAN);
        if (dmean) std::fill(dmean, dmean + nout, NAN);
        if (dvar) std::fill(dvar, dvar + nout, NAN);
        return CUGP_OK;
    }
    cugp_gp *u = s->u, *b = s->b;
    if ((rc = use_device(u))) return rc;
    TuneScope ts(u);
    hipStream_t st = u->stream;
    const int mp = s->mpad, d = s->d;
    const bool want_var = dvar != nullptr;
    int pr[2];
    const int passes = cugp_sparse_predict_plan(s->m, nt, 0, pr);
    if (passes < 1) return passes;
    const int cmax = (pr[1] + TILE - 1) / TILE * TILE;
    const size_t nxt = (((size_t)nt * d + 15) / 16) * 16, nks = (size_t)cmax * mp, pstride = (size_t)pr[1] * d;
    const size_t npart = (size_t)predict_grad_tiles(s->m) * 2 * pstride;
    if ((rc = s->own.pred.grow(nxt + (want_var ? 4 : 3) * nks + npart + 3 * (size_t)mp + 2 * (size_t)nt + 2 * nout, st))) return rc;
    double *dXt = s->own.pred.p, *dKs = dXt + nxt, *dWt = dKs + nks, *dVt = dWt + nks, *dT = dVt + nks;
    double *dP = dT + (want_var ? nks : 0), *dgam = dP + npart, *dbet = dgam + mp, *da = dbet + mp;
    double *dm = da + mp, *dv = dm + nt, *dgm = dv + nt, *dgv = dgm + nout;
    HIPCHK(hipMemcpyAsync(dXt, Xt, (size_t)nt * d * sizeof(double), hipMemcpyHostToDevice, st));
    CovFn cf;
    if ((rc = cov_fn(u, st, nullptr, &cf))) return rc;
    const double sf2 = std::exp(s->theta[s->nh - 2] * 2), s2 = std::exp(s->theta[s->nh - 1] * 2);
    const double* cp = s->own.v(1, mp);                                   // c'
    launch_trmv_upper(b->dU, mp, mp, cp, dgam, st);                    // gamma' = LB^-T c'
    launch_trmv_upper(u->dU, mp, mp, dgam, dbet, st);                  // beta' = Lu^-T gamma'
    hipError_t e = hipGetLastError();
    for (int ps = 0; ps < passes && e == hipSuccess; ps++) {
        (void)cugp_sparse_predict_plan(s->m, nt, ps, pr);
        const int t0 = pr[0], c = pr[1], cpad = (c + TILE - 1) / TILE * TILE;
        const double* xt = dXt + (size_t)t0 * d;
        launch_kcross(u->dX, s->m, d, mp, xt, c, cpad, cf, dKs, st);
        launch_predict_gemm(dKs, u->dT, dWt, mp, cpad / TILE, u->nt, st);      // Wt = Ks Lu^-T
        launch_predict_gemm(dWt, b->dT, dVt, mp, cpad / TILE, b->nt, st);      // Vt = Wt LB^-T
        launch_sparse_predict_finish(dWt, dVt, cp, mp, c, sf2, s2, with_noise ? s2 : 0.0, dm + t0, dv + t0, st);
        if (want_var) launch_targets_alpha(dVt, b->dU, dT, mp, cpad, st);      // T = Vt LB^-1
        if (want_var || ps == 0)                                               // D = Wt - T over Vt; a = beta' / s2 once
            launch_sparse_predict_diff(dWt, dT, want_var ? dVt : nullptr, mp, cpad, dbet, s2, s->m, ps == 0 ? da : nullptr, st);
        if (want_var) launch_targets_alpha(dVt, u->dU, dT, mp, cpad, st);      // U = D Lu^-1
        launch_predict_grad(u->dX, s->m, d, mp, xt, c, cf, dKs, want_var ? dT : nullptr, da, dP, pstride, st);
        launch_predict_grad_finish(dP, pstride, s->m, c, d, cf, dgm + (size_t)t0 * d, want_var ? dgv + (size_t)t0 * d : nullptr, st);
        e = hipGetLastError();
    }
    if (e == hipSuccess && mean) e = hipMemcpyAsync(mean, dm, (size_t)nt * sizeof(double), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && var) e = hipMemcpyAsync(var, dv, (size_t)nt * sizeof(double), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && dmean) e = hipMemcpyAsync(dmean, dgm, nout * sizeof(double), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && dvar) e = hipMemcpyAsync(dvar, dgv, nout * sizeof(double), hipMemcpyDeviceToHost, st);
    return sync_or_fail(st, call, e);
}

int cugp_sparse_cg_solve(cugp_sparse* s, int budget, double* trace, int trace_cap, int* nevals)
{
    return sp_cg(s, &cugp_sparse::own, false, "cugp_sparse_cg_solve", budget, trace, trace_cap, nevals);
}

// ---- the inducing inputs as variables
int cugp_sparse_get_inducing(const cugp_sparse* s, double* Z)
{
    const char* call = "cugp_sparse_get_inducing";
    if (!s || !Z) return invalid_arg(call, "null argument");
    if (!s->have_z) return invalid_arg(call, "no inducing inputs set (cugp_sparse_set_inducing)");
    std::copy(s->z.begin(), s->z.end(), Z);
    return CUGP_OK;
}

int cugp_sparse_bound_grad_z(cugp_sparse* s, double* F, double* g, int nh, double* gZ)
{
    const char* call = "cugp_sparse_bound_grad_z";
    if (!s || !F || !g || !gZ) return invalid_arg(call, "null argument");
    if (nh != s->nh) return invalid_arg(call, "nh is not the handle's (cugp_sparse_num_hyper)");
    if (const int rc = sp_eval(s, s->own, true, call, true)) return rc;
    sp_copy_row(s->own, s->nh, F, g, nullptr);
    std::copy(s->own.gz.begin(), s->own.gz.end(), gZ);
    return CUGP_OK;
}

int cugp_sparse_cg_solve_z(cugp_sparse* s, int budget, double* trace, int trace_cap, int* nevals)
{
    return sp_cg(s, &cugp_sparse::own, true, "cugp_sparse_cg_solve_z", budget, trace, trace_cap, nevals);
}

// ---- p targets over one set of inducing points (include/cugp.h)
// The calls below are the single-target ones with sp_eval, sp_predict and sp_cg asked for the targets' side; what is
// theirs alone is the targets' data.  Either side's evaluation writes the shared factor handle b and P, so it takes the
// other side's validity.
int cugp_sparse_set_targets(cugp_sparse* s, const double* Y, int p)
{
    const char* call = "cugp_sparse_set_targets";
    if (!s || !Y) return invalid_arg(call, "null argument");
    if (p < 1) return invalid_arg(call, "p must be positive");
    if (s->nshards > 0) return sp_shard_refuse(call);
    if (!s->have_data) return invalid_arg(call, "no data set (cugp_sparse_set_data comes first: it supplies X)");
    int rc;
    if ((rc = use_device(s->u))) return rc;
    hipStream_t st = s->u->stream;
    HIPCHK(hipStreamSynchronize(st));
    SparseSide& r = s->tg;
    r.valid = false;
    if (p != r.p && (rc = sp_side_alloc(s, r, p))) return rc;          // (all or none: the handle is left without targets)
    HIPCHK(hipMemsetAsync(r.y, 0, (size_t)p * r.ystride * sizeof(double), st));
    HIPCHK(hipMemsetAsync(r.vec, 0, (size_t)5 * r.rows * s->mpad * sizeof(double), st));
    HIPCHK(hipMemcpy2DAsync(r.y, r.ystride * sizeof(double), Y, (size_t)s->n * sizeof(double), (size_t)s->n * sizeof(double), p,
                            hipMemcpyHostToDevice, st));
    launch_sparse_yy_targets(r.y, r.ystride, s->n, p, r.yy, st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    return CUGP_OK;
}

int cugp_sparse_num_targets(const cugp_sparse* s, int* p)
{
    if (!s || !p) return invalid_arg("cugp_sparse_num_targets", "null argument");
    *p = s->tg.p;
    return CUGP_OK;
}

int cugp_sparse_bound_targets(cugp_sparse* s, double* F, double* F_each)
{
    const char* call = "cugp_sparse_bound_targets";
    if (!s || !F) return invalid_arg(call, "null argument");
    if (const int rc = sp_eval(s, s->tg, false, call)) return rc;
    sp_copy_row(s->tg, s->nh, F, nullptr, F_each);
    return CUGP_OK;
}

int cugp_sparse_bound_grad_targets(cugp_sparse* s, double* F, double* g, int nh, double* F_each)
{
    const char* call = "cugp_sparse_bound_grad_targets";
    if (!s || !F || !g) return invalid_arg(call, "null argument");
    if (nh != s->nh) return invalid_arg(call, "nh is not the handle's (cugp_sparse_num_hyper)");
    if (const int rc = sp_eval(s, s->tg, true, call)) return rc;
    sp_copy_row(s->tg, s->nh, F, g, F_each);
    return CUGP_OK;
}

int cugp_sparse_bound_grad_z_targets(cugp_sparse* s, double* F, double* g, int nh, double* gZ, double* F_each)
{
    const char* call = "cugp_sparse_bound_grad_z_targets";
    if (!s || !F || !g || !gZ) return invalid_arg(call, "null argument");
    if (nh != s->nh) return invalid_arg(call, "nh is not the handle's (cugp_sparse_num_hyper)");
    if (const int rc = sp_eval(s, s->tg, true, call, true)) return rc;
    sp_copy_row(s->tg, s->nh, F, g, F_each);
    std::copy(s->tg.gz.begin(), s->tg.gz.end(), gZ);
    return CUGP_OK;
}

// means of every target [p][nt] and (var given) the variance, which no target enters
int cugp_sparse_predict_targets(cugp_sparse* s, const double* Xt, int nt, int with_noise, double* mean, double* var)
{
    const char* call = "cugp_sparse_predict_targets";
    if (!s || !Xt || !mean) return invalid_arg(call, "null argument");
    if (nt <= 0) return invalid_arg(call, "nt must be positive");
    return sp_predict(s, s->tg, call, Xt, nt, with_noise, mean, var);
}

// cugp_sparse_cg_solve (inducing 0) or cugp_sparse_cg_solve_z (otherwise) on -sum_t F_t: the same loop, record and end point
int cugp_sparse_cg_solve_targets(cugp_sparse* s, int budget, int inducing, double* trace, int trace_cap, int* nevals)
{
    return sp_cg(s, &cugp_sparse::tg, inducing != 0, "cugp_sparse_cg_solve_targets", budget, trace, trace_cap, nevals);
}

// ---- the data rows sharded over ranks (include/cugp.h)
// A shard handle is an ordinary one that knows its place; what it adds is in the phases below, which are sp_eval cut at the
// two points where the shards meet.  The public evaluating calls and both exchanges are comm.cpp's.
int cugp_sparse_create_shard(int n_local, int m, int d, int device, int kernel, int ard, double jitter, int chunk_rows, int shard,
                             int nshards, cugp_sparse** out)
{
    const char* call = "cugp_sparse_create_shard";
    if (!out) return invalid_arg(call, "out is NULL");
    if (nshards < 1 || shard < 0 || shard >= nshards) return invalid_arg(call, "nshards < 1 or shard outside [0, nshards)");
    int rc;
    if ((rc = cugp_sparse_create(n_local, m, d, device, kernel, ard, jitter, chunk_rows, out))) return rc;
    cugp_sparse* s = *out;
    if ((rc = ensure(&s->dglob, (size_t)2 + s->nh))) {
        cugp_sparse_destroy(s);
        *out = nullptr;
        return rc;
    }
    s->shard = shard;
    s->nshards = nshards;
    return CUGP_OK;
}

int cugp_sparse_shard_info(const cugp_sparse* s, int* shard, int* nshards, long long* rows_total)
{
    if (!s) return invalid_arg("cugp_sparse_shard_info", "null handle");
    if (shard) *shard = s->shard;
    if (nshards) *nshards = s->nshards;
    if (rows_total) *rows_total = s->rows_total;
    return CUGP_OK;
}

namespace {
uint64_t fnv1a(uint64_t h, const void* p, size_t bytes)
{
    const unsigned char* b = (const unsigned char*)p;
    for (size_t i = 0; i < bytes; i++) h = (h ^ b[i]) * 1099511628211ull;
    return h;
}

void halves(uint64_t v, double* out)                                   // two doubles that are exact integers below 2^32
{
    out[0] = (double)(v >> 32);
    out[1] = (double)(v & 0xffffffffull);
}

// the header's fields behind {status, local shard count}, for the error texts
const char* const SHARD_FIELD[SHARD_HDR] = {"status", "shard count", "m", "d", "the kernel", "ard", "nh", "nshards", "per", "what",
                                            "the jitter", "the jitter", "the hyper-parameters or Z", "the hyper-parameters or Z",
                                            "rows", ""};

// S_c and W_c of a chunk of shard s against the lead's inner handle (sp_chunk_w with the M side of another handle)
void shard_chunk_w(cugp_sparse* lead, cugp_sparse* s, const CovFn& cf, const SparseShape& c)
{
    cugp_gp* u = lead->u;
    launch_kcross(u->dX, s->m, s->d, s->mpad, s->dX + (size_t)c.r0 * s->d, c.count, c.cpad, cf, s->dS, u->stream);
    launch_predict_gemm(s->dS, u->dT, s->dW, s->mpad, c.cpad / TILE, u->nt, u->stream);
}

int shard_stats_enqueue(ShardEval& e, double* send)
{
    int rc;
    cugp_sparse* L = e.sh[0];
    cugp_gp* u = L->u;
    const bool want_grad = e.what >= 1, want_z = e.what == 2;
    auto grp = std::make_shared<ShardGroup>();
    grp->lead = L;
    for (int i = 0; i < e.nlocal; i++) {
        cugp_sparse* s = e.sh[i];
        sp_touch(s);
        s->grp = grp;
        s->own.valid = s->tg.valid = s->own.pd = false;
    }
    SparseSide& r = L->own;
    r.row.assign((size_t)2 + L->nh, NAN);
    r.row_grad = want_grad;
    r.row_z = want_z;
    if (want_z) r.gz.assign((size_t)L->m * L->d, NAN);
    if ((rc = use_device(u))) return rc;
    for (int i = 0; i < e.nlocal; i++) {                               // every buffer of the evaluation, in front of exchange 1
        if ((rc = sp_ensure(e.sh[i], want_grad))) return rc;
        if (want_z && (rc = sp_ensure_z(e.sh[i]))) return rc;
    }
    std::vector<double> th(L->theta);
    th[L->nh - 1] = 0.5 * std::log(L->jitter);
    if ((rc = set_theta(u, th.data()))) return rc;
    if ((rc = cugp_loglik_grad(u, nullptr, nullptr))) return rc;       // Lu, Lu^-1, Lu^-T: the same on every rank
    if ((rc = use_device(u))) return rc;
    e.kuu_pd = std::isfinite(u->last_ll);
    if (!e.kuu_pd) return CUGP_OK;                                     // (every rank alike: NaN results behind exchange 1)
    if (const int pe = prepare_kernels())
        return fail(CUGP_ERR_DEVICE, "hipFuncSetAttribute(MaxDynamicSharedMemorySize)", (hipError_t)pe);
    hipStream_t st = e.stream;
    const int mp = e.mpad;
    TuneScope ts(u);
    if ((rc = cov_fn(u, st, nullptr, &e.cf))) return rc;
    for (int i = 0; i < e.nlocal; i++) {
        cugp_sparse* s = e.sh[i];
        double *P = send + SHARD_HDR + (size_t)i * e.slot1, *q = P + (size_t)mp * mp;
        const int chunks = sparse_shape(s->n, mp, s->chunk_rows, 0).chunks;
        for (int c = 0; c < chunks; c++) {
            const SparseShape sh = sparse_shape(s->n, mp, s->chunk_rows, c);
            shard_chunk_w(L, s, e.cf, sh);
            launch_sparse_gram(s->dW, mp, sh, P, s->dscr, c == 0, st);
            launch_sparse_wty_targets(s->dW, mp, sh.cpad, s->own.y + sh.r0, s->own.ystride, 1, s->own.part, q, c == 0, st);
        }
        HIPCHK(hipMemcpyAsync(q + mp, s->own.yy, sizeof(double), hipMemcpyDeviceToDevice, st));
        HIPCHK(hipMemcpyAsync(q + mp + 1, e.hsend + SHARD_HDR + i, sizeof(double), hipMemcpyHostToDevice, st));
    }
    HIPCHK(hipGetLastError());
    return CUGP_OK;
}
}  // namespace

namespace cugp {

int sp_shard_begin(ShardEval& e)
{
    const char* call = e.call;
    cugp_sparse* L = e.sh[0];
    if (!L) return invalid_arg(call, "the first shard handle is NULL");
    if (L->nshards == 0)
        return invalid_arg(call, "the first handle is an ordinary one (cugp_sparse_create): a sharded model takes the handles "
                                 "of cugp_sparse_create_shard");
    if (L->device != e.device) return invalid_arg(call, "the first shard is on another device than the communicator");
    e.m = L->m; e.d = L->d; e.mpad = L->mpad; e.nh = L->nh;
    e.slot1 = (size_t)L->mpad * L->mpad + L->mpad + 2;
    e.slot2 = e.what >= 1 ? (size_t)(L->nh - 1) + (e.what == 2 ? (size_t)L->m * L->d : 0) : 0;
    e.stream = L->u->stream;
    char buf[256];
    const int expect = (e.nshards - e.rank + e.world - 1) / e.world;
    int st = CUGP_OK;
    if (e.nlocal != expect || e.nlocal > e.per) {
        snprintf(buf, sizeof buf, "rank %d holds %d shards, %d of %d expected (per = %d)", e.rank, e.nlocal, expect, e.nshards, e.per);
        st = invalid_arg(call, buf);
    }
    for (int i = 0; i < e.nlocal && st == CUGP_OK; i++) {
        const cugp_sparse* s = e.sh[i];
        const char* why = nullptr;
        if (!s) why = "a shard handle is NULL";
        else if (s->nshards == 0) why = "an ordinary handle (cugp_sparse_create) in the list of shards";
        else if (s->nshards != e.nshards || s->shard != e.rank + i * e.world)
            why = "a handle's shard index or count is not its place in the list (slot i holds shard rank + i * world)";
        else if (s->device != e.device) why = "a shard on another device than the communicator";
        else if (s->m != L->m || s->d != L->d || s->kernel != L->kernel || s->ard != L->ard ||
                 memcmp(&s->jitter, &L->jitter, sizeof(double)))
            why = "the local shards disagree in m, d, kernel, ard or jitter";
        else if (!s->have_data) why = "a shard without data (cugp_sparse_set_data)";
        else if (!s->have_z) why = "a shard without inducing inputs (cugp_sparse_set_inducing)";
        else if (memcmp(s->theta.data(), L->theta.data(), (size_t)L->nh * sizeof(double)))
            why = "the local shards disagree in the bits of the hyper-parameters";
        else if (memcmp(s->z.data(), L->z.data(), L->z.size() * sizeof(double)))
            why = "the local shards disagree in the bits of Z";
        if (why) st = invalid_arg(call, why);
    }
    e.status = st;
    return CUGP_OK;
}

void sp_shard_stats(ShardEval& e, double* send)
{
    cugp_sparse* L = e.sh[0];
    double* h = e.hsend;
    double rows = 0.0;
    for (int i = 0; i < e.nlocal && e.status == CUGP_OK; i++) {
        h[SHARD_HDR + i] = (double)e.sh[i]->n;
        rows = rows + (double)e.sh[i]->n;
    }
    if (e.status == CUGP_OK) e.status = shard_stats_enqueue(e, send);
    if (e.status != CUGP_OK)                                           // all-ones slots: NaN wherever they are added
        (void)hipMemsetAsync(send + SHARD_HDR, 0xff, (size_t)e.per * e.slot1 * sizeof(double), e.stream);
    std::fill(h, h + SHARD_HDR, 0.0);
    h[0] = (double)e.status; h[1] = (double)e.nlocal; h[2] = L->m; h[3] = L->d; h[4] = L->kernel; h[5] = L->ard ? 1.0 : 0.0;
    h[6] = L->nh; h[7] = e.nshards; h[8] = e.per; h[9] = e.what;
    uint64_t jb;
    memcpy(&jb, &L->jitter, sizeof jb);
    halves(jb, h + 10);
    uint64_t fp = fnv1a(14695981039346656037ull, L->theta.data(), L->theta.size() * sizeof(double));
    halves(fnv1a(fp, L->z.data(), L->z.size() * sizeof(double)), h + 12);
    h[14] = rows;
    const hipError_t err = hipMemcpyAsync(send, h, SHARD_HDR * sizeof(double), hipMemcpyHostToDevice, e.stream);
    if (err != hipSuccess && e.status == CUGP_OK) e.status = fail(CUGP_ERR_DEVICE, "hipMemcpyAsync (the shard header)", err);
}

int sp_shard_solve(ShardEval& e, const double* g, size_t rstride)
{
    cugp_sparse* L = e.sh[0];
    cugp_gp *u = L->u, *b = L->b;
    hipStream_t st = e.stream;
    SparseSide& r = L->own;
    const int mp = e.mpad;
    const size_t mm = (size_t)mp * mp;
    double *q = r.v(0, mp), *cp = r.v(1, mp);
    const double s2 = std::exp(L->theta[L->nh - 1] * 2);
    int rc;
    if ((rc = use_device(u))) return rc;
    {
        TuneScope ts(u);
        if (e.status == CUGP_OK && e.kuu_pd) {                         // (else: nothing of this rank's is read again)
            launch_sparse_shard_reduce(g, rstride, SHARD_HDR, e.slot1, 0, mm, e.world, e.nshards, L->dP, st);
            launch_sparse_shard_reduce(g, rstride, SHARD_HDR, e.slot1, mm, (size_t)mp, e.world, e.nshards, q, st);
            launch_sparse_shard_reduce(g, rstride, SHARD_HDR, e.slot1, mm + mp, 2, e.world, e.nshards, L->dglob, st);
            launch_sparse_form_b(L->dP, mp, s2, b->dA, st);
        }
        HIPCHK(hipMemcpy2DAsync(e.hall, SHARD_HDR * sizeof(double), g, rstride * sizeof(double), SHARD_HDR * sizeof(double),
                                (size_t)e.world, hipMemcpyDeviceToHost, st));
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(st));
    }
    // ---- every rank reads every rank's header: the same verdict everywhere
    char buf[640];
    double total = 0.0, rows = 0.0;
    for (int k = 0; k < e.world; k++) {
        const double* h = e.hall + (size_t)k * SHARD_HDR;
        const int code = (int)h[0];
        if (h[0] != 0.0) {
            if (k == e.rank) {
                const std::string last = cugp_last_error();
                snprintf(buf, sizeof buf, "%s: rank %d failed (%d): %s", e.call, k, code, last.c_str());
            } else snprintf(buf, sizeof buf, "%s: rank %d failed (%d)", e.call, k, code);
            return fail(code < 0 ? code : CUGP_ERR_DEVICE, buf);
        }
        for (int f = 2; f < 14; f++)
            if (memcmp(h + f, e.hall + f, sizeof(double))) {
                snprintf(buf, sizeof buf, "%s: rank %d disagrees with rank 0 in %s", e.call, k, SHARD_FIELD[f]);
                return fail(CUGP_ERR_INVALID, buf);
            }
        total = total + h[1];
        rows = rows + h[14];
    }
    if (total != (double)e.nshards) {
        snprintf(buf, sizeof buf, "%s: the ranks hold %.0f shards, %d expected", e.call, total, e.nshards);
        return fail(CUGP_ERR_INVALID, buf);
    }
    e.agreed = true;
    for (int i = 0; i < e.nlocal; i++) e.sh[i]->rows_total = (long long)rows;
    if (!e.kuu_pd) {                                                   // Kuu is not positive definite: NaN results
        r.valid = true;
        L->grp->valid = true;
        e.done = true;
        return CUGP_OK;
    }
    if ((rc = la_factor_inverse(b, true))) return rc;                  // LB, LB^-1, LB^-T, B^-1 (cugp_potri's route)
    if ((rc = use_device(u))) return rc;
    TuneScope ts(u);
    launch_trmv_lower(b->dT, mp, mp, q, cp, st);                       // c' = LB^-1 q
    HIPCHK(hipGetLastError());
    return CUGP_OK;
}

int sp_shard_rows(ShardEval& e, double* send)
{
    cugp_sparse* L = e.sh[0];
    cugp_gp *u = L->u, *b = L->b;
    hipStream_t st = e.stream;
    SparseSide& r = L->own;
    const int mp = e.mpad, nl = L->nh - 2, m = L->m, d = L->d;
    const bool want_z = e.what == 2;
    const double s2 = std::exp(L->theta[L->nh - 1] * 2);
    int rc;
    if ((rc = use_device(u))) return rc;
    TuneScope ts(u);
    double *cp = r.v(1, mp), *gp = r.v(2, mp), *bp = r.v(3, mp), *bsc = r.v(4, mp);
    double *H = L->dM[0], *H2 = L->dM[1], *X1 = L->dM[2], *R = L->dM[3];
    launch_trmv_upper(b->dU, mp, mp, cp, gp, st);                      // gamma' = LB^-T c'
    launch_trmv_upper(u->dU, mp, mp, gp, bp, st);                      // beta' = Lu^-T gamma'
    launch_sparse_h_targets(b->dKinv, L->dP, gp, bp, 1, m, mp, s2, H, H2, bsc, st);
    launch_targets_alpha(H, u->dU, X1, mp, mp, st);                    // H Lu^-1
    launch_sparse_transpose(X1, R, mp, 1.0 / s2, st);                  // R = Lu^-T H / s2
    launch_targets_alpha(H2, u->dU, X1, mp, mp, st);                   // H2 Lu^-1
    launch_sparse_transpose(X1, H, mp, 1.0, st);                       // Lu^-T H2
    launch_targets_alpha(H, u->dU, H2, mp, mp, st);                    // 2 G_uu = Lu^-T H2 Lu^-1
    for (int i = 0; i < e.nlocal; i++) {
        cugp_sparse* s = e.sh[i];
        double *row = send + (size_t)i * e.slot2, *zacc = row + nl + 1;  // [S_uf,k | the shard's running sums of the Z pass]
        const size_t nb_uf = sp_blocks_uf(s);
        const int chunks = sparse_shape(s->n, mp, s->chunk_rows, 0).chunks;
        size_t pofs = 0;
        for (int c = 0; c < chunks; c++) {
            const SparseShape sh = sparse_shape(s->n, mp, s->chunk_rows, c);
            if (chunks > 1) shard_chunk_w(L, s, e.cf, sh);             // (one chunk: the shard's W is still there)
            launch_sparse_weights(s->dW, R, s->dG, sh.cpad, mp, st);
            const double *xr = s->dX + (size_t)sh.r0 * d, *yv = s->own.y + sh.r0;
            launch_trace_cross(xr, sh.count, sh.cpad, u->dX, m, d, mp, e.cf, s->dG, yv, bsc, s->dpart, nb_uf, pofs, st);
            if (want_z)
                launch_trace_cross_z(xr, sh.count, sh.cpad, u->dX, m, d, mp, e.cf, s->dG, yv, bsc, s->dzpart, zacc, c == 0, false,
                                     s->dzout, s->hz, st);
            pofs += (size_t)(sh.cpad / 64) * (mp / 64);
        }
        launch_sparse_shard_sums(s->dpart, nb_uf, nl, row, st);
    }
    const size_t nb_uu = (size_t)(mp / 64) * (mp / 64);
    launch_trace_cross(u->dX, m, mp, u->dX, m, d, mp, e.cf, H2, nullptr, nullptr, L->dpart + (size_t)(nl + 1) * sp_blocks_uf(L), nb_uu,
                       0, st);
    HIPCHK(hipGetLastError());
    return CUGP_OK;
}

int sp_shard_finish(ShardEval& e, const double* g, size_t rstride)
{
    cugp_sparse* L = e.sh[0];
    cugp_gp *u = L->u, *b = L->b;
    hipStream_t st = e.stream;
    SparseSide& r = L->own;
    const int mp = e.mpad, nl = L->nh - 2, m = L->m, d = L->d, nrow = 2 + L->nh;
    const bool want_grad = e.what >= 1, want_z = e.what == 2;
    const double sf2 = std::exp(L->theta[L->nh - 2] * 2), s2 = std::exp(L->theta[L->nh - 1] * 2), ls2 = L->theta[L->nh - 1] * 2;
    int rc;
    if ((rc = use_device(u))) return rc;
    TuneScope ts(u);
    const size_t nb_uu = (size_t)(mp / 64) * (mp / 64);
    const double* part_uu = want_grad ? L->dpart + (size_t)(nl + 1) * sp_blocks_uf(L) : nullptr;
    double* suf = want_grad ? L->dglob + 2 : nullptr;
    if (want_grad) launch_sparse_shard_reduce(g, rstride, 0, e.slot2, 0, (size_t)nl + 1, e.world, e.nshards, suf, st);
    if (want_z) {
        launch_sparse_shard_reduce(g, rstride, 0, e.slot2, (size_t)nl + 1, (size_t)m * d, e.world, e.nshards, L->dzacc, st);
        for (size_t i = 0; i < (size_t)m * d; i++) L->hz[i] = NAN;
        launch_trace_cross_z(u->dX, m, mp, u->dX, m, d, mp, e.cf, L->dM[1], nullptr, nullptr, L->dzpart, L->dzacc, false, true,
                             L->dzout, L->hz, st);
    }
    for (int i = 0; i < nrow; i++) r.hout[i] = NAN;
    const SparseFinalSharded fin{L->dP, b->dKinv, r.v(1, mp), r.v(2, mp), b->dlogdet, L->dglob, m, mp, b->nt, sf2, s2, ls2};
    launch_sparse_finalize_sharded(fin, suf, part_uu, nb_uu, nl, r.dout, r.hout, st);
    if ((rc = sync_or_fail(st, e.call, hipGetLastError()))) return rc;
    r.pd = std::isfinite(r.hout[0]);
    if (r.pd) {                                                        // (B is not positive definite, or a NaN in the data: NaN results)
        r.row[0] = r.hout[0];
        if (want_grad) std::copy(r.hout + 1, r.hout + 1 + L->nh, r.row.begin() + 1);
        r.row[1 + L->nh] = r.hout[1 + L->nh];
        if (want_z) std::copy(L->hz, L->hz + (size_t)m * d, r.gz.begin());
    }
    r.valid = true;
    L->grp->valid = true;
    e.done = true;
    return CUGP_OK;
}

int sp_shard_results(const ShardEval& e, double* F, double* g, double* gZ)
{
    const cugp_sparse* L = e.sh[0];
    const SparseSide& r = L->own;
    *F = r.row[0];
    if (e.what >= 1) std::copy(r.row.begin() + 1, r.row.begin() + 1 + L->nh, g);
    if (e.what == 2) std::copy(r.gz.begin(), r.gz.end(), gZ);
    return CUGP_OK;
}

}  // namespace cugp
