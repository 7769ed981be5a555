// Host check of the matrix-free GP's vector kernels (cugp_amd/csrc/iter_device.h; tools/iter_host_check.py builds and runs
// this; no GPU): the kernels' own text behind tools/host_emul.h, 256 host threads per workgroup in lock step, on heap blocks
// of exactly the library's sizes, under -fsanitize=address,undefined.  One sweep of the t recurrences -- b'b, the start, p'q
// and the step length, the update with r'r, the ratio, the new direction, then the true-residual pass, the poisoning of
// broken columns, the closing pass over the still-active columns and k_iter_sum -- on a q the caller supplies (the product itself needs the MFMA), and k_iter_cross_rhs for one
// isotropic and the rational quadratic instantiation; then the mixed mode's cycle kernels (check_mixed below) and the test-input
// gradients' kernel with its finish (iter_xgrad_device.h; check_xgrad below), and the Lanczos quadrature's k_iter_record and k_slq_quad (check_slq below).  Every output is compared BIT FOR BIT with the plain loops below in
// the kernels' order of summation: the 16 row classes of a workgroup each in row order, the classes ascending, the
// workgroups ascending.  Exit code 4: a mismatch.  A stand-alone program: the sanitizer is linked in, nothing is preloaded.
#include "host_emul.h"
namespace cugp {
#include "cov_device.h"
#include "iter_device.h"
#include "iter_xgrad_device.h"
}
using namespace cugp;

namespace {
#pragma clang fp contract(off)
double ref_dot(const double* a, const double* b, int n, int tp, int c)
{
    double tot = 0.0;
    for (int blk = 0; blk < iter_blocks(n); blk++) {
        const size_t r0 = (size_t)blk * IT_ROWS, r1 = std::min<size_t>(r0 + IT_ROWS, n);
        double cls[IT_LANES];
        for (int rho = 0; rho < IT_LANES; rho++) {
            cls[rho] = 0.0;
            for (size_t i = r0 + rho; i < r1; i += IT_LANES) cls[rho] = cls[rho] + a[i * tp + c] * b[i * tp + c];
        }
        double s = cls[0];
        for (int rho = 1; rho < IT_LANES; rho++) s = s + cls[rho];
        tot = blk == 0 ? s : tot + s;
    }
    return tot;
}
bool same_bits(const double* a, const double* b, size_t cnt, const char* what)
{
    for (size_t i = 0; i < cnt; i++)
        if (memcmp(a + i, b + i, 8) != 0) {
            fprintf(stdout, "MISMATCH %s entry %zu: kernel %.17g, plain loop %.17g\n", what, i, a[i], b[i]);
            return false;
        }
    return true;
}
template <bool ARD, int KIND>
bool check_rhs(const double* X, int n, int d, const double* Xt, int count, int tp, const double* hdw, double* R)
{
    const size_t cnt = (size_t)n * tp;
    launch((int)((cnt + 255) / 256), [&] { k_iter_cross_rhs<ARD, KIND>(X, n, d, Xt, count, tp, (const HyperScalars*)hdw, R); });
    std::vector<double> ref(cnt, 0.0);
    const double* w = hdw + 3;
    for (int j = 0; j < n; j++)
        for (int c = 0; c < count; c++) {
            double acc = 0.0;
            for (int f = 0; f < d; f++) {
                double df = X[(size_t)j * d + f] - Xt[(size_t)c * d + f];
                if (ARD) df = df * w[f];
                acc = acc + df * df;
            }
            ref[(size_t)j * tp + c] = kernel_value<ARD, KIND>(acc, div_prepare(hdw[0]), hdw[1], ShapeArgs{w[d], w[d + 1]});
        }
    return same_bits(R, ref.data(), cnt, ARD ? "rhs rq" : "rhs se");
}

// ---- the mixed mode's one-workgroup kernels (k_iter_goal_init, k_iter_step_b_mx, k_iter_step_v_mx): two cycles and a closing
// pass on shares the program lays out itself, one scenario per column, everything in units of the column's b'b.
// T = tol^2 = 2^-10, R = rho^2 = 2^-4; every figure is dyadic, so the shares add up exactly and `equal` cases are equal.
constexpr int MX_STAGES = 6, MX_CASES = 11;
constexpr double MX_T = 0x1p-10, MX_R = 0x1p-4, MX_NAN = __builtin_nan("");
enum { MX_RN1, MX_RT1, MX_PQ, MX_RN2, MX_RT2, MX_RT3 };
// column:                        0 tol   1 goal,  2 grown, 3 stays  4 NaN   5 b = 0 6 goal,  7 at the 8 last leg 9 last leg 10 b NaN
//                                reached   stalls   stalls   active   r'r             NaN true goal     not flagged flagged
const double MX_TAB[MX_STAGES][MX_CASES] = {
    /* r'r, sweep 1        */ {MX_T / 2, MX_R / 2, 0x1p21,  0.5,     MX_NAN, 1.0,    MX_R / 2, MX_R,    MX_R / 2,   MX_R / 2,  1.0},
    /* true r'r, check 1   */ {MX_T,     0.5,      2.0,     1.0,     1.0,    1.0,    MX_NAN,   0.125,   3 * MX_T,   3 * MX_T,  1.0},
    /* p'q                 */ {2.0,      2.0,      2.0,     2.0,     2.0,    2.0,    2.0,      2.0,     2.0,        2.0,       2.0},
    /* r'r, sweep 2        */ {1.0,      0.25,     1.0,     0.25,    1.0,    1.0,    1.0,      0x1p-7,  MX_T / 2,   MX_T / 2,  1.0},
    /* true r'r, check 2   */ {1.0,      1.0,      1.0,     1.0,     1.0,    1.0,    1.0,      MX_T / 2, 1.5 * MX_T, 2 * MX_T, 1.0},
    /* true r'r, final = 1 */ {1.0,      MX_T / 4, 0.5,     MX_NAN,  1.0,    1.0,    1.0,      1.0,     1.0,        1.0,       1.0}};
const double MX_REST[MX_STAGES] = {0.5, 1.0, 2.0, 0.25, 1.0, 0.25};        // columns 11 and up: active to the end

double mx_bb(int c) { return c == 5 ? 0.0 : c == 10 ? MX_NAN : 4.0 * (double)(1 << (c % 3)); }
double mx_value(int stage, int c) { return (c < MX_CASES ? MX_TAB[stage][c] : MX_REST[stage]) * (stage == MX_PQ ? 1.0 : mx_bb(c)); }
// the value v in nblk shares that add up to it exactly: half in the first block, the rest in equal parts
void mx_shares(double* part, int nblk, int tp, int stage)
{
    for (int c = 0; c < tp; c++) {
        const double v = stage < 0 ? mx_bb(c) : mx_value(stage, c);
        for (int b = 0; b < nblk; b++) part[(size_t)b * tp + c] = nblk == 1 ? v : (b == 0 ? v * 0.5 : v * 0.5 / (nblk - 1));
    }
}
double mx_sum(const double* part, int nblk, int tp, int c)
{
    double s = part[c];
    for (int b = 1; b < nblk; b++) s = s + part[(size_t)b * tp + c];
    return s;
}
bool check_mixed(int nblk, int tp, double* sc)
{
    const double tol = 0x1p-5, rho2 = MX_R;
    double* part = (double*)malloc((size_t)nblk * tp * 8);
    std::vector<double> rs(SC_ALLOC * IT_MAXT, -7.0);                 // (-7: a row or column no kernel may touch)
    for (int e = 0; e < SC_ALLOC * IT_MAXT; e++) sc[e] = -7.0;
    auto stage = [&](int st, auto&& kernel) { mx_shares(part, nblk, tp, st); launch(1, kernel); };
    stage(-1, [&] { k_iter_init(part, nblk, tp, tol, sc); });
    launch(1, [&] { k_iter_goal_init(tp, rho2, sc); });
    stage(MX_RN1, [&] { k_iter_step_b_mx(part, nblk, tp, sc); });
    stage(MX_RT1, [&] { k_iter_step_v_mx(part, nblk, tp, 0, rho2, sc); });
    stage(MX_PQ, [&] { k_iter_step_a(part, nblk, tp, sc); });
    stage(MX_RN2, [&] { k_iter_step_b_mx(part, nblk, tp, sc); });
    stage(MX_RT2, [&] { k_iter_step_v_mx(part, nblk, tp, 0, rho2, sc); });
    stage(MX_RT3, [&] { k_iter_step_v_mx(part, nblk, tp, 1, rho2, sc); });
    // the same, column by column
    for (int c = 0; c < tp; c++) {
        auto at = [&](int row) -> double& { return rs[row * IT_MAXT + c]; };
        auto sum = [&](int st) { mx_shares(part, nblk, tp, st); return mx_sum(part, nblk, tp, c); };
        const double bb = sum(-1);
        at(SC_RR) = at(SC_BB) = at(SC_TRUE) = at(SC_PREV) = bb;
        at(SC_TOL2) = (tol * tol) * bb;
        at(SC_A) = at(SC_B) = at(SC_ITERS) = at(SC_STALL) = 0.0;
        at(SC_GOAL) = rho2 * bb;
        double st = bb == 0.0 ? ST_DONE : (bb - bb == 0.0 ? ST_ACTIVE : ST_BROKEN);
        auto sweep = [&](int which) {
            if (st != ST_ACTIVE) return;
            const double rn = sum(which);
            at(SC_ITERS) = at(SC_ITERS) + 1.0;
            if (!(rn - rn == 0.0)) { st = ST_BROKEN; return; }
            at(SC_B) = rn / at(SC_RR);
            at(SC_RR) = rn;
            if (rn <= at(SC_TOL2)) st = ST_CANDIDATE;                 // the tolerance
            else if (rn <= at(SC_GOAL)) st = ST_CANDIDATE;            // the cycle's goal
            else if (rn > 1048576.0 * at(SC_PREV)) st = ST_CANDIDATE; // grown 2^20-fold since the last true residual
        };
        auto verify = [&](int which, bool final) {
            if (!(st == ST_CANDIDATE || (final && st == ST_ACTIVE))) return;
            const double rt = sum(which);
            at(SC_TRUE) = rt;
            if (!(rt - rt == 0.0)) { st = ST_BROKEN; return; }
            if (rt <= at(SC_TOL2)) { st = ST_DONE; return; }
            if (final) return;
            const double low = at(SC_GOAL) > at(SC_TOL2) ? at(SC_GOAL) : at(SC_TOL2), asked = at(SC_PREV) / low;
            double need = 4.0;
            if (asked < 16.0) need = __builtin_sqrt(asked);
            if (need * rt > at(SC_PREV)) at(SC_STALL) = 1.0;
            at(SC_RR) = at(SC_PREV) = rt;
            at(SC_GOAL) = rho2 * rt;
            st = ST_RESTART;
        };
        sweep(MX_RN1);
        verify(MX_RT1, false);
        if (st == ST_RESTART) st = ST_ACTIVE;
        if (st == ST_ACTIVE) at(SC_A) = at(SC_RR) / sum(MX_PQ);      // (p'q = 2 > 0 in every column)
        sweep(MX_RN2);
        verify(MX_RT2, false);
        verify(MX_RT3, true);
        at(SC_STATE) = st;
    }
    free(part);
    return same_bits(sc, rs.data(), SC_ALLOC * IT_MAXT, "mixed scalar");
}

// ---- k_cov_xgrad and its finish (iter_xgrad_device.h) on data of the program's own: ragged nt and n, d = 17 (two feature
// chunks: blockIdx.z), two ranges (blockIdx.y), against plain loops in the kernel's stated order -- per output the four fk
// groups each over their entries j = 32 st + 4 kk + fk in ascending order (rows beyond n as the zeros they are staged as),
// (0 + 1) + (2 + 3), the ranges ascending, then the scale and the sign.  VAR: nt <= tp points against their own columns of Wv.
double xg_rand(unsigned& s) { s = s * 1664525u + 1013904223u; return (double)(s >> 8) / 8388608.0 - 1.0; }
template <bool ARD, int KIND, bool VAR>
bool check_xgrad(int nt, int n, int d, int tp, int split, const char* what)
{
    unsigned seed = 12345u + nt + n;
    auto blk = [&](size_t c) { double* p = (double*)malloc(c * 8); for (size_t i = 0; i < c; i++) p[i] = xg_rand(seed); return p; };
    double *Xt = blk((size_t)nt * d), *X = blk((size_t)n * d), *wm = blk((size_t)n * 16), *Wv = blk((size_t)n * tp), *hdw = blk(3 + d + 2);
    hdw[0] = ARD ? 1.0 : 2.25; hdw[1] = 1.5; hdw[2] = 0.2;
    for (int c = 0; c < d + 2; c++) hdw[3 + c] = 0.6 + 0.4 * std::fabs(hdw[3 + c]);
    hdw[3 + d + 1] = 0.5 / hdw[3 + d];
    for (int c = 0; c < d; c++) Xt[c] = X[(size_t)(n / 2) * d + c];          // one test point on a training point
    const int nq = VAR ? 2 : 1, nst = (n + ITER_JT - 1) / ITER_JT, per = (nst + split - 1) / split, nz = (d + DC - 1) / DC;
    const int row_blocks = (nt + ITER_ROWS - 1) / ITER_ROWS;
    const size_t cnt = (size_t)nt * d;
    double *part = blk((size_t)split * nq * cnt), *om = blk(cnt), *ov = blk(cnt);
    const HyperScalars* hd = (const HyperScalars*)hdw;
    gridDim.y = split; gridDim.z = nz;
    for (int s = 0; s < split; s++)
        for (int z = 0; z < nz; z++) {
            blockIdx.y = s; blockIdx.z = z;
            launch(row_blocks, [&] { k_cov_xgrad<ARD, KIND, VAR>(Xt, nt, X, n, d, hd, wm, VAR ? Wv : nullptr, tp, part, per); });
        }
    blockIdx.y = blockIdx.z = 0; gridDim.y = gridDim.z = 1;
    launch((int)((cnt + 255) / 256), [&] { k_cov_xgrad_finish(part, split, nq, cnt, d, hd, ARD ? 1 : 0, 2.0, om, VAR ? ov : nullptr); });
    std::vector<double> rm(cnt), rv(cnt);
    const double* w = hdw + 3;
    const DivBy dl = div_prepare(hdw[0]);
    const ShapeArgs sh{w[d], w[d + 1]};
    for (int i = 0; i < nt; i++)
        for (int a = 0; a < d; a++) {
            double tm = 0.0, tv = 0.0;
            for (int s = 0; s < split; s++) {
                double gm[4], gv[4];
                for (int fk = 0; fk < 4; fk++) {
                    gm[fk] = gv[fk] = 0.0;
                    for (int st = s * per; st < std::min((s + 1) * per, nst); st++)
                        for (int kk = 0; kk < ITER_JT / 4; kk++) {
                            const int j = st * ITER_JT + 4 * kk + fk;
                            double sq = 0.0;
                            for (int f = 0; f < d; f++) {
                                double df = Xt[(size_t)i * d + f] - (j < n ? X[(size_t)j * d + f] : 0.0);
                                if (ARD) df = df * w[f];
                                sq = sq + df * df;
                            }
                            const double g = xgrad_factor<ARD, KIND>(sq, dl, hdw[1], sh);
                            const double df = Xt[(size_t)i * d + a] - (j < n ? X[(size_t)j * d + a] : 0.0);
                            gm[fk] = gm[fk] + (g * (j < n ? wm[(size_t)j * 16] : 0.0)) * df;
                            if (VAR) gv[fk] = gv[fk] + (g * (j < n ? Wv[(size_t)j * tp + i] : 0.0)) * df;
                        }
                }
                const double pm = (gm[0] + gm[1]) + (gm[2] + gm[3]), pv = (gv[0] + gv[1]) + (gv[2] + gv[3]);
                tm = s == 0 ? pm : tm + pm;
                tv = s == 0 ? pv : tv + pv;
            }
            const double sc = ARD ? w[a] * w[a] : 1.0 / hdw[0];
            rm[(size_t)i * d + a] = -(sc * tm);
            rv[(size_t)i * d + a] = (2.0 * sc) * tv;
        }
    bool ok = same_bits(om, rm.data(), cnt, what) && (!VAR || same_bits(ov, rv.data(), cnt, what));
    double big = 0.0;
    for (size_t e = 0; e < cnt; e++) big = std::max(big, std::fabs(om[e]));
    ok = ok && big > 0.0;                                                    // (not a comparison of zeros)
    for (double* v : {Xt, X, wm, Wv, hdw, part, om, ov}) free(v);
    return ok;
}

// ---- the Lanczos quadrature's one-workgroup kernels (k_iter_record, k_slq_quad; iter_device.h): eight sweeps of scalars the
// program lays out itself, a scenario per column -- active to the end, a candidate at sweep 3 that restarts and runs on (its
// later sweeps must not be logged), broken at sweep 2, done and broken from the start, a candidate at sweep 0, the rest closing
// at sweep c mod 8 -- then every log's quadrature, bit for bit against the plain loops below (the same QL iteration on
// contiguous arrays).  The quadrature's first two moments (sum tau^2 = 1, sum tau^2 lambda = T_00) are checked beside the bits.
constexpr int SQ_CAP = 12, SQ_SWEEPS = 8;
double sq_a(int c, int j) { return 0.5 + 0.03125 * (double)((c + 1) * (j + 1) % 7); }
double sq_b(int c, int j) { return 0.75 / (double)(j + 1 + c % 5); }
double sq_state(int c, int j)      // the column's state as k_iter_record finds it behind sweep j (-1: the start)
{
    if (c == 3) return ST_DONE;
    if (c == 4) return ST_BROKEN;
    if (c == 2) return j >= 2 ? ST_BROKEN : ST_ACTIVE;
    if (c == 0) return ST_ACTIVE;
    const int close = c == 1 ? 3 : c == 5 ? 0 : c % SQ_SWEEPS;
    if (j < close) return ST_ACTIVE;
    return j == close ? ST_CANDIDATE : (j == close + 1 ? ST_RESTART : ST_ACTIVE);
}
double ref_quad(const std::vector<double>& a, const std::vector<double>& b, double w, bool broken, bool* moments)
{
    const int m = (int)a.size();
    if (broken) return __builtin_nan("");
    if (m == 0) return 0.0;
    std::vector<double> dg(m), of(m), tau(m, 0.0);
    for (int j = 0; j < m; j++) {
        dg[j] = j == 0 ? 1.0 / a[j] : 1.0 / a[j] + b[j - 1] / a[j - 1];
        of[j] = j + 1 < m ? __builtin_sqrt(b[j]) / a[j] : 0.0;
    }
    tau[0] = 1.0;
    const double t00 = dg[0];
    for (int l = 0; l < m; l++)
        for (int iter = 0;; iter++) {
            int mm = l;
            for (; mm < m - 1; mm++) {
                const double dd = std::fabs(dg[mm]) + std::fabs(dg[mm + 1]);
                if (std::fabs(of[mm]) + dd == dd) break;
            }
            if (mm == l) break;
            if (iter == 30) return __builtin_nan("");
            double g = (dg[l + 1] - dg[l]) / (2.0 * of[l]), r = __builtin_sqrt(g * g + 1.0);
            g = dg[mm] - dg[l] + of[l] / (g + (g >= 0.0 ? r : -r));
            double s = 1.0, cs = 1.0, p = 0.0;
            int i = mm - 1;
            for (; i >= l; i--) {
                double f = s * of[i];
                const double bb = cs * of[i];
                r = __builtin_sqrt(f * f + g * g);
                of[i + 1] = r;
                if (r == 0.0) { dg[i + 1] = dg[i + 1] - p; of[mm] = 0.0; break; }
                s = f / r; cs = g / r;
                g = dg[i + 1] - p;
                r = (dg[i] - g) * s + 2.0 * cs * bb;
                p = s * r;
                dg[i + 1] = g + p;
                g = cs * r - bb;
                f = tau[i + 1];
                tau[i + 1] = s * tau[i] + cs * f;
                tau[i] = cs * tau[i] - s * f;
            }
            if (r == 0.0 && i >= l) continue;
            dg[l] = dg[l] - p; of[l] = g; of[mm] = 0.0;
        }
    for (int i = 1; i < m; i++)
        for (int k = i; k > 0 && dg[k - 1] > dg[k]; k--) { std::swap(dg[k - 1], dg[k]); std::swap(tau[k - 1], tau[k]); }
    double s = 0.0, m0 = 0.0, m1 = 0.0;
    for (int i = 0; i < m; i++) {
        if (!(dg[i] > 0.0 && dg[i] - dg[i] == 0.0)) return __builtin_nan("");
        const double term = (tau[i] * tau[i]) * log(dg[i]);
        s = i == 0 ? term : s + term;
        m0 += tau[i] * tau[i]; m1 += tau[i] * tau[i] * dg[i];
    }
    *moments = *moments && std::fabs(m0 - 1.0) < 1e-13 && std::fabs(m1 - t00) < 1e-13 * t00;
    return w * s;
}
bool check_slq(int tp)
{
    auto blk = [&](size_t c) { double* p = (double*)malloc(c * 8); for (size_t i = 0; i < c; i++) p[i] = -7.0; return p; };
    double *sc = blk(SC_ALLOC * IT_MAXT), *rec = blk((size_t)2 * SQ_CAP * IT_MAXT), *meta = blk(ML_ROWS * IT_MAXT);
    double *work = blk((size_t)3 * SQ_CAP * IT_MAXT), *quad = blk(IT_MAXT);
    std::vector<double> rrec((size_t)2 * SQ_CAP * IT_MAXT, -7.0), rmeta(ML_ROWS * IT_MAXT, -7.0), rquad(IT_MAXT, -7.0);
    for (int c = 0; c < tp; c++) { sc[SC_STATE * IT_MAXT + c] = sq_state(c, -1); sc[SC_RZ * IT_MAXT + c] = 3.0 + c; }
    launch(1, [&] { k_iter_record(sc, tp, 1, SC_RZ, SQ_CAP, rec, meta); });
    for (int j = 0; j < SQ_SWEEPS; j++) {
        for (int c = 0; c < tp; c++) {
            sc[SC_STATE * IT_MAXT + c] = sq_state(c, j);
            sc[SC_A * IT_MAXT + c] = sq_a(c, j);
            sc[SC_B * IT_MAXT + c] = sq_b(c, j);
        }
        launch(1, [&] { k_iter_record(sc, tp, 0, 0, SQ_CAP, rec, meta); });
    }
    launch(1, [&] { k_slq_quad(rec, meta, tp, SQ_CAP, work, quad); });
    bool moments = true;
    int lens = 0;
    for (int c = 0; c < tp; c++) {
        std::vector<double> a, b;
        bool closed = false, broken = false;
        for (int j = 0; j < SQ_SWEEPS && !closed; j++) {
            const double st = sq_state(c, j);
            if (st == ST_ACTIVE) { a.push_back(sq_a(c, j)); b.push_back(sq_b(c, j)); continue; }
            closed = true;
            broken = st == ST_BROKEN;
            if (st == ST_CANDIDATE) { a.push_back(sq_a(c, j)); b.push_back(0.0); }
        }
        for (size_t j = 0; j < a.size(); j++) { rrec[j * IT_MAXT + c] = a[j]; rrec[(SQ_CAP + j) * IT_MAXT + c] = b[j]; }
        rmeta[ML_LEN * IT_MAXT + c] = (double)a.size();
        rmeta[ML_CLOSED * IT_MAXT + c] = closed ? 1.0 : 0.0;
        rmeta[ML_BROKEN * IT_MAXT + c] = broken ? 1.0 : 0.0;
        rmeta[ML_W * IT_MAXT + c] = 3.0 + c;
        rquad[c] = ref_quad(a, b, 3.0 + c, broken, &moments);
        lens += (int)a.size();
    }
    bool ok = same_bits(rec, rrec.data(), rrec.size(), "log") && same_bits(meta, rmeta.data(), rmeta.size(), "log meta") &&
              same_bits(quad, rquad.data(), IT_MAXT, "quadrature");
    ok = ok && moments && lens > 3 * tp && quad[3] == 0.0 && quad[2] != quad[2] && quad[4] != quad[4] && rmeta[ML_LEN * IT_MAXT + 1] == 4.0;
    for (double* v : {sc, rec, meta, work, quad}) free(v);
    return ok;
}
}  // namespace

int main(int argc, char** argv)
{
    // `--slq` (a mode of its own, no files): k_iter_record and k_slq_quad at both block widths
    if (argc == 2 && strcmp(argv[1], "--slq") == 0) return check_slq(16) && check_slq(IT_MAXT) ? 0 : 4;
    // input: ints n tp d count, doubles hd[3 + d + 2] X[n d] Xt[count d] b[n tp] q[n tp] -> output: x r p sc R_se R_rq
    // `--xgrad` (a mode of its own: the data is the program's, no files): k_cov_xgrad and its finish, (nt, n, d, tp, split)
    if (argc == 2 && strcmp(argv[1], "--xgrad") == 0) {
        bool ok = check_xgrad<true, KERNEL_RQ, true>(21, 77, 17, 64, 2, "xgrad rq var");
        ok = check_xgrad<true, KERNEL_MATERN32, true>(17, 40, 3, 64, 1, "xgrad matern32 ard var") && ok;
        ok = check_xgrad<false, KERNEL_MATERN52, true>(5, 33, 3, 16, 1, "xgrad matern52 var") && ok;
        ok = check_xgrad<false, KERNEL_SE, false>(70, 77, 17, 16, 2, "xgrad se mean") && ok;
        return ok ? 0 : 4;
    }
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    int hdr[4];
    if (!f || fread(hdr, sizeof(int), 4, f) != 4) return 2;
    const int n = hdr[0], tp = hdr[1], d = hdr[2], count = hdr[3];
    auto rd = [&](size_t cnt) { double* p = (double*)malloc(cnt * 8); if (fread(p, 8, cnt, f) != cnt) exit(3); return p; };
    const size_t cnt = (size_t)n * tp;
    double *hdw = rd(3 + d + 2), *X = rd((size_t)n * d), *Xt = rd((size_t)count * d), *b = rd(cnt), *q = rd(cnt);
    fclose(f);
    const int nblk = iter_blocks(n);
    auto blk = [&](size_t c) { return (double*)malloc(c * 8); };
    double *x = blk(cnt), *r = blk(cnt), *p = blk(cnt), *part = blk((size_t)nblk * tp), *sc = blk(SC_ROWS * IT_MAXT);
    double *Rs = blk(cnt), *Rq = blk(cnt);
    const double tol = 0.5;                              // (loose: some columns pass after one sweep, some do not)
    launch(nblk, [&] { k_iter_dot(b, b, n, tp, part); });
    launch(1, [&] { k_iter_init(part, nblk, tp, tol, sc); });
    launch((int)((cnt + 255) / 256), [&] { k_iter_start(b, x, r, p, cnt); });
    launch(nblk, [&] { k_iter_dot(p, q, n, tp, part); });
    launch(1, [&] { k_iter_step_a(part, nblk, tp, sc); });
    launch(nblk, [&] { k_iter_update(x, r, p, q, n, tp, sc, part); });
    launch(1, [&] { k_iter_step_b(part, nblk, tp, sc); });
    launch(nblk, [&] { k_iter_dir(p, r, n, tp, sc, 0); });
    launch(nblk, [&] { k_iter_resid(b, q, r, n, tp, sc, 0, part); });
    launch(1, [&] { k_iter_step_v(part, nblk, tp, 0, sc); });
    launch(nblk, [&] { k_iter_dir(p, r, n, tp, sc, 1); });
    launch(nblk, [&] { k_iter_poison(x, n, tp, sc); });
    // the closing pass of a solve that ran out of sweeps: the true residual of the still-active columns, then the whole sums
    double* sums = blk(tp);
    launch(nblk, [&] { k_iter_resid(b, q, r, n, tp, sc, 1, part); });
    launch(1, [&] { k_iter_step_v(part, nblk, tp, 1, sc); });
    launch(1, [&] { k_iter_sum(part, nblk, tp, sums); });
    // the mixed mode's fall back, on copies: the unfinished columns start again, the finished and the broken ones stay
    double *x2 = blk(cnt), *r2 = blk(cnt), *sc2 = blk(SC_ROWS * IT_MAXT);
    memcpy(x2, x, cnt * 8); memcpy(r2, r, cnt * 8); memcpy(sc2, sc, SC_ROWS * IT_MAXT * 8);
    launch(nblk, [&] { k_iter_again(b, x2, r2, n, tp, sc2); });
    launch(1, [&] { k_iter_again_sc(tp, sc2); });
    // the same sweep, column by column
    std::vector<double> rx(cnt), rr(cnt), rp(cnt), rs(SC_ROWS * IT_MAXT, 0.0);
    bool ok = true;
    for (int c = 0; c < tp; c++) {
        auto at = [&](int row) -> double& { return rs[row * IT_MAXT + c]; };
        const double bb = ref_dot(b, b, n, tp, c);
        at(SC_RR) = at(SC_BB) = at(SC_TRUE) = bb;
        at(SC_TOL2) = (tol * tol) * bb;
        double st = bb == 0.0 ? ST_DONE : (bb - bb == 0.0 ? ST_ACTIVE : ST_BROKEN);
        for (int i = 0; i < n; i++) { rx[(size_t)i * tp + c] = 0.0; rr[(size_t)i * tp + c] = rp[(size_t)i * tp + c] = b[(size_t)i * tp + c]; }
        if (st == ST_ACTIVE) {
            const double pq = ref_dot(rp.data(), q, n, tp, c);
            if (pq > 0.0 && pq - pq == 0.0) at(SC_A) = bb / pq; else st = ST_BROKEN;
        }
        if (st == ST_ACTIVE) {
            for (int i = 0; i < n; i++) {
                const size_t e = (size_t)i * tp + c;
                rx[e] = rx[e] + at(SC_A) * rp[e];
                rr[e] = rr[e] - at(SC_A) * q[e];
            }
            const double rn = ref_dot(rr.data(), rr.data(), n, tp, c);
            at(SC_ITERS) = 1.0;
            if (!(rn - rn == 0.0)) st = ST_BROKEN;
            else {
                at(SC_B) = rn / at(SC_RR);
                at(SC_RR) = rn;
                if (rn <= at(SC_TOL2)) st = ST_CANDIDATE;
            }
        }
        if (st == ST_ACTIVE)
            for (int i = 0; i < n; i++) { const size_t e = (size_t)i * tp + c; rp[e] = rr[e] + at(SC_B) * rp[e]; }
        if (st == ST_CANDIDATE) {
            for (int i = 0; i < n; i++) { const size_t e = (size_t)i * tp + c; rr[e] = b[e] - q[e]; }
            const double rt = ref_dot(rr.data(), rr.data(), n, tp, c);
            at(SC_TRUE) = rt;
            if (!(rt - rt == 0.0)) st = ST_BROKEN;
            else if (rt <= at(SC_TOL2)) st = ST_DONE;
            else { at(SC_RR) = rt; st = ST_RESTART; }
        }
        if (st == ST_RESTART)
            for (int i = 0; i < n; i++) rp[(size_t)i * tp + c] = rr[(size_t)i * tp + c];
        if (st == ST_BROKEN)
            for (int i = 0; i < n; i++) rx[(size_t)i * tp + c] = __builtin_nan("");
        if (st == ST_ACTIVE) {                                   // final: it stays active unless the true residual passes
            for (int i = 0; i < n; i++) { const size_t e = (size_t)i * tp + c; rr[e] = b[e] - q[e]; }
            const double rt = ref_dot(rr.data(), rr.data(), n, tp, c);
            at(SC_TRUE) = rt;
            if (!(rt - rt == 0.0)) st = ST_BROKEN;
            else if (rt <= at(SC_TOL2)) st = ST_DONE;
        }
        const double whole = ref_dot(rr.data(), rr.data(), n, tp, c);
        ok = ok && same_bits(sums + c, &whole, 1, "sum");
        at(SC_STATE) = st;
        for (int row = 0; row < SC_ROWS; row++) ok = ok && same_bits(sc + row * IT_MAXT + c, &at(row), 1, "scalar");
    }
    ok = ok && same_bits(x, rx.data(), cnt, "x") && same_bits(r, rr.data(), cnt, "r") && same_bits(p, rp.data(), cnt, "p");
    int again = 0;
    for (int c = 0; c < tp; c++) {
        auto at = [&](int row) -> double& { return rs[row * IT_MAXT + c]; };
        if (at(SC_STATE) != ST_ACTIVE && at(SC_STATE) != ST_RESTART) continue;
        for (int i = 0; i < n; i++) { rx[(size_t)i * tp + c] = 0.0; rr[(size_t)i * tp + c] = b[(size_t)i * tp + c]; }
        at(SC_RR) = at(SC_TRUE) = at(SC_BB);
        at(SC_STATE) = ST_RESTART;
        again++;
    }
    ok = ok && same_bits(x2, rx.data(), cnt, "x again") && same_bits(r2, rr.data(), cnt, "r again");
    for (int row = 0; row < SC_ROWS; row++) ok = ok && same_bits(sc2 + row * IT_MAXT, rs.data() + row * IT_MAXT, tp, "scalar again");
    ok = ok && (n == 1 || again > 0);
    ok = check_rhs<false, KERNEL_SE>(X, n, d, Xt, count, tp, hdw, Rs) && ok;
    ok = check_rhs<true, KERNEL_RQ>(X, n, d, Xt, count, tp, hdw, Rq) && ok;
    double* scm = blk(SC_ALLOC * IT_MAXT);
    ok = check_mixed(nblk, tp, scm) && ok;
    FILE* o = fopen(argv[2], "wb");
    for (const double* v : {x, r, p}) fwrite(v, 8, cnt, o);
    fwrite(sc, 8, SC_ROWS * IT_MAXT, o);
    fwrite(Rs, 8, cnt, o);
    fwrite(Rq, 8, cnt, o);
    fwrite(scm, 8, SC_ALLOC * IT_MAXT, o);
    fclose(o);
    for (double* v : {hdw, X, Xt, b, q, x, r, p, part, sc, Rs, Rq, sums, scm, x2, r2, sc2}) free(v);
    return ok ? 0 : 4;
}
