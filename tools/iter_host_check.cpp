// Host check of the matrix-free GP's vector kernels (cugp_amd/csrc/iter_device.h; tools/iter_host_check.py builds and runs
// this; no GPU): the kernels' own text behind tools/host_emul.h, 256 host threads per workgroup in lock step, on heap blocks
// of exactly the library's sizes, under -fsanitize=address,undefined.  One sweep of the t recurrences -- b'b, the start, p'q
// and the step length, the update with r'r, the ratio, the new direction, then the true-residual pass, the poisoning of
// broken columns, the closing pass over the still-active columns and k_iter_sum -- on a q the caller supplies (the product itself needs the MFMA), and k_iter_cross_rhs for one
// isotropic and the rational quadratic instantiation.  Every output is compared BIT FOR BIT with the plain loops below in
// the kernels' order of summation: the 16 row classes of a workgroup each in row order, the classes ascending, the
// workgroups ascending.  Exit code 4: a mismatch.  A stand-alone program: the sanitizer is linked in, nothing is preloaded.
#include "host_emul.h"
namespace cugp {
#include "cov_device.h"
#include "iter_device.h"
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
}  // namespace

int main(int argc, char** argv)
{
    // input: ints n tp d count, doubles hd[3 + d + 2] X[n d] Xt[count d] b[n tp] q[n tp] -> output: x r p sc R_se R_rq
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
    ok = check_rhs<false, KERNEL_SE>(X, n, d, Xt, count, tp, hdw, Rs) && ok;
    ok = check_rhs<true, KERNEL_RQ>(X, n, d, Xt, count, tp, hdw, Rq) && ok;
    FILE* o = fopen(argv[2], "wb");
    for (const double* v : {x, r, p}) fwrite(v, 8, cnt, o);
    fwrite(sc, 8, SC_ROWS * IT_MAXT, o);
    fwrite(Rs, 8, cnt, o);
    fwrite(Rq, 8, cnt, o);
    fclose(o);
    for (double* v : {hdw, X, Xt, b, q, x, r, p, part, sc, Rs, Rq, sums}) free(v);
    return ok ? 0 : 4;
}
