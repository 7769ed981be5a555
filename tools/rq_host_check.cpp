// Host check of the rational quadratic instantiations of the ARD gradient pass -- trace_ard_body<KERNEL_RQ, false>
// (k_trace<true, RQ>), trace_ard_body<KERNEL_RQ, true> (k_trace_targets<true, RQ>) -- and of k_predict_grad<true, RQ>
// (tools/rq_host_check.py builds and runs this; no GPU).  The kernels' own text, cugp_amd/csrc/cov_device.h, runs behind the
// emulation shim tools/host_emul.h, one workgroup at a time as 256 host threads in lock step, on heap blocks of exactly the
// size the library gives them: a build with -fsanitize=address,undefined sees any access beyond one, and the script puts
// NaN where the kernels must not read.  The results are compared BIT FOR BIT with the plain loops below, which restate
// the passes entry by entry in the kernels' order of summation: a thread's 4 x 4 entries row by row, the 64 lanes of a
// wave by the halving tree of wave_sum (predict-grad: the 16 lanes of a row by the xor butterfly), the four waves as
// (w0 + w1) + (w2 + w3), the tiles of the input gradient in tile order.  Exit code 4: a mismatch (the first one is printed).
// The plain loops call the header's own rq_entry for the entry: what is compared bit for bit is the order of summation,
// the masking and the indexing of the passes, NOT the entry's arithmetic -- that is checked by tools/rq_host_check.py against
// fp64 numpy (1e-12 of the sum of the terms' absolute values) and by tests/truth_rq.py's entry_fp64 against longdouble.
// A stand-alone program: the sanitizer is linked in, nothing is preloaded.
#include "host_emul.h"
namespace cugp {
#include "cov_device.h"
}
using namespace cugp;

namespace {
#pragma clang fp contract(off)
// the weighted squared distance of rows xa, xb in sqdist_4x4<true>'s order
double wdist(const double* xa, const double* xb, const double* w, int d)
{
    double acc = 0.0;
    for (int c = 0; c < d; c++) {
        double df = xa[c] - xb[c];
        df = df * w[c];
        acc = acc + df * df;
    }
    return acc;
}
double tree64(double* v)                                   // wave_sum: v[l] += v[l + o], o = 32 .. 1; lane 0 holds the sum
{
    for (int o = 32; o > 0; o >>= 1)
        for (int l = 0; l + o < 64; l++) v[l] = v[l] + v[l + o];   // (ascending l: v[l + o] is still the previous level's)
    return v[0];
}
double four(const double* r) { return (r[0] + r[1]) + (r[2] + r[3]); }

// one lower 64 x 64 tile of the gradient pass -> column c of part at [c * nb + blk]
void ref_trace_tile(int blk, int nb, const double* X, int n, int d, int npad, const double* hdw, const double* Kinv,
                    const double* AV, int m, bool targets, double* part)
{
    const double sf2 = hdw[1], sn2 = hdw[2], *w = hdw + 3, alpha = w[d], h2a = w[d + 1];
    int ti, tj;
    tri_index(blk, ti, tj);
    const int i0 = ti * KT, j0 = tj * KT;
    static thread_local double e[256][4][4];
    double t2[256], t3[256], t4[256];
    const double zero[64] = {};
    for (int t = 0; t < 256; t++) {
        const int tx = t & 15, ty = t >> 4;
        double s2 = 0.0, s3 = 0.0, s4 = 0.0;
        for (int a = 0; a < 4; a++)
            for (int b = 0; b < 4; b++) {
                const int i = i0 + ty * 4 + a, j = j0 + col4(tx, b);
                double ev = 0.0;
                if (i < n && j < n && (ti != tj || j <= i)) {
                    double wv;
                    if (targets) {
                        double S = 0.0;
                        for (int q = 0; q < m; q++) S = S + AV[(size_t)q * npad + i] * AV[(size_t)q * npad + j];
                        wv = (double)m * Kinv[(size_t)i * npad + j] - S;
                    } else {
                        wv = Kinv[(size_t)i * npad + j] - AV[i] * AV[j];
                    }
                    double kf, hh, da;
                    rq_entry(wdist(X + (size_t)i * d, X + (size_t)j * d, w, d), sf2, alpha, h2a, kf, hh, da);
                    if (i != j) s4 += 2.0 * (wv * da);
                    if (i == j) {
                        kf += sn2;
                        s2 += wv * kf;
                        s3 += wv;
                    } else {
                        ev = 2.0 * (wv * hh);
                        s2 += 2.0 * (wv * kf);
                    }
                }
                e[t][a][b] = ev;
            }
        t2[t] = s2; t3[t] = s3; t4[t] = s4;
    }
    double r2[4], r3[4], r4[4];
    for (int wv = 0; wv < 4; wv++) { r2[wv] = tree64(t2 + 64 * wv); r3[wv] = tree64(t3 + 64 * wv); r4[wv] = tree64(t4 + 64 * wv); }
    part[(size_t)(d + 1) * nb + blk] = four(r2);
    part[(size_t)(d + 2) * nb + blk] = four(r3);
    part[(size_t)d * nb + blk] = four(r4);
    for (int c = 0; c < d; c++) {
        double tc[256];
        for (int t = 0; t < 256; t++) {
            const int tx = t & 15, ty = t >> 4;
            double acc = 0.0;
            for (int a = 0; a < 4; a++)
                for (int b = 0; b < 4; b++) {
                    const int i = i0 + ty * 4 + a, j = j0 + col4(tx, b);
                    const double xi = i < n ? X[(size_t)i * d + c] : 0.0, xj = j < n ? X[(size_t)j * d + c] : 0.0;
                    const double df = (xi - xj) * w[c];
                    acc = acc + e[t][a][b] * (df * df);
                }
            tc[t] = acc;
        }
        double r[4];
        for (int wv = 0; wv < 4; wv++) r[wv] = tree64(tc + 64 * wv);
        part[(size_t)c * nb + blk] = four(r);
    }
    (void)zero;
}

// the input gradient: dmean / dvar [nt][d] from the tiles' partial sums in tile order
void ref_predict_grad(const double* X, int n, int d, int npad, const double* Xt, int nt, const double* hdw, const double* V,
                      const double* alv, double* dm, double* dv)
{
    const double sf2 = hdw[1], *w = hdw + 3, alpha = w[d], h2a = w[d + 1];
    const int tiles = (n + KT - 1) / KT;
    for (int tr = 0; tr < nt; tr++)
        for (int c = 0; c < d; c++) {
            double sm = 0.0, sv = 0.0;
            for (int ti = 0; ti < tiles; ti++) {
                double pm[16], pv[16];
                for (int tx = 0; tx < 16; tx++) {
                    pm[tx] = 0.0; pv[tx] = 0.0;
                    for (int b = 0; b < 4; b++) {
                        const int i = ti * KT + col4(tx, b);
                        double ga = 0.0, gv = 0.0, df = Xt[(size_t)tr * d + c];
                        if (i < n) {
                            double kf, hh, da;
                            rq_entry(wdist(Xt + (size_t)tr * d, X + (size_t)i * d, w, d), sf2, alpha, h2a, kf, hh, da);
                            ga = hh * alv[i];
                            gv = V ? hh * V[(size_t)tr * npad + i] : 0.0;
                            df = Xt[(size_t)tr * d + c] - X[(size_t)i * d + c];
                        }
                        pm[tx] = pm[tx] + ga * df;
                        pv[tx] = pv[tx] + gv * df;
                    }
                }
                for (int msk = 1; msk < 16; msk <<= 1) {
                    double qm[16], qv[16];
                    for (int l = 0; l < 16; l++) { qm[l] = pm[l] + pm[l ^ msk]; qv[l] = pv[l] + pv[l ^ msk]; }
                    for (int l = 0; l < 16; l++) { pm[l] = qm[l]; pv[l] = qv[l]; }
                }
                if (ti == 0) { sm = pm[c & 15]; sv = pv[c & 15]; }
                else { sm = sm + pm[c & 15]; sv = sv + pv[c & 15]; }
            }
            const double sc = w[c] * w[c];
            dm[(size_t)tr * d + c] = -(sc * sm);
            if (dv) dv[(size_t)tr * d + c] = (2.0 * sc) * sv;
        }
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
}  // namespace

int main(int argc, char** argv)
{
    // input file: ints mode (0 trace, 1 trace over m targets, 2 predict-grad) n d npad nt cpad m wantV, then doubles:
    //   sf2 sn2 w[d] alpha h2a X[n*d], and
    //   trace:         Kinv[npad*npad] alpha_vec[npad] | A[m*npad]     -> part[(d + 3) * nblocks]
    //   predict-grad:  Xt[nt*d] V[cpad*npad] alpha_vec[npad]           -> dmean[nt*d] (dvar[nt*d])
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    int hdr[8];
    if (!f || fread(hdr, sizeof(int), 8, f) != 8) return 2;
    const int mode = hdr[0], n = hdr[1], d = hdr[2], npad = hdr[3], nt = hdr[4], cpad = hdr[5], m = hdr[6], wantV = hdr[7];
    auto rd = [&](size_t cnt) { double* p = (double*)malloc(cnt * 8 ? cnt * 8 : 8); if (fread(p, 8, cnt, f) != cnt) exit(3); return p; };
    // hd: the hyper-scalars directly followed by the d weights and by alpha, 0.5 / alpha -- the handle's staging area, exact size
    double* hs = rd(2);
    double* hdw = (double*)malloc((3 + d + 2) * 8);
    hdw[0] = NAN; hdw[1] = hs[0]; hdw[2] = hs[1];                   // (ell_sq is never read: NaN)
    if (fread(hdw + 3, 8, d + 2, f) != (size_t)d + 2) return 3;
    const HyperScalars* hd = (const HyperScalars*)hdw;
    double* X = rd((size_t)n * d);
    bool ok = true;
    FILE* o = nullptr;
    if (mode == 0 || mode == 1) {
        double *Kinv = rd((size_t)npad * npad), *AV = rd(mode == 1 ? (size_t)m * npad : (size_t)npad);
        fclose(f);
        const int nb = (npad / KT) * (npad / KT + 1) / 2;
        const size_t np = (size_t)(d + 3) * nb;
        double *part = (double*)malloc(np * 8), *ref = (double*)malloc(np * 8);
        for (size_t i = 0; i < np; i++) part[i] = ref[i] = NAN;
        if (mode == 0) launch(nb, [&] { trace_ard_body<KERNEL_RQ, false>(X, n, d, npad, hd, Kinv, AV, 1, part, nullptr); });
        else launch(nb, [&] { trace_ard_body<KERNEL_RQ, true>(X, n, d, npad, hd, Kinv, AV, m, part, nullptr); });
        for (int b = 0; b < nb; b++) ref_trace_tile(b, nb, X, n, d, npad, hdw, Kinv, AV, m, mode == 1, ref);
        ok = same_bits(part, ref, np, "part");
        o = fopen(argv[2], "wb");
        fwrite(part, 8, np, o);
        free(part); free(ref); free(Kinv); free(AV);
    } else {
        double *Xt = rd((size_t)nt * d), *V = rd((size_t)cpad * npad), *alv = rd(npad);
        fclose(f);
        const int tiles = (n + 63) / 64;
        const size_t pstride = (size_t)nt * d;
        double* part = (double*)malloc(tiles * 2 * pstride * 8);
        for (size_t i = 0; i < tiles * 2 * pstride; i++) part[i] = NAN;
        const double* Vp = wantV ? V : nullptr;
        const int blocks = ((nt + 63) / 64) * tiles;
        launch(blocks, [&] { k_predict_grad<true, KERNEL_RQ>(X, n, d, npad, Xt, nt, HyperScalars{}, nullptr, Vp, alv, part, pstride, hd); });
        double *dm = (double*)malloc(pstride * 8), *dv = (double*)malloc(pstride * 8);
        double *rm = (double*)malloc(pstride * 8), *rv = (double*)malloc(pstride * 8);
        const int fblocks = (int)((pstride + 255) / 256);
        for (int b = 0; b < fblocks; b++)
            for (int t = 0; t < 256; t++) {
                blockIdx.x = b; threadIdx.x = t;
                k_predict_grad_finish(part, pstride, tiles, nt, d, NAN, hdw + 3, dm, wantV ? dv : nullptr);
            }
        ref_predict_grad(X, n, d, npad, Xt, nt, hdw, Vp, alv, rm, wantV ? rv : nullptr);
        ok = same_bits(dm, rm, pstride, "dmean") && (!wantV || same_bits(dv, rv, pstride, "dvar"));
        o = fopen(argv[2], "wb");
        fwrite(dm, 8, pstride, o);
        if (wantV) fwrite(dv, 8, pstride, o);
        free(part); free(dm); free(dv); free(rm); free(rv); free(Xt); free(V); free(alv);
    }
    fclose(o);
    free(hs); free(hdw); free(X);
    return ok ? 0 : 4;
}
