// Host check of the inducing-input gradient's kernels (tools/sparse_z_host_check.py builds and runs this; no GPU).  The
// kernels' own text -- cugp_amd/csrc/sparse_z_device.h with cov_device.h and sparse_device.h, the headers kernels.hip
// includes -- runs behind the emulation shim tools/host_emul.h, one workgroup at a time as 256 host threads in lock step:
// k_trace_cross_z<ARD, KIND> over one chunk with the rank-one part (the first pass) and over the square (Z, Z) (the last
// pass), k_trace_cross_z_finish behind each.  Beside them runs a plain double loop in the kernels' summation order -- a
// thread's tiles ascending and its four rows in index order, the four row groups of a wave as (v0 + v1) + (v2 + v3), the
// four waves as (w0 + w1) + (w2 + w3), the slots in index order -- whose results the script compares bit for bit.  Every
// buffer is a heap block of exactly the size the library gives it, so a build with -fsanitize=address,undefined sees any
// access beyond one; the script puts NaN wherever a kernel must not read.  A stand-alone program: the sanitizer is linked
// in, nothing is preloaded.
#include "host_emul.h"
namespace cugp {
#include "cov_device.h"
#include "sparse_device.h"
#include "sparse_z_device.h"
}
using namespace cugp;

struct Pass {
    const double *Xr, *Z, *G, *yv, *bv;
    int nr, m, d, ld, row_tiles, per, ranges;
};

template <bool ARD, int KIND>
static void run(const Pass& p, HyperScalars h, const HyperScalars* hd, double* part)
{
    launch((p.ld / KT) * p.ranges, [&] {
        k_trace_cross_z<ARD, KIND>(p.Xr, p.nr, p.Z, p.m, p.d, p.ld, h, hd, p.G, p.yv, p.bv, p.row_tiles, p.per, p.ranges, part,
                                   (size_t)p.m * p.d);
    });
}

static void run_any(int sel, const Pass& p, HyperScalars h, const HyperScalars* hd, double* part)
{
    if (sel == 0) run<false, 0>(p, h, nullptr, part);
    else if (sel == 1) run<false, 1>(p, h, nullptr, part);
    else if (sel == 2) run<false, 2>(p, h, nullptr, part);
    else if (sel == 3) run<true, 0>(p, h, hd, part);
    else if (sel == 4) run<true, 1>(p, h, hd, part);
    else run<true, 2>(p, h, hd, part);
}

// H of one pair from the (weighted) squared distance, by the entry helpers the kernels call
static double h_entry(int sel, double s, const HyperScalars& h, const DivBy& dl)
{
#pragma clang fp contract(off)
    double kf = 0.0, dk = 0.0, hh = 0.0;
    switch (sel) {
    case 0: kf = h.signal_var * exp(div_by(-s * 0.5, dl)); hh = kf; break;
    case 1: matern_entry<1>(div_by(s, dl), h.signal_var, kf, dk, hh); break;
    case 2: matern_entry<2>(div_by(s, dl), h.signal_var, kf, dk, hh); break;
    case 3: ard_entry<0>(s, h.signal_var, kf, hh); break;
    case 4: ard_entry<1>(s, h.signal_var, kf, hh); break;
    default: ard_entry<2>(s, h.signal_var, kf, hh); break;
    }
    return hh;
}

// the plain loop: part[rg][j][c] in the kernel's order
static void reference(int sel, const Pass& p, const HyperScalars& h, const double* wts, double* part)
{
#pragma clang fp contract(off)
    const DivBy dl = div_prepare(h.ell_sq);
    const int rows = p.row_tiles * KT;
    std::vector<double> E((size_t)rows * p.m, 0.0);                    // w_ij H_ij, exact zeros beyond row nr
    for (int i = 0; i < p.nr; i++)
        for (int j = 0; j < p.m; j++) {
            double s = 0.0;
            for (int c = 0; c < p.d; c++) {
                double df = p.Xr[(size_t)i * p.d + c] - p.Z[(size_t)j * p.d + c];
                if (sel >= 3) df = df * wts[c];
                s = s + df * df;
            }
            const double w = p.G[(size_t)i * p.ld + j] + (p.yv ? p.yv[i] : 0.0) * (p.yv ? p.bv[j] : 0.0);
            E[(size_t)i * p.m + j] = w * h_entry(sel, s, h, dl);
        }
    for (int rg = 0; rg < p.ranges; rg++) {
        const int t0 = rg * p.per, t1 = t0 + p.per < p.row_tiles ? t0 + p.per : p.row_tiles;
        for (int j = 0; j < p.m; j++)
            for (int c = 0; c < p.d; c++) {
                const double z = p.Z[(size_t)j * p.d + c];
                double wv[4];
                for (int w = 0; w < 4; w++) {
                    double v[4];
                    for (int q = 0; q < 4; q++) {
                        const int ty = 4 * w + q;
                        v[q] = 0.0;
                        for (int rt = t0; rt < t1; rt++)
                            for (int a = 0; a < 4; a++) {
                                const int i = rt * KT + ty * 4 + a;
                                const double x = i < p.nr ? p.Xr[(size_t)i * p.d + c] : 0.0;
                                v[q] = v[q] + E[(size_t)i * p.m + j] * (x - z);
                            }
                    }
                    wv[w] = (v[0] + v[1]) + (v[2] + v[3]);
                }
                part[((size_t)rg * p.m + j) * p.d + c] = (wv[0] + wv[1]) + (wv[2] + wv[3]);
            }
    }
}

static void finish_reference(const double* part, size_t md, int nslots, int d, bool first, bool last, double ell_sq,
                             const double* wts, double* acc, double* out)
{
#pragma clang fp contract(off)
    for (size_t e = 0; e < md; e++) {
        double s = first ? 0.0 : acc[e];
        for (int k = 0; k < nslots; k++) s = s + part[(size_t)k * md + e];
        acc[e] = s;
        if (last) out[e] = -((wts ? wts[e % d] * wts[e % d] : 1.0 / ell_sq) * s);
    }
}

int main(int argc, char** argv)
{
    // input: ints nr m d ld rows_pad kind ard ranges_uf ranges_uu, then doubles: ell_sq sf2 sn2 w[d] | Xr[nr*d] Z[m*d]
    //        G[rows_pad*ld] yv[rows_pad] bv[ld] Guu[ld*ld]
    // output, the kernels' and then the plain loop's: part_uf[ranges_uf*m*d] part_uu[ranges_uu*m*d] acc1[m*d] acc2[m*d]
    //        out[m*d]; the kernels' pinned copy hout[m*d] last
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    int hdr[9];
    if (!f || fread(hdr, sizeof(int), 9, f) != 9) return 2;
    const int nr = hdr[0], m = hdr[1], d = hdr[2], ld = hdr[3], rows_pad = hdr[4], kind = hdr[5], ard = hdr[6];
    const int ranges_uf = hdr[7], ranges_uu = hdr[8];
    auto rd = [&](size_t cnt) { double* p = (double*)malloc(cnt * 8 ? cnt * 8 : 8); if (fread(p, 8, cnt, f) != cnt) exit(3); return p; };
    double* hdw = rd(3 + (size_t)d);                       // the hyper-scalars directly followed by the d weights
    const HyperScalars* hd = (const HyperScalars*)hdw;
    const HyperScalars h = *hd;
    const double* wts = ard ? hdw + 3 : nullptr;
    double *Xr = rd((size_t)nr * d), *Z = rd((size_t)m * d), *G = rd((size_t)rows_pad * ld), *yv = rd(rows_pad), *bv = rd(ld);
    double* Guu = rd((size_t)ld * ld);
    fclose(f);
    const int sel = ard * 3 + kind;
    const size_t md = (size_t)m * d;
    auto shape = [](int rows, int ranges) {
        const int tiles = rows / KT, per = (tiles + ranges - 1) / ranges;
        return Pass{nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, 0, 0, tiles, per, (tiles + per - 1) / per};
    };
    Pass uf = shape(rows_pad, ranges_uf), uu = shape(ld, ranges_uu);
    uf.Xr = Xr; uf.Z = Z; uf.G = G; uf.yv = yv; uf.bv = bv; uf.nr = nr; uf.m = m; uf.d = d; uf.ld = ld;
    uu.Xr = Z; uu.Z = Z; uu.G = Guu; uu.nr = m; uu.m = m; uu.d = d; uu.ld = ld;
    auto nan_block = [](size_t cnt) { double* p = (double*)malloc(cnt * 8 ? cnt * 8 : 8); for (size_t i = 0; i < cnt; i++) p[i] = NAN; return p; };
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    double* hout = nan_block(md);
    for (int ref = 0; ref < 2; ref++) {
        double *puf = nan_block(uf.ranges * md), *puu = nan_block(uu.ranges * md);
        double *acc = nan_block(md), *acc1 = nan_block(md), *out = nan_block(md);
        if (!ref) {
            run_any(sel, uf, h, hd, puf);
            launch((int)((md + 255) / 256), [&] { k_trace_cross_z_finish(puf, md, uf.ranges, m, d, 1, 0, h.ell_sq, wts, acc, out, hout); });
            memcpy(acc1, acc, md * 8);
            for (size_t e = 0; e < md; e++)
                if (!std::isnan(out[e]) || !std::isnan(hout[e])) return 4;      // (only the last pass writes the result)
            run_any(sel, uu, h, hd, puu);
            launch((int)((md + 255) / 256), [&] { k_trace_cross_z_finish(puu, md, uu.ranges, m, d, 0, 1, h.ell_sq, wts, acc, out, hout); });
        } else {
            reference(sel, uf, h, wts, puf);
            finish_reference(puf, md, uf.ranges, d, true, false, h.ell_sq, wts, acc, out);
            memcpy(acc1, acc, md * 8);
            reference(sel, uu, h, wts, puu);
            finish_reference(puu, md, uu.ranges, d, false, true, h.ell_sq, wts, acc, out);
        }
        fwrite(puf, 8, uf.ranges * md, o);
        fwrite(puu, 8, uu.ranges * md, o);
        fwrite(acc1, 8, md, o);
        fwrite(acc, 8, md, o);
        fwrite(out, 8, md, o);
        for (double* p : {puf, puu, acc, acc1, out}) free(p);
    }
    fwrite(hout, 8, md, o);
    fclose(o);
    for (double* p : {hdw, Xr, Z, G, yv, bv, Guu, hout}) free(p);
    return 0;
}
