// Host check of the sparse-GP kernels (tools/sparse_host_check.py builds and runs this; no GPU).  The kernels' own text --
// cugp_amd/csrc/sparse_device.h and sparse_targets_device.h with cov_device.h, the headers kernels.hip includes -- runs
// behind the emulation shim tools/host_emul.h, one workgroup at a time as 256 host threads in lock step: the rectangular
// gradient pass k_trace_cross<ARD, KIND> over one chunk (with the rank-one part, its partials behind an offset of 3
// blocks) and over the square (Z, Z), and as the handle's own y runs them, with p = 1: k_sparse_finalize_targets on both
// and the small passes around the products (k_sparse_gram_finish, k_sparse_form_b, k_sparse_wty_targets with its finish,
// k_sparse_yy_targets, k_sparse_h_targets, k_sparse_transpose, k_sparse_predict_finish).
// The MFMA product k_sparse_gram is not emulated: its partial tiles are an input.  Every buffer is a heap block of exactly
// the size the library gives it, so a build with -fsanitize=address,undefined sees any access beyond one; the script puts
// NaN wherever a kernel must not read.  A stand-alone program: the sanitizer is linked in, nothing is preloaded.
#include "host_emul.h"
namespace cugp {
#include "cov_device.h"
#include "sparse_device.h"
#include "sparse_targets_device.h"
}
using namespace cugp;

template <bool ARD, int KIND>
static void trace(int nb, const double* Xr, int nr, const double* Z, int m, int d, int ld, HyperScalars h,
                  const HyperScalars* hd, const double* G, const double* yv, const double* bv, double* part, size_t pstride,
                  size_t pofs)
{
    launch(nb, [&] { k_trace_cross<ARD, KIND>(Xr, nr, Z, m, d, ld, h, hd, G, yv, bv, part, pstride, pofs); });
}

static void trace_any(int sel, int nb, const double* Xr, int nr, const double* Z, int m, int d, int ld, HyperScalars h,
                      const HyperScalars* hd, const double* G, const double* yv, const double* bv, double* part,
                      size_t pstride, size_t pofs)
{
    if (sel == 0) trace<false, 0>(nb, Xr, nr, Z, m, d, ld, h, nullptr, G, yv, bv, part, pstride, pofs);
    else if (sel == 1) trace<false, 1>(nb, Xr, nr, Z, m, d, ld, h, nullptr, G, yv, bv, part, pstride, pofs);
    else if (sel == 2) trace<false, 2>(nb, Xr, nr, Z, m, d, ld, h, nullptr, G, yv, bv, part, pstride, pofs);
    else if (sel == 3) trace<true, 0>(nb, Xr, nr, Z, m, d, ld, h, hd, G, yv, bv, part, pstride, pofs);
    else if (sel == 4) trace<true, 1>(nb, Xr, nr, Z, m, d, ld, h, hd, G, yv, bv, part, pstride, pofs);
    else trace<true, 2>(nb, Xr, nr, Z, m, d, ld, h, hd, G, yv, bv, part, pstride, pofs);
}

int main(int argc, char** argv)
{
    // input: ints nr m d ld rows_pad kind ard nscr, then doubles: ell_sq sf2 sn2 w[d] | n s2 log_s2 yy | Xr[nr*d] Z[m*d]
    //        G[rows_pad*ld] yv[rows_pad] bv[ld] Guu[ld*ld] P[ld*ld] Binv[ld*ld] cp[ld] gp[ld] bp[ld] logdet[ld/128]
    //        scr[nscr*ld*ld]
    // output: part_uf[(nl+1)*(nb_uf+3)] part_uu[(nl+1)*nb_uu] row[1+nh] (its F_1 slot is compared here) rowF[1] Pacc[ld*ld] Bm[ld*ld] q[ld] yy[1] H[ld*ld]
    //         H2[ld*ld] bsc[ld] Gt[ld*ld] mean[nr] var[nr]
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    int hdr[8];
    if (!f || fread(hdr, sizeof(int), 8, f) != 8) return 2;
    const int nr = hdr[0], m = hdr[1], d = hdr[2], ld = hdr[3], rows_pad = hdr[4], kind = hdr[5], ard = hdr[6], nscr = hdr[7];
    auto rd = [&](size_t cnt) { double* p = (double*)malloc(cnt * 8 ? cnt * 8 : 8); if (fread(p, 8, cnt, f) != cnt) exit(3); return p; };
    double* hdw = rd(3 + (size_t)d);                       // the hyper-scalars directly followed by the d weights
    const HyperScalars* hd = (const HyperScalars*)hdw;
    const HyperScalars h = *hd;
    double* sc = rd(4);
    const size_t ll = (size_t)ld * ld;
    double *Xr = rd((size_t)nr * d), *Z = rd((size_t)m * d), *G = rd((size_t)rows_pad * ld), *yv = rd(rows_pad), *bv = rd(ld);
    double *Guu = rd(ll), *P = rd(ll), *Binv = rd(ll), *cp = rd(ld), *gp = rd(ld), *bp = rd(ld), *logdet = rd(ld / TILE);
    double* scr = rd((size_t)nscr * ll);
    fclose(f);
    const int nl = ard ? d : 1, nh = nl + 2, sel = ard * 3 + kind;
    const int nb_uf = (rows_pad / KT) * (ld / KT), nb_uu = (ld / KT) * (ld / KT), ntl = ld / TILE, tiles = ntl * (ntl + 1) / 2;
    const size_t ps_uf = (size_t)nb_uf + 3;
    auto nan_block = [](size_t cnt) { double* p = (double*)malloc(cnt * 8 ? cnt * 8 : 8); for (size_t i = 0; i < cnt; i++) p[i] = NAN; return p; };
    double *part_uf = nan_block((size_t)(nl + 1) * ps_uf), *part_uu = nan_block((size_t)(nl + 1) * nb_uu);
    double *row = nan_block(2 + nh), *hrow = nan_block(2 + nh), *rowF = nan_block(2 + nh), *hrowF = nan_block(2 + nh);

    trace_any(sel, nb_uf, Xr, nr, Z, m, d, ld, h, hd, G, yv, bv, part_uf, ps_uf, 3);
    trace_any(sel, nb_uu, Z, m, Z, m, d, ld, h, hd, Guu, nullptr, nullptr, part_uu, nb_uu, 0);
    const SparseFinalTargets fin{P, Binv, cp, gp, logdet, sc + 3, m, ld, ntl, 1, sc[0], h.signal_var, sc[1], sc[2]};
    // (the finalize of the check sums the rectangle's blocks behind the offset: its columns start 3 entries in)
    double* uf = nan_block((size_t)(nl + 1) * nb_uf);
    for (int c = 0; c <= nl; c++) memcpy(uf + (size_t)c * nb_uf, part_uf + (size_t)c * ps_uf + 3, (size_t)nb_uf * 8);
    launch(1, [&] { k_sparse_finalize_targets(fin, uf, nb_uf, part_uu, nb_uu, nl, row, hrow); });
    launch(1, [&] { k_sparse_finalize_targets(fin, nullptr, 0, nullptr, 0, nl, rowF, hrowF); });
    for (int i = 0; i < 2 + nh; i++)
        if (memcmp(&row[i], &hrow[i], 8) != 0) return 4;  // the device row and its pinned copy carry the same bits
    if (memcmp(&rowF[0], &hrowF[0], 8) != 0 || memcmp(&rowF[0], &row[0], 8) != 0) return 4;
    if (memcmp(&row[1 + nh], &row[0], 8) != 0 || memcmp(&rowF[1 + nh], &row[0], 8) != 0) return 4;   // F_1, the one target's share, is F

    double *Pacc = (double*)malloc(ll * 8), *Bm = nan_block(ll), *q = nan_block(ld), *qpart = nan_block((size_t)(rows_pad / TILE) * ld);
    memcpy(Pacc, P, ll * 8);
    launch(tiles * 16, [&] { k_sparse_gram_finish(Pacc, ld, scr, ll, nscr, 0); });
    launch(tiles * 16, [&] { k_sparse_form_b(P, ld, sc[1], Bm); });
    // W and y as the library holds them: exact zeros beyond the chunk's rows and beyond column m (the script's NaN there
    // is for the passes that must mask)
    double *Wz = (double*)malloc((size_t)rows_pad * ld * 8), *yz = (double*)malloc((size_t)rows_pad * 8);
    for (size_t i = 0; i < (size_t)rows_pad * ld; i++) Wz[i] = std::isnan(G[i]) ? 0.0 : G[i];
    for (int i = 0; i < rows_pad; i++) yz[i] = std::isnan(yv[i]) ? 0.0 : yv[i];
    launch((ld / KT) * (rows_pad / TILE), [&] { k_sparse_wty_targets(Wz, ld, rows_pad / TILE, yz, (size_t)rows_pad, 1, qpart); });
    launch((ld + 255) / 256, [&] { k_sparse_wty_targets_finish(qpart, rows_pad / TILE, ld, 1, q, 1); });
    double* yy = nan_block(1);
    launch(1, [&] { k_sparse_yy_targets(yv, (size_t)rows_pad, nr, yy); });
    double *H = nan_block(ll), *H2 = nan_block(ll), *bsc = nan_block(ld), *Gt = nan_block(ll);
    launch(nb_uu, [&] { k_sparse_h_targets(Binv, P, gp, bp, 1, m, ld, sc[1], H, H2, bsc); });
    launch(nb_uu, [&] { k_sparse_transpose(Guu, Gt, ld, 0.5); });
    double *mean = nan_block(nr), *var = nan_block(nr);
    launch((nr + 3) / 4, [&] { k_sparse_predict_finish(Wz, Wz, cp, ld, nr, h.signal_var, sc[1], sc[1], mean, var); });

    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    fwrite(part_uf, 8, (size_t)(nl + 1) * ps_uf, o);
    fwrite(part_uu, 8, (size_t)(nl + 1) * nb_uu, o);
    fwrite(row, 8, 1 + nh, o);
    fwrite(rowF, 8, 1, o);
    fwrite(Pacc, 8, ll, o);
    fwrite(Bm, 8, ll, o);
    fwrite(q, 8, ld, o);
    fwrite(yy, 8, 1, o);
    fwrite(H, 8, ll, o);
    fwrite(H2, 8, ll, o);
    fwrite(bsc, 8, ld, o);
    fwrite(Gt, 8, ll, o);
    fwrite(mean, 8, nr, o);
    fwrite(var, 8, nr, o);
    fclose(o);
    for (double* p : {hdw, sc, Xr, Z, G, yv, bv, Guu, P, Binv, cp, gp, bp, logdet, scr, part_uf, part_uu, row, hrow, rowF, hrowF, uf,
                      Pacc, Bm, q, qpart, Wz, yz, yy, H, H2, bsc, Gt, mean, var})
        free(p);
    return 0;
}
