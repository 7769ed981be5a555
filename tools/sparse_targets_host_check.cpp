// Host check of the multi-target sparse-GP kernels (tools/sparse_targets_host_check.py builds and runs this; no GPU).  The
// kernels' own text -- cugp_amd/csrc/sparse_targets_device.h, the header kernels.hip includes -- runs behind the emulation
// shim tools/host_emul.h, one workgroup at a time as 256 host threads in lock step: k_sparse_wty_targets with its finish
// (twice: first, then accumulating), k_sparse_yy_targets, k_sparse_h_targets, k_sparse_weights_targets,
// k_sparse_scale_targets and k_sparse_finalize_targets (with and without the gradient).  Every buffer is a heap block of
// exactly the size the library gives it, so a build with -fsanitize=address,undefined sees any access beyond one; the script
// puts NaN wherever a kernel must not read, and restates every target's slab shares, y_t'y_t and (p = 1) H in the one
// order a target's sums have, bit for bit.  A stand-alone program: the sanitizer is linked in, nothing is preloaded.
#include "host_emul.h"
namespace cugp {
#include "cov_device.h"
#include "sparse_device.h"
#include "sparse_targets_device.h"
}
using namespace cugp;

int main(int argc, char** argv)
{
    // input: ints p m ld nr rows_pad nl nb_uf, then doubles: n sf2 s2 log_s2 | W[rows_pad*ld] (zero padded) Yz[p*rows_pad]
    //        (zero padded) Yn[p*rows_pad] (NaN padded) P[ld*ld] Binv[ld*ld] Cp[p*ld] Gm[p*ld] Bt[p*ld] G[rows_pad*ld]
    //        logdet[ld/128] part_uf[(nl+1)*nb_uf] part_uu[(nl+1)*nb_uu]
    // output: part[p*slabs*ld] Q1[p*ld] Q2[p*ld] yy[p] H[ld*ld] H2[ld*ld] Bs[p*ld] G[rows_pad*ld] Cs[p64*ld] row[1+nh+p]
    //         rowF[1+nh+p]
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    int hdr[7];
    if (!f || fread(hdr, sizeof(int), 7, f) != 7) return 2;
    const int p = hdr[0], m = hdr[1], ld = hdr[2], nr = hdr[3], rows_pad = hdr[4], nl = hdr[5], nb_uf = hdr[6];
    auto rd = [&](size_t cnt) { double* q = (double*)malloc(cnt * 8 ? cnt * 8 : 8); if (fread(q, 8, cnt, f) != cnt) exit(3); return q; };
    auto nan_block = [](size_t cnt) { double* q = (double*)malloc(cnt * 8 ? cnt * 8 : 8); for (size_t i = 0; i < cnt; i++) q[i] = NAN; return q; };
    double* sc = rd(4);
    const double s2 = sc[2];
    const size_t ll = (size_t)ld * ld, pl = (size_t)p * ld, cl = (size_t)rows_pad * ld, ys = (size_t)rows_pad;
    const int slabs = rows_pad / TILE, nb_uu = (ld / KT) * (ld / KT), ntl = ld / TILE, nh = nl + 2, p64 = (p + 63) / 64 * 64;
    double *W = rd(cl), *Yz = rd(p * ys), *Yn = rd(p * ys), *P = rd(ll), *Binv = rd(ll), *Cp = rd(pl), *Gm = rd(pl), *Bt = rd(pl);
    double *G = rd(cl), *logdet = rd(ntl), *part_uf = rd((size_t)(nl + 1) * nb_uf), *part_uu = rd((size_t)(nl + 1) * nb_uu);
    fclose(f);

    // Q: the slabs' shares, then the sums -- first, and once more on top of them
    const int groups = (p + SPT_GROUP - 1) / SPT_GROUP;
    double *part = nan_block((size_t)p * slabs * ld), *Q1 = nan_block(pl), *Q2 = nan_block(pl);
    launch((ld / KT) * slabs * groups, [&] { k_sparse_wty_targets(W, ld, slabs, Yz, ys, p, part); });
    launch(p * ((ld + 255) / 256), [&] { k_sparse_wty_targets_finish(part, slabs, ld, p, Q1, 1); });
    memcpy(Q2, Q1, pl * 8);
    launch(p * ((ld + 255) / 256), [&] { k_sparse_wty_targets_finish(part, slabs, ld, p, Q2, 0); });
    double* yy = nan_block(p);
    launch(p, [&] { k_sparse_yy_targets(Yn, ys, nr, yy); });
    double *H = nan_block(ll), *H2 = nan_block(ll), *Bs = nan_block(pl);
    launch(nb_uu, [&] { k_sparse_h_targets(Binv, P, Gm, Bt, p, m, ld, s2, H, H2, Bs); });
    // the weights in place: Bs as the library holds it (zero beyond m) is what k_sparse_h_targets just wrote; the check
    // hands over a copy with NaN beyond m, which the kernel must not read
    double* Bn = (double*)malloc(pl * 8);
    for (size_t e = 0; e < pl; e++) Bn[e] = (int)(e % ld) < m ? Bs[e] : NAN;
    launch((rows_pad / KT) * (ld / KT), [&] { k_sparse_weights_targets(G, ld, Yn, ys, Bn, p, nr, m); });
    double* Cs = nan_block((size_t)p64 * ld);
    launch(3, [&] { k_sparse_scale_targets(Cp, p, p64, m, ld, s2, Cs); });
    double *row = nan_block(1 + nh + p), *hrow = nan_block(1 + nh + p), *rowF = nan_block(1 + nh + p), *hrowF = nan_block(1 + nh + p);
    const SparseFinalTargets fin{P, Binv, Cp, Gm, logdet, yy, m, ld, ntl, p, sc[0], sc[1], s2, sc[3]};
    launch(1, [&] { k_sparse_finalize_targets(fin, part_uf, nb_uf, part_uu, nb_uu, nl, row, hrow); });
    launch(1, [&] { k_sparse_finalize_targets(fin, nullptr, 0, nullptr, 0, nl, rowF, hrowF); });
    if (memcmp(row, hrow, (size_t)(1 + nh + p) * 8) != 0) return 4;       // the device row and its pinned copy
    if (memcmp(rowF, hrowF, (size_t)(1 + nh + p) * 8) != 0) return 4;
    if (memcmp(rowF, row, 8) != 0 || memcmp(rowF + 1 + nh, row + 1 + nh, (size_t)p * 8) != 0) return 4;   // F and F_t without the gradient

    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    fwrite(part, 8, (size_t)p * slabs * ld, o);
    fwrite(Q1, 8, pl, o);
    fwrite(Q2, 8, pl, o);
    fwrite(yy, 8, p, o);
    fwrite(H, 8, ll, o);
    fwrite(H2, 8, ll, o);
    fwrite(Bs, 8, pl, o);
    fwrite(G, 8, cl, o);
    fwrite(Cs, 8, (size_t)p64 * ld, o);
    fwrite(row, 8, 1 + nh + p, o);
    fwrite(rowF, 8, 1 + nh + p, o);
    fclose(o);
    for (double* q : {sc, W, Yz, Yn, P, Binv, Cp, Gm, Bt, G, logdet, part_uf, part_uu, part, Q1, Q2, yy, H, H2, Bs, Bn, Cs,
                      row, hrow, rowF, hrowF})
        free(q);
    return 0;
}
