// Host check of the leave-one-out kernels (tools/loo_host_check.py builds and runs this; no GPU).  The kernels' own text --
// cugp_amd/csrc/loo_device.h with cov_device.h, the headers kernels.hip includes -- runs behind the emulation shim
// tools/host_emul.h, one workgroup at a time as 256 host threads in lock step, in the order cugp_loo launches them; the one
// pass that needs the device, k_loo_product, is a plain loop here (lower 128-tiles of P, diagonal tiles complete, NaN
// elsewhere).  Every buffer is a heap block of exactly the size the library gives it, so a build with
// -fsanitize=address,undefined sees any read or write beyond one; the script poisons the padding and the strict upper
// triangle of K^-1 and the padding of alpha and y with NaN, so a missing mask shows in the results.  A stand-alone
// program: the sanitizer is linked in, nothing is preloaded.
#include "host_emul.h"
namespace cugp {
#include "cov_device.h"
#include "loo_device.h"
}
using namespace cugp;

template <bool ARD, int KIND>
static void trace(int nb, const double* X, int n, int d, int npad, HyperScalars h, const HyperScalars* hd, const double* P,
                  const double* alpha, const double* b, double* part)
{
    launch(nb, [&] { k_trace_loo<ARD, KIND>(X, n, d, npad, h, hd, P, alpha, b, part); });
}

int main(int argc, char** argv)
{
    // input: ints n d npad kind ard, then doubles: ell_sq sf2 sn2 w[d] X[n*d] Kinv[npad*npad] alpha[npad] y[npad]
    // output: pt[5*npad] b[npad] row[1 + nh] B[npad*npad]
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    int hdr[5];
    if (!f || fread(hdr, sizeof(int), 5, f) != 5) return 2;
    const int n = hdr[0], d = hdr[1], npad = hdr[2], kind = hdr[3], ard = hdr[4];
    auto rd = [&](size_t cnt) { double* p = (double*)malloc(cnt * 8 ? cnt * 8 : 8); if (fread(p, 8, cnt, f) != cnt) exit(3); return p; };
    double* hdw = rd(3 + (size_t)d);                       // the hyper-scalars directly followed by the d weights
    const HyperScalars* hd = (const HyperScalars*)hdw;
    const HyperScalars h = *hd;
    double *X = rd((size_t)n * d), *Kinv = rd((size_t)npad * npad), *alpha = rd(npad), *y = rd(npad);
    fclose(f);
    const int nl = ard ? d : 1, nh = nl + 2;
    const int nb = (npad / KT) * (npad / KT + 1) / 2, nt = npad / TILE;
    const size_t nn = (size_t)npad * npad;
    auto nan_block = [](size_t cnt) { double* p = (double*)malloc(cnt * 8); for (size_t i = 0; i < cnt; i++) p[i] = NAN; return p; };
    double *pt = nan_block((size_t)LOO_ROWS * npad), *b = nan_block(npad), *bpart = nan_block((size_t)(npad / KT) * npad);
    double *part = nan_block((size_t)nh * nb), *row = nan_block(1 + nh), *hrow = nan_block(1 + nh);
    double *B = nan_block(nn), *P = nan_block(nn);

    launch((npad + 255) / 256, [&] { k_loo_point(Kinv, alpha, y, n, npad, pt); });
    launch(1, [&] { k_loo_sum(pt, npad, row, hrow); });
    launch((npad / KT) * (npad / KT), [&] { k_loo_mirror_scale(Kinv, pt, n, npad, B, bpart); });
    launch((npad + 255) / 256, [&] { k_loo_bsum(bpart, npad, b); });
    for (int ti = 0; ti < nt; ti++)                        // the stand-in of k_loo_product
        for (int tj = 0; tj <= ti; tj++)
            for (int i = ti * TILE; i < (ti + 1) * TILE; i++)
                for (int j = tj * TILE; j < (tj + 1) * TILE; j++) {
                    double s = 0.0;
                    for (int k = 0; k < npad; k++) s += B[(size_t)i * npad + k] * B[(size_t)j * npad + k];
                    P[(size_t)i * npad + j] = s;
                }
    const int sel = ard * 3 + kind;
    if (sel == 0) trace<false, 0>(nb, X, n, d, npad, h, nullptr, P, alpha, b, part);
    else if (sel == 1) trace<false, 1>(nb, X, n, d, npad, h, nullptr, P, alpha, b, part);
    else if (sel == 2) trace<false, 2>(nb, X, n, d, npad, h, nullptr, P, alpha, b, part);
    else if (sel == 3) trace<true, 0>(nb, X, n, d, npad, h, hd, P, alpha, b, part);
    else if (sel == 4) trace<true, 1>(nb, X, n, d, npad, h, hd, P, alpha, b, part);
    else trace<true, 2>(nb, X, n, d, npad, h, hd, P, alpha, b, part);
    launch(1, [&] { k_loo_finalize(part, nb, nl, h.noise_var, row, hrow); });
    for (int i = 0; i < 1 + nh; i++)
        if (memcmp(&row[i], &hrow[i], 8) != 0) return 4;  // the device row and its pinned copy carry the same bits

    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    fwrite(pt, 8, (size_t)LOO_ROWS * npad, o);
    fwrite(b, 8, npad, o);
    fwrite(row, 8, 1 + nh, o);
    fwrite(B, 8, nn, o);
    fclose(o);
    free(hdw); free(X); free(Kinv); free(alpha); free(y); free(pt); free(b); free(bpart); free(part); free(row); free(hrow);
    free(B); free(P);
    return 0;
}
