// Host check of the k_predict_grad family (tools/predict_grad_host_check.py builds and runs this; no GPU).
// The kernels' own text -- cugp_amd/csrc/cov_device.h, the header kernels.hip includes -- runs behind the emulation shim
// tools/host_emul.h, one workgroup at a time as 256 host threads in lock step.
// Every buffer is a heap block of exactly the size the library gives it, so a build with -fsanitize=address,undefined sees
// any read or write beyond one; the script poisons all padding of Ks, V and alpha with NaN, so a missing mask shows in
// the results.  A stand-alone program: the sanitizer is linked in, nothing is preloaded.
#include "host_emul.h"
namespace cugp {
#include "cov_device.h"
}
using namespace cugp;

int main(int argc, char** argv)
{
    // input file: ints n d npad nt cpad kind wantV ard, then doubles: ell_sq sf2, X[n*d], Xt[nt*d], Ks[cpad*npad], V[cpad*npad], alpha[npad], w[d]
    FILE* f = fopen(argv[1], "rb");
    int hdr[8];
    if (fread(hdr, sizeof(int), 8, f) != 8) return 2;
    const int n = hdr[0], d = hdr[1], npad = hdr[2], nt = hdr[3], cpad = hdr[4], kind = hdr[5], wantV = hdr[6], ard = hdr[7];
    double hs[2];
    if (fread(hs, 8, 2, f) != 2) return 2;
    auto rd = [&](size_t cnt) { double* p = (double*)malloc(cnt * 8 ? cnt * 8 : 8); if (fread(p, 8, cnt, f) != cnt) exit(3); return p; };
    // exact-size heap blocks: AddressSanitizer sees any read or write beyond them
    double *X = rd((size_t)n * d), *Xt = rd((size_t)nt * d), *Ks = rd((size_t)cpad * npad), *V = rd((size_t)cpad * npad);
    double *alpha = rd(npad), *w = rd(d);
    fclose(f);
    const int tiles = (n + 63) / 64;
    const size_t pstride = (size_t)nt * d;
    double* part = (double*)malloc(tiles * 2 * pstride * 8);
    for (size_t i = 0; i < tiles * 2 * pstride; i++) part[i] = NAN;
    HyperScalars h{hs[0], hs[1], 0.0};
    const double* Vp = wantV ? V : nullptr;
    const int blocks = ((nt + 63) / 64) * tiles;
    if (kind == 0) launch(blocks, [&] { k_predict_grad<false, 0>(X, n, d, npad, Xt, nt, h, Ks, Vp, alpha, part, pstride, nullptr); });
    else if (kind == 1) launch(blocks, [&] { k_predict_grad<false, 1>(X, n, d, npad, Xt, nt, h, Ks, Vp, alpha, part, pstride, nullptr); });
    else launch(blocks, [&] { k_predict_grad<false, 2>(X, n, d, npad, Xt, nt, h, Ks, Vp, alpha, part, pstride, nullptr); });
    double* dm = (double*)malloc(pstride * 8);
    double* dv = (double*)malloc(pstride * 8);
    const int fblocks = (int)((pstride + 255) / 256);
    for (int b = 0; b < fblocks; b++)
        for (int t = 0; t < 256; t++) {
            blockIdx.x = b; threadIdx.x = t;
            k_predict_grad_finish(part, pstride, tiles, nt, d, h.ell_sq, ard ? w : nullptr, dm, wantV ? dv : nullptr);
        }
    FILE* o = fopen(argv[2], "wb");
    fwrite(dm, 8, pstride, o);
    if (wantV) fwrite(dv, 8, pstride, o);
    fclose(o);
    return 0;
}
