// Host check of trace_ard_body<KIND, false> (k_trace<true, KIND>) and k_predict_grad<true, KIND> (tools/ard_matern_host_check.py builds and runs this; no
// GPU).  The kernels' own text -- cugp_amd/csrc/cov_device.h, the header kernels.hip includes -- runs behind the emulation
// shim tools/host_emul.h, one workgroup at a time as 256 host threads in lock step.  Every buffer is a heap block of exactly the
// size the library gives it, so a build with -fsanitize=address,undefined sees any read or write beyond one; the script
// poisons all padding of K^-1, alpha and V with NaN, so a missing mask shows in the results.  A stand-alone program: the
// sanitizer is linked in, nothing is preloaded.
#include "host_emul.h"
namespace cugp {
#include "cov_device.h"
}
using namespace cugp;

int main(int argc, char** argv)
{
    // input file: ints mode (0 trace, 1 predict-grad) n d npad nt cpad kind wantV, then doubles: sf2 sn2 w[d] X[n*d], and
    //   trace:        Kinv[npad*npad] alpha[npad]                 -> part[(d + 2) * nblocks]
    //   predict-grad: Xt[nt*d] V[cpad*npad] alpha[npad]           -> dmean[nt*d] (dvar[nt*d])
    FILE* f = fopen(argv[1], "rb");
    int hdr[8];
    if (!f || fread(hdr, sizeof(int), 8, f) != 8) return 2;
    const int mode = hdr[0], n = hdr[1], d = hdr[2], npad = hdr[3], nt = hdr[4], cpad = hdr[5], kind = hdr[6], wantV = hdr[7];
    auto rd = [&](size_t cnt) { double* p = (double*)malloc(cnt * 8 ? cnt * 8 : 8); if (fread(p, 8, cnt, f) != cnt) exit(3); return p; };
    // exact-size heap blocks: AddressSanitizer sees any read or write beyond them.  hd: the hyper-scalars directly followed
    // by the d weights, as the handle's staging area
    double* hs = rd(2);
    double* hdw = (double*)malloc((3 + d) * 8);
    hdw[0] = NAN; hdw[1] = hs[0]; hdw[2] = hs[1];                   // (ell_sq is never read: NaN)
    if (fread(hdw + 3, 8, d, f) != (size_t)d) return 3;
    const HyperScalars* hd = (const HyperScalars*)hdw;
    double* X = rd((size_t)n * d);
    FILE* o = nullptr;
    if (mode == 0) {
        double *Kinv = rd((size_t)npad * npad), *alpha = rd(npad);
        fclose(f);
        const int nb = (npad / KT) * (npad / KT + 1) / 2;
        const size_t np = (size_t)(d + 2) * nb;
        double* part = (double*)malloc(np * 8);
        for (size_t i = 0; i < np; i++) part[i] = NAN;
        if (kind == 1) launch(nb, [&] { trace_ard_body<1, false>(X, n, d, npad, hd, Kinv, alpha, 1, part, nullptr); });
        else launch(nb, [&] { trace_ard_body<2, false>(X, n, d, npad, hd, Kinv, alpha, 1, part, nullptr); });
        o = fopen(argv[2], "wb");
        fwrite(part, 8, np, o);
        free(part); free(Kinv); free(alpha);
    } else {
        double *Xt = rd((size_t)nt * d), *V = rd((size_t)cpad * npad), *alpha = rd(npad);
        fclose(f);
        const int tiles = (n + 63) / 64;
        const size_t pstride = (size_t)nt * d;
        double* part = (double*)malloc(tiles * 2 * pstride * 8);
        for (size_t i = 0; i < tiles * 2 * pstride; i++) part[i] = NAN;
        const double* Vp = wantV ? V : nullptr;
        const int blocks = ((nt + 63) / 64) * tiles;
        if (kind == 1) launch(blocks, [&] { k_predict_grad<true, 1>(X, n, d, npad, Xt, nt, HyperScalars{}, nullptr, Vp, alpha, part, pstride, hd); });
        else launch(blocks, [&] { k_predict_grad<true, 2>(X, n, d, npad, Xt, nt, HyperScalars{}, nullptr, Vp, alpha, part, pstride, hd); });
        double* dm = (double*)malloc(pstride * 8);
        double* dv = (double*)malloc(pstride * 8);
        const int fblocks = (int)((pstride + 255) / 256);
        for (int b = 0; b < fblocks; b++)
            for (int t = 0; t < 256; t++) {
                blockIdx.x = b; threadIdx.x = t;
                k_predict_grad_finish(part, pstride, tiles, nt, d, NAN, hdw + 3, dm, wantV ? dv : nullptr);
            }
        o = fopen(argv[2], "wb");
        fwrite(dm, 8, pstride, o);
        if (wantV) fwrite(dv, 8, pstride, o);
        free(part); free(dm); free(dv); free(Xt); free(V); free(alpha);
    }
    fclose(o);
    free(hs); free(hdw); free(X);
    return 0;
}
