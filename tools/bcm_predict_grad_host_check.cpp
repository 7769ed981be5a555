// Host check of the batched test-input gradient kernels and of the device chain rule (tools/bcm_predict_grad_host_check.py
// builds and runs this; no GPU).  The kernels' own text -- cugp_amd/csrc/cov_device.h and bcm_grad_device.h, the headers
// kernels.hip includes -- runs behind the emulation shim tools/host_emul.h, one workgroup at a time as 256 host threads in
// lock step, blockIdx.y set per expert.  Every buffer is a heap block of exactly the size the library gives it, so a build
// with -fsanitize=address,undefined sees any read or write beyond one; the script poisons everything the kernels must not
// use with NaN.  A stand-alone program: the sanitizer is linked in, nothing is preloaded.
#include "host_emul.h"
namespace cugp {
#include "cov_device.h"
#include "bcm_grad_device.h"
}
using namespace cugp;

static FILE* g_in = nullptr;
static double* rd(size_t cnt)
{
    double* p = (double*)malloc(cnt * 8 ? cnt * 8 : 8);
    if (fread(p, 8, cnt, g_in) != cnt) exit(3);
    return p;
}
static double* nans(size_t cnt)
{
    double* p = (double*)malloc(cnt * 8 ? cnt * 8 : 8);
    for (size_t i = 0; i < cnt; i++) p[i] = NAN;
    return p;
}

// one thread per entry, no barrier and no shuffle: the threads of a workgroup one after the other
template <class F> static void launch_flat(size_t total, int by, F f)
{
    const int blocks = (int)((total + 255) / 256);
    gridDim.x = blocks;
    for (int y = 0; y < by; y++)
        for (int b = 0; b < blocks; b++)
            for (int t = 0; t < 256; t++) {
                blockIdx.x = b; blockIdx.y = y; threadIdx.x = t;
                f();
            }
    blockIdx.y = 0;
}

// mode 0: ints K d npad nt cpad kind ard wantV n[K]; doubles ell_sq sf2 sn2 w[d], per expert X[n d] alpha[npad], Xt[nt d],
//         Ks[K][cpad][npad], V[K][cpad][npad]  ->  rows of the batched launches [K][(2 + 2 d) nt], then the same from the
//         single-expert kernels on each expert's slices
template <bool ARD, int KIND>
static void grads(int K, int d, int npad, int nt, int cpad, int wantV, const int* n, const HyperScalars& h,
                  const HyperScalars* hd, const double* wts, ExpertPtrs* tab, const double* Xt, const double* Ks,
                  const double* V, double* rows, double* single)
{
    const size_t kslice = (size_t)cpad * npad, pstride = (size_t)nt * d, slot = (2 + 2 * (size_t)d) * nt;
    int tiles = 0;
    for (int k = 0; k < K; k++) tiles = predict_grad_tiles(n[k]) > tiles ? predict_grad_tiles(n[k]) : tiles;
    const size_t pslice = (size_t)tiles * 2 * pstride;
    const int tiles_t = (nt + 63) / 64;
    const double* Vp = wantV ? V : nullptr;
    double* part = nans((size_t)K * pslice);
    for (int k = 0; k < K; k++) {
        blockIdx.y = k;
        launch(tiles_t * tiles, [&] { k_predict_grad_batched<ARD, KIND>(d, npad, Xt, nt, h, Ks, Vp, kslice, part, pstride, pslice, hd, tab); });
    }
    blockIdx.y = 0;
    launch_flat(pstride, K, [&] {
        k_predict_grad_finish_batched(part, pstride, pslice, nt, d, h.ell_sq, wts, rows + 2 * (size_t)nt,
                                      wantV ? rows + 2 * (size_t)nt + pstride : nullptr, slot, tab);
    });
    free(part);
    for (int k = 0; k < K; k++) {                       // the existing single-expert kernels in the same emulation
        const int tk = predict_grad_tiles(n[k]);
        double* p1 = nans((size_t)tk * 2 * pstride);
        launch(tiles_t * tk, [&] {
            k_predict_grad<ARD, KIND>(tab[k].X, n[k], d, npad, Xt, nt, h, Ks + k * kslice, Vp ? Vp + k * kslice : nullptr,
                                      tab[k].alpha, p1, pstride, hd);
        });
        double* r = single + k * slot;
        launch_flat(pstride, 1, [&] {
            k_predict_grad_finish(p1, pstride, tk, nt, d, h.ell_sq, wts, r + 2 * (size_t)nt, wantV ? r + 2 * (size_t)nt + pstride : nullptr);
        });
        free(p1);
    }
}

int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    g_in = fopen(argv[1], "rb");
    int mode = -1;
    if (!g_in || fread(&mode, sizeof(int), 1, g_in) != 1) return 2;
    FILE* o = nullptr;
    if (mode == 0) {
        int hdr[8];
        if (fread(hdr, sizeof(int), 8, g_in) != 8) return 2;
        const int K = hdr[0], d = hdr[1], npad = hdr[2], nt = hdr[3], cpad = hdr[4], kind = hdr[5], ard = hdr[6], wantV = hdr[7];
        std::vector<int> n(K);
        if (fread(n.data(), sizeof(int), K, g_in) != (size_t)K) return 2;
        double* hs = rd(3);
        double* hdw = (double*)malloc((3 + d) * 8);           // the hyper-scalars directly followed by the d weights
        hdw[0] = ard ? NAN : hs[0]; hdw[1] = hs[1]; hdw[2] = hs[2];
        if (fread(hdw + 3, 8, d, g_in) != (size_t)d) return 3;
        const HyperScalars h{ard ? NAN : hs[0], hs[1], hs[2]};
        const HyperScalars* hd = ard ? (const HyperScalars*)hdw : nullptr;
        const double* wts = ard ? hdw + 3 : nullptr;
        ExpertPtrs* tab = (ExpertPtrs*)calloc(K, sizeof(ExpertPtrs));
        for (int k = 0; k < K; k++) { tab[k].X = rd((size_t)n[k] * d); tab[k].alpha = rd(npad); tab[k].n = n[k]; }
        double* Xt = rd((size_t)nt * d);
        double* Ks = rd((size_t)K * cpad * npad);
        double* V = rd((size_t)K * cpad * npad);
        fclose(g_in);
        const size_t slot = (2 + 2 * (size_t)d) * nt;
        double *rows = nans(K * slot), *single = nans(K * slot);
        if (ard && kind == 0) grads<true, 0>(K, d, npad, nt, cpad, wantV, n.data(), h, hd, wts, tab, Xt, Ks, V, rows, single);
        else if (ard && kind == 2) grads<true, 2>(K, d, npad, nt, cpad, wantV, n.data(), h, hd, wts, tab, Xt, Ks, V, rows, single);
        else if (!ard && kind == 0) grads<false, 0>(K, d, npad, nt, cpad, wantV, n.data(), h, hd, wts, tab, Xt, Ks, V, rows, single);
        else return 4;
        o = fopen(argv[2], "wb");
        fwrite(rows, 8, K * slot, o);
        fwrite(single, 8, K * slot, o);
        for (int k = 0; k < K; k++) { free((void*)tab[k].X); free(tab[k].alpha); }
        free(tab); free(hs); free(hdw); free(Xt); free(Ks); free(V); free(rows); free(single);
    } else if (mode == 1) {
        // ints world K nt d per combine with_noise want_dvar; doubles sf2 sn2 gathered[world][2 + per (2 + 2 d) nt]
        //   -> out [mean nt | var nt | dmean nt d | dvar nt d | world x {status, count}]
        int hdr[8];
        if (fread(hdr, sizeof(int), 8, g_in) != 8) return 2;
        const int world = hdr[0], K = hdr[1], nt = hdr[2], d = hdr[3], per = hdr[4], combine = hdr[5], with_noise = hdr[6], want_dvar = hdr[7];
        double* sc = rd(2);
        const size_t rstride = 2 + (size_t)per * (2 + 2 * (size_t)d) * nt, nout = (2 + 2 * (size_t)d) * nt + 2 * (size_t)world;
        double* g = rd(world * rstride);
        fclose(g_in);
        double* out = nans(nout);
        launch_flat((size_t)nt * d, 1, [&] { k_poe_reduce_grad(g, rstride, world, K, nt, d, combine, sc[0], sc[1], with_noise, want_dvar, out); });
        o = fopen(argv[2], "wb");
        fwrite(out, 8, nout, o);
        free(sc); free(g); free(out);
    } else return 2;
    fclose(o);
    return 0;
}
