// Host check of trace_ard_body<KIND, false> (k_trace<true, KIND>) and k_predict_grad<true, KIND> (tools/ard_matern_host_check.py builds and runs this; no
// GPU).  The kernels' own text -- cut out of cugp_amd/csrc/kernels.hip into body.inc by the script -- runs one workgroup at
// a time as 256 host threads in lock step: a barrier stands for __syncthreads, an exchange array and two barriers for the
// shuffles (__shfl_down inside a 64-lane wave, __shfl_xor inside 16 lanes).  Every buffer is a heap block of exactly the
// size the library gives it, so a build with -fsanitize=address,undefined sees any read or write beyond one; the script
// poisons all padding of K^-1, alpha and V with NaN, so a missing mask shows in the results.  A stand-alone program: the
// sanitizer is linked in, nothing is preloaded.
#include <barrier>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>
#include <functional>
typedef double d2 __attribute__((ext_vector_type(2)));
struct Idx { int x = 0, y = 0, z = 0; };
static thread_local Idx threadIdx;
static Idx blockIdx, gridDim;
static std::barrier<> g_bar(256);
static double g_slot[256];
#define __device__
#define __global__
#define __forceinline__ inline
#define __restrict__
#define __launch_bounds__(...)
#define __shared__ static
static inline void __syncthreads() { g_bar.arrive_and_wait(); }
static inline double __shfl_xor(double v, int m, int w)
{
    g_slot[threadIdx.x] = v;
    g_bar.arrive_and_wait();
    const double r = g_slot[threadIdx.x ^ m];
    g_bar.arrive_and_wait();
    return r;
}
static inline double __shfl_down(double v, int o, int w)     // (a lane beyond the wave's end keeps its own value)
{
    g_slot[threadIdx.x] = v;
    g_bar.arrive_and_wait();
    const int lane = threadIdx.x & 63;
    const double r = lane + o < 64 ? g_slot[threadIdx.x + o] : v;
    g_bar.arrive_and_wait();
    return r;
}
using std::exp;
using std::sqrt;
struct HyperScalars { double ell_sq, signal_var, noise_var; };
struct ExpertPtrs {
    double *A, *T, *U, *Kinv, *d16, *d64, *logdet, *y, *z, *alpha, *w, *part, *out;
    const double* X;
    unsigned* tickets;
    int n;
};
template <class T> static inline T* GP(T* p) { return p; }
enum { KERNEL_SE = 0, KERNEL_MATERN32 = 1, KERNEL_MATERN52 = 2 };
constexpr int KT = 64, DC = 16;
#include "body.inc"

template <class F> void launch(int blocks, F f)
{
    gridDim.x = blocks;
    for (int b = 0; b < blocks; b++) {
        blockIdx.x = b;
        std::vector<std::thread> th;
        for (int t = 0; t < 256; t++) th.emplace_back([=] { threadIdx.x = t; f(); });
        for (auto& x : th) x.join();
    }
}

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
