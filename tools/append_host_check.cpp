// Host check of k_append_border and k_append_kinv (tools/append_host_check.py builds and runs this; no GPU).
// The kernels' own text -- cugp_amd/csrc/append_device.h, the header kernels.hip includes -- runs behind the emulation
// shim tools/host_emul.h, one workgroup at a time as 256 host threads in lock step.
// The fp64 MFMA tile product and its accumulate-and-store epilogue (tile_nt, tile_accum_store: existing
// code) are stood in for by plain loops over the same pointers and k range, so what is checked of k_append_kinv is its
// own part: which tiles, which rows of Qt, which k range, the alpha update.  Every buffer is a heap block of exactly the
// size the library gives it, so a build with -fsanitize=address,undefined sees any access beyond one; the script fills
// what the kernels must not read with NaN.  A stand-alone program: the sanitizer is linked in, nothing is preloaded.
#include "host_emul.h"
namespace cugp {
#include "cov_device.h"
// stand-ins for the fp64 MFMA tile machinery: one 64 x 64 accumulator per workgroup, filled and stored by thread 0
static double g_acc[64][64];
template <int WM> static void acc_zero(d4 (&)[WM][WM]) { __syncthreads(); if (threadIdx.x == 0) memset(g_acc, 0, sizeof g_acc); __syncthreads(); }
template <bool NEGA, int WM>
static void tile_nt(const double* A, int lda, const double* B, int ldb, int k0, int k1, d4 (&)[WM][WM], char*)
{
    if (threadIdx.x == 0)
        for (int i = 0; i < 64; i++)
            for (int j = 0; j < 64; j++)
                for (int k = k0; k < k1; k++) g_acc[i][j] += A[(size_t)i * lda + k] * B[(size_t)j * ldb + k];
    __syncthreads();
}
template <int SIGN, int WM> static void tile_accum_store(double* C, int ldc, const d4 (&)[WM][WM])
{
    if (threadIdx.x == 0)
        for (int i = 0; i < 64; i++)
            for (int j = 0; j < 64; j++) C[(size_t)i * ldc + j] += SIGN * g_acc[i][j];
    __syncthreads();
}
#include "append_device.h"
}
using namespace cugp;

int main(int argc, char** argv)
{
    // input: ints r0 k npad, then doubles P[128*npad] V[128*npad] Cf[128*128] Ci[128*128] flog[1] A T U Kinv [npad*npad each]
    // y z alpha [npad each] logdet[npad/128]; output: A T U Kinv y z alpha logdet, Qt[npad*128]
    FILE* f = fopen(argv[1], "rb");
    int hdr[3];
    if (!f || fread(hdr, sizeof(int), 3, f) != 3) return 2;
    const int r0 = hdr[0], k = hdr[1], npad = hdr[2];
    auto rd = [&](size_t cnt) { double* p = (double*)malloc(cnt * 8); if (fread(p, 8, cnt, f) != cnt) exit(3); return p; };
    const size_t strip = (size_t)128 * npad, nn = (size_t)npad * npad;
    double *P = rd(strip), *V = rd(strip), *Cf = rd(128 * 128), *Ci = rd(128 * 128), *flog = rd(1);
    double *A = rd(nn), *T = rd(nn), *U = rd(nn), *Kinv = rd(nn), *y = rd(npad), *z = rd(npad), *alpha = rd(npad);
    double* logdet = rd(npad / 128);
    fclose(f);
    double* Qt = (double*)malloc(strip * 8);
    for (size_t i = 0; i < strip; i++) Qt[i] = NAN;
    const int nq = (r0 + 63) / 64 * (64 / APB_COLS);
    launch(nq + 1, [&] { k_append_border(P, V, Cf, Ci, flog, r0, k, npad, nq, A, T, U, Kinv, y, z, alpha, logdet, Qt); });
    const int n64 = (r0 + 63) / 64, lower = n64 * (n64 + 1) / 2, tiles = lower + n64 / 2, k16 = (k + 15) / 16 * 16;
    launch(tiles + (r0 + 255) / 256, [&] { k_append_kinv(Qt, k16, k, r0, npad, lower, tiles, Kinv, z + r0, alpha); });
    f = fopen(argv[2], "wb");
    for (double* p : {A, T, U, Kinv}) fwrite(p, 8, nn, f);
    for (double* p : {y, z, alpha}) fwrite(p, 8, npad, f);
    fwrite(logdet, 8, npad / 128, f);
    fwrite(Qt, 8, strip, f);
    fclose(f);
    for (double* p : {P, V, Cf, Ci, flog, A, T, U, Kinv, y, z, alpha, logdet, Qt}) free(p);
    return 0;
}
