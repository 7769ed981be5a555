// Host check of the sharded sparse model's kernels (tools/sparse_shard_host_check.py builds and runs this; no GPU).  The
// kernels' own text -- cugp_amd/csrc/sparse_shard_device.h behind cov_device.h, the headers kernels.hip includes -- runs
// behind the emulation shim tools/host_emul.h, one workgroup at a time as 256 host threads in lock step:
// k_sparse_shard_reduce over a gathered block, k_sparse_shard_sums over a shard's trace partials and
// k_sparse_finalize_sharded.  Every buffer is a heap block of exactly the size the library gives it, so a build with
// -fsanitize=address,undefined sees any access beyond one; the script puts NaN wherever a kernel must not read (headers,
// empty slots, the slot's entries outside the reduced range, columns beyond m) and compares the results bit for bit with
// its own plain loops.  A stand-alone program: the sanitizer is linked in, nothing is preloaded.
#include "host_emul.h"
namespace cugp {
#include "cov_device.h"
#include "sparse_shard_device.h"
}
using namespace cugp;

int main(int argc, char** argv)
{
    // input: ints K W per hdr slot off len grid nb_uf nl nb_uu m ld nt grad, then doubles: gathered[W * (hdr + per * slot)]
    //        part_uf[(nl + 1) * nb_uf] | P[ld * ld] Binv[ld * ld] Cp[ld] Gm[ld] logdet[nt] yyn[2] {sf2, s2, log_s2} suf[nl + 1]
    //        part_uu[(nl + 1) * nb_uu]
    // output: reduce[len] sums[nl + 1] out[nl + 4] hout[nl + 4]
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    int h[15];
    if (!f || fread(h, sizeof(int), 15, f) != 15) return 2;
    const int K = h[0], W = h[1], per = h[2], hdr = h[3], slot = h[4], off = h[5], len = h[6], grid = h[7], nb_uf = h[8], nl = h[9],
              nb_uu = h[10], m = h[11], ld = h[12], nt = h[13], grad = h[14];
    auto rd = [&](size_t cnt) { double* p = (double*)malloc(cnt * 8 ? cnt * 8 : 8); if (fread(p, 8, cnt, f) != cnt) exit(3); return p; };
    auto nan_block = [](size_t cnt) { double* p = (double*)malloc(cnt * 8 ? cnt * 8 : 8); for (size_t i = 0; i < cnt; i++) p[i] = NAN; return p; };
    const size_t rstride = (size_t)hdr + (size_t)per * slot;
    double* gathered = rd((size_t)W * rstride);
    double* part_uf = rd((size_t)(nl + 1) * nb_uf);
    double *P = rd((size_t)ld * ld), *Binv = rd((size_t)ld * ld), *Cp = rd(ld), *Gm = rd(ld), *logdet = rd(nt), *yyn = rd(2);
    double* sc = rd(3);
    double *suf = rd(nl + 1), *part_uu = rd((size_t)(nl + 1) * nb_uu);
    fclose(f);
    double *red = nan_block(len), *sums = nan_block(nl + 1), *out = nan_block(nl + 4), *hout = nan_block(nl + 4);
    launch(grid, [&] { k_sparse_shard_reduce(gathered, rstride, (size_t)hdr, (size_t)slot, (size_t)off, (size_t)len, W, K, red); });
    launch(1, [&] { k_sparse_shard_sums(part_uf, (size_t)nb_uf, nl, sums); });
    const SparseFinalSharded fin{P, Binv, Cp, Gm, logdet, yyn, m, ld, nt, sc[0], sc[1], sc[2]};
    launch(1, [&] { k_sparse_finalize_sharded(fin, grad ? suf : nullptr, grad ? part_uu : nullptr, (size_t)nb_uu, nl, out, hout); });
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    fwrite(red, 8, len, o);
    fwrite(sums, 8, nl + 1, o);
    fwrite(out, 8, nl + 4, o);
    fwrite(hout, 8, nl + 4, o);
    fclose(o);
    for (double* p : {gathered, part_uf, P, Binv, Cp, Gm, logdet, yyn, sc, suf, part_uu, red, sums, out, hout}) free(p);
    return 0;
}
