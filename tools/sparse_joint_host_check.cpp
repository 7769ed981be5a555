// Host check of the sparse model's input-gradient pass (tools/sparse_joint_host_check.py builds and runs this; no GPU).  The
// kernel's own text -- cugp_amd/csrc/sparse_predict_device.h, the header kernels.hip includes -- runs behind the emulation
// shim tools/host_emul.h, one workgroup at a time as 256 host threads: k_sparse_predict_diff with D and a, with a alone (D
// null, Wt and T null too: they must not be read) and with D alone (a and bp null).  Wt, T and D are heap blocks of
// rows + 64 rows, the 64 spare rows NaN in the inputs and a marker in the output: a pass that reads or writes beyond `rows`
// shows; bp is a heap block of exactly m doubles, so a read beyond m is a sanitizer report.  A stand-alone program: the
// sanitizer is linked in, nothing is preloaded.
#include "host_emul.h"
namespace cugp {
#include "sparse_predict_device.h"
}
using namespace cugp;

int main(int argc, char** argv)
{
    // input: ints rows ld m, then doubles: s2 | Wt[(rows + 64) * ld] T[(rows + 64) * ld] bp[m]
    // output: D[(rows + 64) * ld] a[ld] | a_alone[ld] | D_alone[(rows + 64) * ld] | Dref[(rows + 64) * ld] aref[ld]
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    int hdr[3];
    if (!f || fread(hdr, sizeof(int), 3, f) != 3) return 2;
    const int rows = hdr[0], ld = hdr[1], m = hdr[2];
    auto rd = [&](size_t cnt) { double* p = (double*)malloc(cnt * 8 ? cnt * 8 : 8); if (fread(p, 8, cnt, f) != cnt) exit(3); return p; };
    double* sc = rd(1);
    const size_t all = (size_t)(rows + 64) * ld, used = (size_t)rows * ld;
    double *Wt = rd(all), *T = rd(all), *bp = rd(m);
    fclose(f);
    const double s2 = sc[0], marker = -12345.0;
    auto block = [&](size_t cnt) { double* p = (double*)malloc(cnt * 8 ? cnt * 8 : 8); for (size_t i = 0; i < cnt; i++) p[i] = marker; return p; };
    double *D = block(all), *a = block(ld), *a1 = block(ld), *D1 = block(all), *Dref = block(all), *aref = block(ld);
    const size_t total = used > (size_t)ld ? used : (size_t)ld;
    launch((int)((total + 255) / 256), [&] { k_sparse_predict_diff(Wt, T, D, ld, rows, bp, s2, m, a); });
    launch((ld + 255) / 256, [&] { k_sparse_predict_diff(nullptr, nullptr, nullptr, ld, rows, bp, s2, m, a1); });
    launch((int)((total + 255) / 256), [&] { k_sparse_predict_diff(Wt, T, D1, ld, rows, nullptr, s2, m, nullptr); });
    // the plain loop
    for (size_t e = 0; e < used; e++) Dref[e] = Wt[e] - T[e];
    for (int i = 0; i < ld; i++) aref[i] = i < m ? bp[i] / s2 : 0.0;

    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    fwrite(D, 8, all, o);
    fwrite(a, 8, ld, o);
    fwrite(a1, 8, ld, o);
    fwrite(D1, 8, all, o);
    fwrite(Dref, 8, all, o);
    fwrite(aref, 8, ld, o);
    fclose(o);
    for (double* p : {sc, Wt, T, bp, D, a, a1, D1, Dref, aref}) free(p);
    return 0;
}
