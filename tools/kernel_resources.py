"""Registers, LDS and scratch of every kernel of libcugp.so, from the code-object notes hipcc writes for gfx950
(no GPU needed):  python tools/kernel_resources.py > profiles/r03_kernel_resources.txt
Workgroups per CU = min over the limits: 512 unified VGPRs per SIMD lane (VGPR + AGPR, allocation granule 8),
160 KiB LDS per CU (static + the dynamic size the launcher asks for), 32 waves per CU.
--digest: instead of the table, one line per kernel with a sha256 of its instructions (label to .Lfunc_end, without
comments, .loc / .file / .section / .text lines and blank lines, block labels .LBB<n>_ and the kernel's own symbol
normalised, so that a renamed kernel or one that became a template keeps its digest) -- equal digests before and after a
refactor of kernels.hip mean that no kernel's code changed:  python tools/kernel_resources.py --digest [kernels.hip]"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "cugp_amd", "csrc", "kernels.hip")
# dynamic LDS per launch (kernels.hip: set_big_lds / the launchers): Geo<4>::LDS, Geo<2>::LDS, POTF2_LDS, TRTRI_LDS
GEMM4, GEMM2, POTF2, TRTRI = 66048, 33280, 79360, 78336
DYN = {"k_lauum<4>": GEMM4, "k_lauum<2>": GEMM2, "k_trtri_level<4>": GEMM4, "k_trtri_level<2>": GEMM2,
       "k_trtri_border<4>": GEMM4, "k_trtri_border<2>": GEMM2, "k_predict_gemm": GEMM4, "k_test_gemm": GEMM4,
       "k_syrk_wide": GEMM4, "k_syrk_step": POTF2, "k_potf2": POTF2, "k_trtri_diag": TRTRI,
       "k_predict_cov<4>": GEMM4, "k_predict_cov<2>": GEMM2, "k_targets_alpha": GEMM2, "k_targets_alpha_batched": GEMM2, "k_targets_mean": GEMM2, "k_append_kinv": GEMM2,
       "k_loo_product<4>": GEMM4, "k_loo_product<2>": GEMM2, "k_sparse_gram": GEMM4,
       "k_sparse_predict_cov<4>": GEMM4, "k_sparse_predict_cov<2>": GEMM2,
       "k_syrk_wide8": GEMM4, "k_lauum8": GEMM4, "k_trtri_border8": GEMM4,
       "k_syrk_wide_rest": GEMM2, "k_lauum_rest": GEMM2, "k_trtri_border_rest": GEMM2}

with tempfile.TemporaryDirectory() as td:
    out = os.path.join(td, "k.s")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-x", "hip", "-S",
                           "--cuda-device-only", "-o", out, sys.argv[-1] if sys.argv[-1].endswith(".hip") else SRC],
                          stderr=subprocess.DEVNULL)
    txt = open(out).read()
if "--digest" in sys.argv:
    names = sorted(re.findall(r"^    \.name:\s+(\S+)$", txt[txt.index("amdhsa.kernels:"):], re.M))
    dems = subprocess.run(["c++filt"] + names, capture_output=True, text=True).stdout.split("\n")
    for name, dem in zip(names, dems):
        body = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end\d+:" % re.escape(name), txt, re.M | re.S).group(1)
        lines = [re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r";.*", "", ln)).replace(name, "<kernel>").strip() for ln in body.split("\n")]
        lines = [ln for ln in lines if ln and not ln.startswith((".loc", ".file", ".section", ".text"))]
        print("%s  %5d  %s" % (hashlib.sha256("\n".join(lines).encode()).hexdigest()[:32], len(lines),
                               re.sub(r"^void |cugp::|\(.*$", "", dem)))
    sys.exit(0)
blocks = re.split(r"\n  - \.agpr_count:", txt[txt.index("amdhsa.kernels:"):])
print("%-22s %5s %5s %5s %8s %8s %8s %7s %6s" % ("kernel", "vgpr", "agpr", "sgpr", "lds_stat", "lds_dyn", "scratch", "threads", "wg/CU"))
for b in blocks[1:]:
    def f(key):
        m = re.search(r"\.%s:\s+(\S+)" % key, b)
        return m.group(1) if m else "0"
    agpr = int(b.strip().split()[0])
    name = f("name")
    dem = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
    short = re.sub(r"^void |cugp::|\(.*$", "", dem)
    vg, sg = int(f("vgpr_count")), int(f("sgpr_count"))
    lds, scr, thr = int(f("group_segment_fixed_size")), int(f("private_segment_fixed_size")), int(f("max_flat_workgroup_size"))
    dyn = DYN.get(short, 0)
    waves = thr // 64
    regs = -(-(-(-vg // 4) * 4 + agpr) // 8) * 8   # unified file: accumulation registers follow the (4-aligned) VGPRs
    by_reg = (512 // regs) * 4 // waves if regs else 99
    by_lds = (160 * 1024) // (lds + dyn) if lds + dyn else 99
    by_waves = 32 // waves
    print("%-22s %5d %5d %5d %8d %8d %8d %7d %6d" % (short, vg, agpr, sg, lds, dyn, scr, thr, min(by_reg, by_lds, by_waves)))
