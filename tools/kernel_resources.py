"""Registers, LDS and scratch of every kernel of libcugp.so, from the code-object notes hipcc writes for gfx950
(no GPU needed):  python tools/kernel_resources.py > profiles/kernel_resources.txt
Workgroups per CU = min over the limits: 512 unified VGPRs per SIMD lane (VGPR + AGPR, allocation granule 8),
160 KiB LDS per CU (static + the dynamic size the launcher asks for), 32 waves per CU.
The dynamic size is read from the source text, which states it once: the LDS argument of the kernel's launch line
(CUGP_LAUNCH / hipLaunchKernelGGL in kernels.hip and the headers it includes) names a constant, and a static_assert beside
that constant's definition pins its number.  A launch whose LDS argument has no such static_assert, or a kernel launched
with two different sizes, ends the run with a message that names the kernel.
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
SRC = sys.argv[-1] if sys.argv[-1].endswith(".hip") else os.path.join(ROOT, "cugp_amd", "csrc", "kernels.hip")


def source_text(path, seen=None):
    """the file and, in place of each #include "x.h" line, the text of x.h beside it; macro definitions dropped (the body of
    CUGP_LAUNCH is a launch line of its own parameters)"""
    seen = set() if seen is None else seen
    out, in_macro = [], False
    for ln in open(path).read().split("\n"):
        if in_macro or ln.startswith("#define"):
            in_macro = ln.endswith("\\")
            continue
        m = re.match(r'#include "([^"]+)"', ln)
        inc = os.path.join(os.path.dirname(path), m.group(1)) if m else None
        if inc and os.path.exists(inc) and inc not in seen:
            seen.add(inc)
            out.append(source_text(inc, seen))
        else:
            out.append(ln)
    return "\n".join(out)


def call_args(txt, start):
    """top-level arguments of the call whose opening parenthesis is at txt[start]"""
    args, depth, cur = [], 0, ""
    for ch in txt[start:]:
        if ch in "([{":
            depth += 1
            if depth == 1:
                continue
        elif ch in ")]}":
            depth -= 1
            if depth == 0:
                break
        if ch == "," and depth == 1:
            args.append(cur)
            cur = ""
        else:
            cur += ch
    return [" ".join(a.split()) for a in args + [cur]]


def dynamic_lds(txt):
    """{kernel as the code object's demangled name spells it, or a template's stem: bytes of dynamic LDS it is launched with}"""
    txt = re.sub(r"//[^\n]*", "", txt)
    pinned = {m.group(1): int(m.group(2)) for m in re.finditer(r"static_assert\(([\w<>:]+) == (\d+),", txt)}
    dyn = {}
    for m in re.finditer(r"\b(?:CUGP_LAUNCH|hipLaunchKernelGGL)\(", txt):
        a = call_args(txt, m.end() - 1)
        kernel, lds = a[0], a[3]
        cov = re.match(r"CUGP_COV_KERNEL3?\(\w+, (\w+)\)$", kernel)          # every <ARD, KIND> of the pass: the stem
        kernel = cov.group(1) if cov else re.sub(r"^\((.*)\)$", r"\1", kernel)
        if lds != "0" and lds not in pinned:
            sys.exit("kernel_resources: %s is launched with dynamic LDS '%s', which no static_assert pins to a number" % (kernel, lds))
        size = 0 if lds == "0" else pinned[lds]
        if dyn.setdefault(kernel, size) != size:
            sys.exit("kernel_resources: %s is launched with two dynamic LDS sizes, %d and %d" % (kernel, dyn[kernel], size))
    return dyn


DYN = {} if "--digest" in sys.argv else dynamic_lds(source_text(SRC))      # (before the compile: a launch it cannot read ends the run at once)
with tempfile.TemporaryDirectory() as td:
    out = os.path.join(td, "k.s")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-x", "hip", "-S",
                           "--cuda-device-only", "-o", out, SRC], stderr=subprocess.DEVNULL)
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
    dyn = DYN.get(short, DYN.get(short.split("<")[0], 0))
    waves = thr // 64
    regs = -(-(-(-vg // 4) * 4 + agpr) // 8) * 8   # unified file: accumulation registers follow the (4-aligned) VGPRs
    by_reg = (512 // regs) * 4 // waves if regs else 99
    by_lds = (160 * 1024) // (lds + dyn) if lds + dyn else 99
    by_waves = 32 // waves
    print("%-22s %5d %5d %5d %8d %8d %8d %7d %6d" % (short, vg, agpr, sg, lds, dyn, scr, thr, min(by_reg, by_lds, by_waves)))
