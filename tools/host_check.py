"""What the host checks (tools/*_host_check.py) share: build one of the stand-alone programs tools/<name>.cpp -- the
emulation shim tools/host_emul.h, the device headers of cugp_amd/csrc that kernels.hip includes, and a main -- with
-fsanitize=address,undefined, run it on one case's input file, and the command-line driver.  No GPU, nothing preloaded."""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CLANG = os.environ.get("CLANGXX", "/opt/rocm/lib/llvm/bin/clang++")


def build(name, tmp):
    exe = os.path.join(tmp, "host_check")
    subprocess.check_call([CLANG, "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-pthread",
                           "-I", os.path.join(ROOT, "tools"), "-I", os.path.join(ROOT, "cugp_amd", "csrc"),
                           os.path.join(ROOT, "tools", name + ".cpp"), "-o", exe])
    return exe


def execute(exe, fin, fout, *what):
    """One case: False (and the reason printed) on a non-zero exit or on anything on stderr -- a sanitizer's report."""
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    if r.returncode != 0 or r.stderr.strip():
        print(*what, "FAILED with", r.returncode, r.stderr[-3000:])
        return False
    return True


def main(name, cases, run):
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(name, tmp)
        ok = all([run(exe, tmp, *c) for c in cases])
    print("ALL OK" if ok else "SOME BAD")
    return 0 if ok else 1
