"""INTEGRATION.md A-C, executed as written against the reference's UNMODIFIED drivers.

Build container only: needs the reference checkout (CUGP_REFERENCE or /root/reference) and skips without it, so
nothing of the reference travels.  Every ```sh block of INTEGRATION.md whose first line is `# binding-test: NAME`
is run with CUGP = this repository and REF = a symlink shadow of the reference tree (`cp -rs`: the checkout stays
untouched, no file of it is copied).  Compile + link only -- there is no GPU here; the same call sequences run on
the GPU in tests/test_gpu_dropin_cpp.py.
"""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

REF = os.environ.get("CUGP_REFERENCE", "/root/reference")
LIBDIR = os.path.join(ROOT, "cugp_amd", "lib")

# only the recipes themselves need the reference checkout; the checks of INTEGRATION.md and of the host library run anywhere
needs_reference = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "cpp_serial_gp")),
                                     reason="reference checkout not present (build container only)")


def _blocks():
    txt = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    out = {}
    for m in re.finditer(r"```sh\n# binding-test: (\w+)\n(.*?)```", txt, re.S):
        out[m.group(1)] = m.group(2)
    return out


@pytest.fixture(scope="module")
def shadow(tmp_path_factory):
    if not (os.path.exists(os.path.join(LIBDIR, "libcugp.so"))):
        pytest.skip("libcugp.so not built")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "cugp_amd", "host")])
    d = tmp_path_factory.mktemp("refshadow")
    ref = d / "reference"
    subprocess.check_call(["cp", "-rs", REF, str(ref)])
    # distributed_gp includes "eigen3/Eigen/Dense" (a system Eigen on the authors' machines); the only Eigen in
    # this image is the reference's vendored copy under cuda_src/ -- map the path, copy nothing
    inc = d / "inc"
    inc.mkdir()
    os.symlink(os.path.join(REF, "cuda_src"), inc / "eigen3")
    env = dict(os.environ, CUGP=ROOT, REF=str(ref), EIGEN_FLAGS="-I" + str(inc))
    yield ref, env
    shutil.rmtree(d, ignore_errors=True)


def _undefined(exe):
    out = subprocess.run(["nm", "-D", "--undefined-only", exe], capture_output=True, text=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


def _run(name, shadow):
    ref, env = shadow
    blocks = _blocks()
    assert name in blocks, "INTEGRATION.md has no `# binding-test: %s` block" % name
    r = subprocess.run(["bash", "-euo", "pipefail", "-c", blocks[name]], env=env, capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, "recipe %s failed:\n%s\n%s" % (name, blocks[name], r.stderr[-4000:])
    return ref


def test_integration_md_has_every_recipe():
    assert set(_blocks()) == {"A", "B", "B2", "C"}


@needs_reference
def test_recipe_A_serial_driver_links_unmodified(shadow):
    """cpp_serial_gp/serial_gp.cpp against the drop-in covkernel.h (cpp_serial_gp/covkernel.h:20-37)."""
    ref = _run("A", shadow)
    exe = ref / "cpp_serial_gp" / "gp"
    assert exe.exists()
    # the driver source is still the reference's file, and the header it picked up is ours
    assert os.path.realpath(ref / "cpp_serial_gp" / "serial_gp.cpp") == os.path.join(REF, "cpp_serial_gp", "serial_gp.cpp")
    und = _undefined(str(exe))
    assert any("Covsum" in s and "compute_loglikelihood" in s for s in und)      # resolved from libcugp_host.so
    ldd = subprocess.run(["ldd", str(exe)], capture_output=True, text=True).stdout
    assert "libcugp_host.so" in ldd and "libcugp.so" in ldd and "not found" not in ldd


@needs_reference
def test_recipe_C_bcm_driver_links_unmodified(shadow):
    """distributed_gp/distributed_ver1.cpp (its own by-value cg_solve(BCM), Eigen bookkeeping) against the drop-in
    covkernel.h + BCM.h (distributed_gp/BCM.h:2-27)."""
    ref = _run("C", shadow)
    exe = ref / "distributed_gp" / "dgp"
    assert exe.exists()
    und = _undefined(str(exe))
    for want in ("get_BCM_loglikelihood", "get_BCM_gradient_hyper", "set_BCM_log_hyperparam"):   # the prediction calls are dead code there (:288)
        assert any(want in s for s in und), want
    # passing the class by value needs its copy constructor
    assert any(re.search(r"_ZN3BCMC[12]ERKS_", s) for s in und)


@needs_reference
@pytest.mark.parametrize("name,sub", [("B", "cuda_scalingdist"), ("B2", "cuda_bettersinglenode_ver2")])
def test_recipe_B_gpu_drivers_link_unmodified(shadow, name, sub):
    """main.cpp + cg_solver.cpp + csapp.cpp (cuda_scalingdist/main.cpp:14-67, cg_solver.cpp:14-40) with
    libcugp_host.so in the place of cuda_gp.cu; set_loghyper_eigen(Eigen::VectorXd) from gp_api_eigen.cpp."""
    ref = _run(name, shadow)
    exe = ref / sub / "gp"
    assert exe.exists()
    und = _undefined(str(exe))
    for want in ("_Z22compute_log_likelihoodv", "_Z32compute_gradient_log_hyperparamsPd", "_Z17get_loghyperparamv",
                 "_Z12set_loghyperPKd"):
        assert want in und, want
    if name == "B":
        # (the four data symbols X_host* / labels_host* bind by copy relocation: checked on the library side below)
        for want in ("_Z27read_trainingdata_into_dramNSt7__cxx1112basic_stringIcSt11char_traitsIcESaIcEEES4_PdS5_",
                     "_Z25copy_training_data_to_GPUPdS_", "_Z5setupii"):
            assert want in und, want


def test_host_library_exports_surface_b():
    """Every symbol the reference's GPU drivers forward-declare and do not define themselves."""
    if not os.path.exists(os.path.join(LIBDIR, "libcugp_host.so")):
        pytest.skip("libcugp_host.so not built")
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIBDIR, "libcugp_host.so")],
                         capture_output=True, text=True).stdout
    have = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for want in ("X_host", "labels_host", "X_host_buffers", "labels_host_buffers", "_Z5setupii",
                 "_Z22compute_log_likelihoodv", "_Z32compute_gradient_log_hyperparamsPd", "_Z17get_loghyperparamv",
                 "_Z8cg_solvePc", "_Z13testing_phaseii", "_Z23destruct_cublas_cusolerv", "_Z12set_loghyperPKd",
                 "_Z25copy_training_data_to_GPUPdS_"):
        assert want in have, want
    # the drivers define these themselves (main.cpp:14-16): the library must not
    assert "numtrain" not in have and "dimensions" not in have
