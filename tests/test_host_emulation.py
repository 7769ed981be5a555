"""The host checks of the emulable device code as tests, without a GPU: cugp_amd/csrc/cov_device.h and append_device.h --
the text kernels.hip compiles for gfx950 -- run behind tools/host_emul.h as 256 host threads per workgroup in stand-alone
programs built with -fsanitize=address,undefined (tools/*_host_check.cpp), on exact-size heap buffers with NaN where the
kernels must not read, and are compared with numpy by the scripts' own run(): their formulas and tolerances (1e-12 of the
sum of the terms' absolute values for the traces, 1e-13 for the gradients, 1e-12 for append).  Each program is built once
per module.  The cases are those of the scripts' lists with npad <= 384 (a few seconds each); the scripts run all.
A case fails on a non-zero exit, on anything a sanitizer writes to stderr, and on a result beyond its tolerance."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import host_check  # noqa: E402
import append_host_check  # noqa: E402
import ard_matern_host_check  # noqa: E402
import predict_grad_host_check  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists(host_check.CLANG), reason="no host compiler at " + host_check.CLANG)

PREDICT_GRAD = [("se", "n2", None, 1), ("se", "n64", None, 1), ("se", "n65", None, 1), ("se", "n65", None, 0),
                ("matern32", "n65", None, 1), ("ard", "n257_d3_shift", None, 1), ("matern52", "n300_d17", 129, 1),
                ("matern32", "n2", None, 1), ("ard", "n2_d2", None, 1), ("se", "n63", 1, 1)]
ARD_MATERN = [("trace", "n65_d2", 1, None, 1), ("trace", "n65_d2", 2, None, 1), ("trace", "n257_d3_shift", 2, None, 1),
              ("grad", "n65_d2", 1, None, 1), ("grad", "n65_d2", 2, None, 0), ("grad", "n257_d3_shift", 2, None, 1),
              ("grad", "n257_d3", 2, 129, 1),
              ("trace", "n2_d2", 1, None, 1), ("trace", "n63_d2", 2, None, 1), ("grad", "n2_d2", 2, None, 1),
              ("grad", "n63_d2", 1, None, 1)]
APPEND = list(append_host_check.CASES)
CHECKS = {"predict_grad": predict_grad_host_check, "ard_matern": ard_matern_host_check, "append": append_host_check}
ident = lambda case: "-".join(str(v) for v in case)


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """name -> (the program, built on first use; a directory for its case files)"""
    built = {}

    def get(name):
        if name not in built:
            tmp = str(tmp_path_factory.mktemp(name))
            built[name] = (host_check.build(name + "_host_check", tmp), tmp)
        return built[name]
    return get


def check(programs, capfd, name, case):
    assert case in CHECKS[name].CASES                  # (the scripts' lists contain the suite's)
    exe, tmp = programs(name)
    ok = CHECKS[name].run(exe, tmp, *case)
    line = capfd.readouterr().out
    print(line, end="")
    assert ok and "BAD" not in line and "FAILED" not in line, line
    assert line.rstrip().endswith("ok"), line


@pytest.mark.parametrize("case", PREDICT_GRAD, ids=ident)
def test_predict_grad(programs, capfd, case):
    check(programs, capfd, "predict_grad", case)


@pytest.mark.parametrize("case", ARD_MATERN, ids=ident)
def test_ard_matern(programs, capfd, case):
    check(programs, capfd, "ard_matern", case)


@pytest.mark.parametrize("case", APPEND, ids=ident)
def test_append(programs, capfd, case):
    check(programs, capfd, "append", case)
