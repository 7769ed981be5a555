"""The host check of the product of experts' gradient kernels as tests, without a GPU: cugp_amd/csrc/bcm_grad_device.h on
cov_device.h -- the text kernels.hip compiles for gfx950 -- behind tools/host_emul.h in a stand-alone program built with
-fsanitize=address,undefined (tools/bcm_predict_grad_host_check.cpp), every case of the script's list:

  grad    three experts of one padded size with n = 64, 64, 66 (1, 1 and 2 training tiles), nt = 65, d = 3 and 17, with and
          without V, SE-ARD / Matern-5/2-ARD / isotropic SE (d = 3 also with the two-tile expert first): every expert's slot carries the bits of the existing
          single-expert kernels run in the same emulation; NaN wherever the kernels must not read or write
          and at d = 3 three experts of 1, 2 and 63 rows (below one 64-row build tile) in one padded size
  reduce  k_poe_reduce_grad against cugp_poe_combine / cugp_poe_finish / cugp_poe_combine_grad, K = 1, 3, 5, world = 1, 2,
          nt = 1 and 257, all five modes, bit for bit in all four outputs

The program is built once per module.  A case fails on a non-zero exit, on anything a sanitizer writes to stderr, and on a
result that differs."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import host_check  # noqa: E402
import bcm_predict_grad_host_check as check  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists(host_check.CLANG), reason="no host compiler at " + host_check.CLANG)

ident = lambda case: "-".join(str(v) for v in case)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("bcm_predict_grad"))
    return host_check.build("bcm_predict_grad_host_check", tmp), tmp


@pytest.mark.parametrize("case", check.CASES, ids=ident)
def test_case(program, capfd, case):
    exe, tmp = program
    ok = check.run(exe, tmp, *case)
    line = capfd.readouterr().out
    print(line, end="")
    assert ok and "BAD" not in line and "FAILED" not in line, line
    assert line.rstrip().endswith("ok"), line
