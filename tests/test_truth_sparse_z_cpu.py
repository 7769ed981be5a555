"""The CPU counterpart of tests/test_gpu_sparse_z.py: everything its accuracy bound rests on, without a GPU.

  - the truth of gZ (the formula, longdouble, explicit G_uf and G_uu) against longdouble central differences of the
    DEFINITION of F (truth_sparse.bound_definition) in Z
  - the yardsticks are sane (no outlier among the permutations, under truth.YARDSTICK_CAP)
  - the stand-in -- the library's formulation, chunked by cugp_sparse_plan -- within F_SPARSE_Z of the yardstick, and
    F_SPARSE_Z is the larger of F_SPARSE and truth.factor_rule of the largest ratio measured here
  - three mutations of the stand-in leave the bound: the square term weighed 1/2, the rank-one part dropped, dimension 0's
    s_c for every dimension of the ARD case
"""
import numpy as np
import pytest

import truth
import truth_sparse as ts
import truth_sparse_z as tz

LD = truth.LD
pytestmark = pytest.mark.skipif(not truth.EXTENDED, reason="numpy.longdouble is not an extended-precision type here")
NAMES = list(tz.CASES)
# central differences evaluate the N x N definition twelve times: every case but the 1300-row one (a 1300 x 1300 longdouble
# factorisation takes most of a minute; its gradient runs through the same code as the other SE cases)
CD_NAMES = [n for n in NAMES if tz.CASES[n][1] <= 300]
CD_SAMPLE = 6


@pytest.mark.parametrize("name", CD_NAMES)
def test_truth_against_central_differences(name):
    X, y, Z, cov, _ = tz.inputs(name)
    t = tz.case(name)["tz"]
    h = 1e-5
    rng = np.random.default_rng(CD_SAMPLE + len(y) + Z.shape[1])
    flat = rng.choice(Z.size, CD_SAMPLE, replace=False)
    worst = 0.0
    for e in flat:
        j, c = divmod(int(e), Z.shape[1])
        f, at = [], []
        for sgn in (1, -1):
            Zs = np.array(Z, dtype=np.float64)
            Zs[j, c] += sgn * h                                  # (fp64, as the definition takes it: the step is what was stored)
            at.append(LD(Zs[j, c]))
            f.append(ts.bound_definition(X, y, Zs, cov))
        cd = -(f[0] - f[1]) / (at[0] - at[1])
        worst = max(worst, float(abs(cd - t[j, c]) / np.max(np.abs(t))))
    print("CD-Z %-24s max |central difference - truth| / max|gZ| = %.2e" % (name, worst))
    assert worst <= 1e-9            # h^2 truncation of a smooth function at h = 1e-5, longdouble rounding 1e-19 / h


@pytest.mark.parametrize("name", NAMES)
def test_yardstick_is_sane(name):
    c = tz.case(name)
    print("YARD-Z %-24s gZ %.2e (as given %.2e, permutations %.2e)" % (name, c["noise"], c["first"], c["rest"]))
    tz.assert_yardstick_is_sane(c, name)


_RATIOS = {}


def standin_ratio(name):
    if name not in _RATIOS:
        c = tz.case(name)
        _RATIOS[name] = tz.ratio(c, tz.standin_gz(c["cov"], c["X"], c["y"], c["Z"], c["chunk"]))
    return _RATIOS[name]


@pytest.mark.parametrize("name", NAMES)
def test_standin_within_the_bound(name):
    r = standin_ratio(name)
    print("STANDIN-Z %-24s gZ %.2f" % (name, r))
    assert r <= tz.F_SPARSE_Z[tz.CASES[name][0]], r


def test_factors_follow_the_rule():
    worst = {}
    for name in NAMES:
        fam = tz.CASES[name][0]
        worst[fam] = max(worst.get(fam, 0.0), standin_ratio(name))
    for fam, w in worst.items():
        rule = truth.factor_rule(w)
        print("F_SPARSE_Z %-12s largest stand-in ratio %.2f  factor_rule %d  F_SPARSE %d  F_SPARSE_Z %d"
              % (fam, w, rule, ts.F_SPARSE[fam], tz.F_SPARSE_Z[fam]))
        assert rule <= tz.F_SPARSE_Z[fam], (fam, w, rule)
        assert tz.F_SPARSE_Z[fam] >= ts.F_SPARSE[fam], fam
    assert set(worst) == set(tz.F_SPARSE_Z)                      # every family has a case of its own


@pytest.mark.parametrize("name, mutate", [("se_n300_m65_d3", "square_half"), ("se_n300_m65_d3", "no_rank_one"),
                                          ("ard_n300_m130_d17", "square_half"), ("ard_n300_m130_d17", "no_rank_one"),
                                          ("ard_n300_m130_d17", "s0_for_all")])
def test_mutations_leave_the_bound(name, mutate):
    c = tz.case(name)
    r = tz.ratio(c, tz.standin_gz(c["cov"], c["X"], c["y"], c["Z"], c["chunk"], mutate=mutate))
    print("MUTATION-Z %-24s %-12s gZ ratio %.3g" % (name, mutate, r))
    assert r > 1000 * tz.F_SPARSE_Z[c["family"]]


def test_row_ranges_where_the_cases_say():
    """The Z pass's row ranges of the default-chunk cases are ragged -- 5, 5, 4 and 5, 5, 5, 5, 2 tiles --, those of the
    earlier cases equal; the replay's constant is the library's."""
    import os
    import re
    from conftest import ROOT
    with open(os.path.join(ROOT, "cugp_amd", "csrc", "kernels.h")) as f:
        assert int(re.search(r"constexpr int SPARSE_Z_SLOTS = (\d+);", f.read()).group(1)) == tz.Z_SLOTS

    def of(name):
        _, N, M, d, chunk, _ = tz.CASES[name]
        return [tz.z_ranges(p[2], -(-M // 128) * 128, d) for p in ts.plan(N, M, chunk)]
    assert of("se_n800_m65_d3_c0") == of("matern52_n800_m65_d3_c0") == [[5, 5, 4]]
    assert of("se_n1300_m260_c0") == [[5, 5, 5, 5, 2]]
    assert of("matern32_ard_n1000_m130") == [[5, 5, 4], [2]]
    assert of("se_n1300_m200") == [[4, 4], [4, 4], [6]] and of("se_n300_m65_d3") == [[2], [2], [2]]
    assert tz.z_ranges(384, 384, 6) == [6]                       # the square of mpad 384: six column tiles, one range


def test_the_cases_and_what_is_left_out():
    assert set(tz.MUTATIONS) == {"square_half", "no_rank_one", "s0_for_all"}
    assert {tz.CASES[n][0] for n in NAMES} == {"se", "matern32", "matern52", "ard", "matern32_ard", "matern52_ard"}
    for left_out in ("se_n300_m65", "se_n300_dup60", "se_n128_m128"):
        assert left_out in ts.CASES and left_out not in tz.CASES and left_out in tz.__doc__
