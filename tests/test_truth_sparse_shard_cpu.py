"""The CPU counterpart of tests/test_gpu_sparse_shard.py: everything its accuracy bound rests on, without a GPU.

  - the stand-in with the sums in global shard order (truth_sparse_shard.standin_sharded) within
    F_SPARSE[family] max(yardstick, 4 ulp) of the truth of the truth_sparse case it is built over, every case of SHARD_CASES;
    the largest ratio per family is printed (docs/ACCURACY.md: the table)
  - F_SPARSE_SHARD is the larger of F_SPARSE and truth.factor_rule of the largest ratio measured here -- never the GPU's
  - one shard: the stand-in is truth_sparse.standin bit for bit
  - two mutations leave the bound: y'y without one shard, S_uf with the last shard added twice
"""
import numpy as np
import pytest

import truth
import truth_sparse as ts
import truth_sparse_shard as tsh

pytestmark = pytest.mark.skipif(not truth.EXTENDED, reason="numpy.longdouble is not an extended-precision type here")
IDS = [tsh.case_id(sc) for sc in tsh.SHARD_CASES]
_RATIOS = {}


def standin(sc, mutate=None):
    shards, Z, Xt, cov, chunk = tsh.shards_of(*sc)
    return tsh.standin_sharded(cov, shards, Z, Xt, chunk, mutate=mutate)


def ratios(sc):
    if sc not in _RATIOS:
        _RATIOS[sc] = ts.ratios(ts.case(sc[0]), standin(sc))
    return _RATIOS[sc]


def test_the_cases_are_the_issues():
    assert dict((tsh.case_id(sc), sc[1]) for sc in tsh.SHARD_CASES) == {
        "se_n300_m65-171_128_1": (171, 128, 1), "se_n300_m65-300": (300,), "se_n128_m128-26_26_26_26_24": (26, 26, 26, 26, 24),
        "se_n1300_m200-700_600": (700, 600), "ard_n300_m130_d17-129_127_44": (129, 127, 44),
        "matern32_ard_n1000_m130-900_100": (900, 100), "matern52_n800_m65_d3_c0-400_400": (400, 400),
        "se_n300_dup60-150_150": (150, 150)}
    for name, counts in tsh.SHARD_CASES:
        assert sum(counts) == ts.CASES[name][1]
    # two passes in shard 0 of the Matern-3/2-ARD case, split-k inside a shard of the 1300-row case
    assert len(ts.plan(900, 130, ts.CASES["matern32_ard_n1000_m130"][4])) == 2
    assert max(p[3] for p in ts.plan(700, 200, ts.CASES["se_n1300_m200"][4])) >= 2


@pytest.mark.parametrize("sc", tsh.SHARD_CASES, ids=IDS)
def test_standin_within_the_bound(sc):
    r = ratios(sc)
    fam = ts.CASES[sc[0]][0]
    print("STANDIN-SHARD %-34s " % tsh.case_id(sc) + "  ".join("%s %.2f" % kv for kv in r.items()))
    assert max(r.values()) <= ts.F_SPARSE[fam], r
    assert max(r.values()) <= tsh.F_SPARSE_SHARD[fam], r


def test_factors_follow_the_rule():
    worst = {}
    for sc in tsh.SHARD_CASES:
        fam = ts.CASES[sc[0]][0]
        worst[fam] = max(worst.get(fam, 0.0), max(ratios(sc).values()))
    for fam, w in worst.items():
        rule = truth.factor_rule(w)
        print("F_SPARSE_SHARD %-12s largest stand-in ratio %.2f  factor_rule %d  F_SPARSE %d  F_SPARSE_SHARD %d"
              % (fam, w, rule, ts.F_SPARSE[fam], tsh.F_SPARSE_SHARD[fam]))
        assert tsh.F_SPARSE_SHARD[fam] == max(ts.F_SPARSE[fam], rule)
    assert tsh.F_SPARSE_SHARD_Z == dict(tsh.tz.F_SPARSE_Z)


@pytest.mark.parametrize("name", ["se_n300_m65", "se_n1300_m200", "matern32_ard_n1000_m130"])
def test_one_shard_is_the_plain_standin_bit_for_bit(name):
    X, y, Z, Xt, cov, chunk = ts.inputs(name)
    a = tsh.standin_sharded(cov, [(X, y)], Z, Xt, chunk)
    b = ts.standin(cov, X, y, Z, Xt, chunk)
    for u, v in zip(a, b):
        u, v = np.atleast_1d(np.asarray(u, dtype=np.float64)), np.atleast_1d(np.asarray(v, dtype=np.float64))
        assert np.array_equal(u.view(np.uint64), v.view(np.uint64))


@pytest.mark.parametrize("mutate", tsh.MUTATIONS)
def test_mutations_are_caught(mutate):
    sc = tsh.SHARD_CASES[0]                                           # (171, 128, 1): the last shard is ONE row
    c = ts.case(sc[0])
    r = ts.ratios(c, standin(sc, mutate))
    print("MUTATION-SHARD %-22s " % mutate + "  ".join("%s %.2g" % kv for kv in r.items()))
    assert max(r.values()) > tsh.F_SPARSE_SHARD[ts.CASES[sc[0]][0]], r
