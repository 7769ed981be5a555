"""CPU checks of everything tests/test_gpu_append.py leans on (cugp_append, cugp_append_plan): the stand-in of the update
(tests/truth_append.py: standin_append, fp64 numpy / LAPACK in the order of the header's algebra) stays inside the bound on
every case, F_APPEND is what the project's rule gives on this BLAS or larger, two mutations of the algebra leave the bound by
orders of magnitude, the yardsticks of the cases used are sane -- and the passes the stand-in walks are the library's
(cugp_append_plan, replayed without a device).  No case is skipped.
"""
import ctypes as C

import numpy as np
import pytest

import accuracy
import truth
import truth_append as ta
from cugp_amd import capi

pytestmark = pytest.mark.skipif(not truth.EXTENDED, reason="numpy.longdouble is not an extended-precision type here")

IDS = [ta.case_id(c) for c in ta.CASES]


def library_plan(n, k):
    """The passes of cugp_append_plan (pure arithmetic: no device is touched)."""
    out = (C.c_int * 2)()
    count = capi.lib().cugp_append_plan(n, k, 0, out)
    assert count >= 1
    got = []
    for p in range(count):
        assert capi.lib().cugp_append_plan(n, k, p, out) == count
        got.append((out[0], out[1]))
    return got


@pytest.fixture(scope="module", autouse=True)
def plan_is_the_librarys():
    """Every (n, chunk) the cases append: truth_append.plan cuts where cugp_append_plan cuts."""
    for family, name, n0, chunks in ta.CASES:
        n = n0
        for k in chunks:
            assert ta.plan(n, k) == library_plan(n, k), (name, n, k)
            n += k
        assert n == truth.family_inputs(family, name)[0].shape[0]


@pytest.fixture(scope="module")
def table(oracle):
    """Stand-in ratios of every case, printed as the table of docs/ACCURACY.md."""
    out = {}
    for case in ta.CASES:
        r, rs = out[case] = ta.standin_ratios(oracle, case)
        print("STANDIN-APPEND %-34s " % ta.case_id(case) + "  ".join("%s %.2f" % kv for kv in list(r.items()) + list(rs.items())))
    return out


@pytest.mark.parametrize("case", ta.CASES, ids=IDS)
def test_standin_inside_the_bound(oracle, table, case):
    """cugp_append's algebra in fp64, LAPACK / BLAS order, against the live case's truth at all rows."""
    family = case[0]
    r, rs = table[case]
    assert max(r.values()) <= ta.F_APPEND[family], (case, r)
    assert max(rs.values()) <= ta.F_SOLVE, (case, rs)


def test_F_APPEND_covers_the_rule(table):
    """F_APPEND[family] >= truth.factor_rule(largest stand-in ratio over the family's cugp_append cases) and >= the family's
    own factor; alpha and K^-1 likewise against F_SOLVE.  The ratios are those of the BLAS this runs on."""
    own = {"se": truth.F, "ard": truth.F_ARD, "matern32": truth.F_MATERN, "matern52": truth.F_MATERN}
    worst, worst_solve = {}, 0.0
    for case, (r, rs) in table.items():
        fam = "matern" if case[0].startswith("matern") else case[0]
        worst[fam] = max(worst.get(fam, 0.0), max(r.values()))
        worst_solve = max(worst_solve, max(rs.values()))
    for fam, w in worst.items():
        key = "matern32" if fam == "matern" else fam
        print("cugp_append stand-in, %s: largest ratio %.2f -> rule %d (F_APPEND %d)" % (fam, w, truth.factor_rule(w), ta.F_APPEND[key]))
        assert truth.factor_rule(w) <= ta.F_APPEND[key], (fam, w)
        assert ta.F_APPEND[key] >= own[key]
    assert ta.F_APPEND["matern32"] == ta.F_APPEND["matern52"]
    print("alpha / K^-1: largest ratio %.2f -> rule %d (F_SOLVE %d)" % (worst_solve, truth.factor_rule(worst_solve), ta.F_SOLVE))
    assert truth.factor_rule(worst_solve) <= ta.F_SOLVE


@pytest.mark.parametrize("mutate", ["drop_qtq", "plus_q"])
def test_mutations_leave_the_bound(oracle, mutate):
    """cugp_append with K^-1's leading block left as it was, or with Q = +C^-1 V: far outside the bound (the test has teeth)."""
    # (Q = +C^-1 V on a single pass: a second pass on top of the wrong inverse would not even find S positive definite)
    family, name, n0, chunks = ta.CASES[2] if mutate == "drop_qtq" else ta.CASES[5]
    assert mutate == "drop_qtq" or len(ta.plan(n0, chunks[0])) == len(chunks) == 1
    c = accuracy.live(oracle, family, name)
    r, rs = ta.ratios(c, *ta.standin_append(c["cov"], c["X"], c["y"], c["Xt"], n0, chunks, mutate=mutate))
    worst = max(max(r.values()) / ta.F_APPEND[family], max(rs.values()) / ta.F_SOLVE)
    print("mutation %s: %.3g times the bound" % (mutate, worst))
    assert worst > 1e3, (mutate, r, rs)


def test_yardsticks_are_sane(oracle):
    """The live cases cugp_append's tests use: accuracy.assert_yardstick_is_sane on each."""
    for family, name in sorted({(c[0], c[1]) for c in ta.CASES}):
        accuracy.assert_yardstick_is_sane(accuracy.live(oracle, family, name), (family, name))
