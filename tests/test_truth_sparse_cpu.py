"""The CPU counterpart of tests/test_gpu_sparse.py: everything its accuracy bound rests on, without a GPU.

  - the truth's gradient (the G formulas, longdouble) against longdouble central differences of the DEFINITION of F
  - F <= the exact log marginal likelihood of the same data in every case, and F -> LL as Z = X, eps -> 0
  - the yardsticks are sane (no outlier among the permutations, under truth.YARDSTICK_CAP)
  - the stand-in -- the library's formulation, chunked by cugp_sparse_plan -- within F_SPARSE of the yardstick, and
    F_SPARSE is the larger of the family's factor and truth.factor_rule of the largest ratio measured here
  - two mutations of the stand-in leave the bound: F without its trace term, G_uf without the factor 2
  - cugp_sparse_plan replayed: every data row in exactly one chunk, every k of a Gram tile in exactly one split, ascending;
    the two default-chunk SE cases sit on the odd-stage, shorter-last-split shapes they were chosen for
  - beyond one test tile (tests/test_gpu_sparse_wide.py): at 129, 200 and 257 test points, and at the two-pass prediction's
    P + 129, the yardstick is sane and the stand-in within the family's factor, which truth.factor_rule confirms
"""
import numpy as np
import pytest

import truth
import truth_sparse as ts

LD = truth.LD
pytestmark = pytest.mark.skipif(not truth.EXTENDED, reason="numpy.longdouble is not an extended-precision type here")
NAMES = list(ts.CASES)
# central differences evaluate the N x N definition 2 nh times: every case of up to 300 rows (six evaluations of a
# 1300 x 1300 longdouble factorisation would take minutes; the gradients of the larger cases run through the same code as
# their families' small ones -- matern32_ard_n257_m64 is there for matern32_ard_n1000_m130)
CD_NAMES = [n for n in NAMES if ts.CASES[n][1] <= 300]


@pytest.mark.parametrize("name", CD_NAMES)
def test_truth_gradient_against_central_differences(name):
    X, y, Z, _, cov, _ = ts.inputs(name)
    t = ts.case(name)["t"]
    make = truth.FAMILIES[ts.CASES[name][0]][1]
    h = 1e-6
    worst = 0.0
    for j in range(len(cov.hp)):
        f = []
        for sgn in (1, -1):
            c = make(list(cov.hp))
            # the shifted hyper-parameter in longdouble: the descriptor's scalars are recomputed from it
            th = LD(cov.hp[j]) + sgn * LD(h)
            if hasattr(c, "w") and j < len(c.w):
                c.w[j] = np.exp(-th)
            elif j == len(cov.hp) - 2:
                c.sf2 = np.exp(2 * th)
            elif j == len(cov.hp) - 1:
                c.sn2 = np.exp(2 * th)
            else:
                c.l2 = np.exp(2 * th)
            f.append(ts.bound_definition(X, y, Z, c))
        cd = -(f[0] - f[1]) / (2 * LD(h))
        worst = max(worst, float(abs(cd - t.grad[j]) / np.max(np.abs(t.grad))))
    print("CD %-24s max |central difference - truth| / max|g| = %.2e" % (name, worst))
    assert worst <= 1e-9            # h^2 truncation of a smooth function at h = 1e-6, longdouble rounding 1e-19 / h


@pytest.mark.parametrize("name", NAMES)
def test_bound_is_below_the_exact_log_marginal_likelihood(name):
    """truth.Truth's ll uses the literal 1.83787 for log 2 pi; F uses log 2 pi itself: the comparison is made on the same
    constant (the literal is the larger, so F <= ll holds with it too)."""
    c = ts.case(name)
    t = truth.Truth(c["X"], c["y"], c["cov"], keep=False)
    ll = t.ll + len(c["y"]) * (LD(truth.LL_CONST) - ts.LOG2PI) / 2
    print("BOUND %-24s F %.9f  LL %.9f  gap %.3e" % (name, float(c["t"].F), float(ll), float(ll - c["t"].F)))
    assert c["t"].F <= ll
    assert c["t"].F <= t.ll


def test_bound_tends_to_the_log_marginal_likelihood():
    """Z = X: Qff = Kff (Kff + eps I)^-1 Kff -> Kff and the trace term -> 0 as eps -> 0."""
    X, y = ts.synth(24, d=2, seed=74, scale=4.0)
    cov = truth.SE(list(ts.HP_DEFAULT))
    ll = truth.Truth(X, y, cov, keep=False).ll + len(y) * (LD(truth.LL_CONST) - ts.LOG2PI) / 2
    gaps = [float(ll - ts.bound_definition(X, y, X, cov, jitter=eps)) for eps in (1e-2, 1e-4, 1e-6, 1e-8)]
    print("LIMIT gaps", gaps)
    assert all(g >= 0 for g in gaps) and all(b < a for a, b in zip(gaps, gaps[1:]))
    assert gaps[-1] <= 1e-6 * abs(float(ll))


@pytest.mark.parametrize("name", NAMES)
def test_yardstick_is_sane(name):
    c = ts.case(name)
    print("YARD %-24s " % name + "  ".join("%s %.2e" % (q, c["noise"][q]) for q in c["cov"].quantities))
    ts.assert_yardstick_is_sane(c, name)


_RATIOS = {}


def standin_ratios(name):
    if name not in _RATIOS:
        c = ts.case(name)
        _RATIOS[name] = ts.ratios(c, ts.standin(c["cov"], c["X"], c["y"], c["Z"], c["Xt"], c["chunk"]))
    return _RATIOS[name]


@pytest.mark.parametrize("name", NAMES)
def test_standin_within_the_bound(name):
    r = standin_ratios(name)
    print("STANDIN %-24s " % name + "  ".join("%s %.2f" % kv for kv in r.items()))
    assert max(r.values()) <= ts.F_SPARSE[ts.CASES[name][0]], r


def test_factors_follow_the_rule():
    """F_SPARSE[family] is the larger of the family's existing factor and truth.factor_rule of the largest stand-in ratio
    over its cases: the rule's value is at most F_SPARSE, and F_SPARSE at least the existing factor (the ratios are those of
    the BLAS this runs on)."""
    worst = {}
    for name in NAMES:
        fam = ts.CASES[name][0]
        worst[fam] = max(worst.get(fam, 0.0), max(standin_ratios(name).values()))
    for fam, w in worst.items():
        rule = truth.factor_rule(w)
        print("F_SPARSE %-12s largest stand-in ratio %.2f  factor_rule %d  existing %d  F_SPARSE %d"
              % (fam, w, rule, ts.EXISTING[fam], ts.F_SPARSE[fam]))
        assert rule <= ts.F_SPARSE[fam], (fam, w, rule)
        assert ts.F_SPARSE[fam] >= ts.EXISTING[fam], fam
    assert set(worst) == set(ts.F_SPARSE)                        # every family has a case of its own


@pytest.mark.parametrize("mutate, quantity", [("drop_tr", 0), ("guf_without_2", 1)])
@pytest.mark.parametrize("name", ["se_n300_m65", "ard_n300_m130_d17"])
def test_mutations_leave_the_bound(name, mutate, quantity):
    """F without its trace term moves F; G_uf without the factor 2 moves the length-scale components."""
    c = ts.case(name)
    r = ts.ratios(c, ts.standin(c["cov"], c["X"], c["y"], c["Z"], c["Xt"], c["chunk"], mutate=mutate))
    q = c["cov"].quantities[quantity]
    print("MUTATION %-24s %-14s %s ratio %.3g" % (name, mutate, q, r[q]))
    assert r[q] > 1000 * ts.F_SPARSE[c["family"]]


@pytest.mark.parametrize("n, m, chunk_rows", [(128, 128, 128), (300, 65, 128), (1300, 200, 512), (300, 130, 256),
                                              (257, 64, 128), (5000, 1024, 0), (100000, 2048, 0), (70000, 128, 16384),
                                              (800, 65, 0), (1000, 130, 896), (1300, 260, 0)])
def test_plan_covers_rows_and_k_once(n, m, chunk_rows):
    passes = ts.plan(n, m, chunk_rows)
    rows = np.zeros(n, dtype=int)
    nxt = 0
    for r0, cnt, cpad, split, kstep in passes:
        assert r0 == nxt and cnt > 0 and cpad % 128 == 0 and cnt <= cpad < cnt + 128
        assert chunk_rows == 0 or cnt <= chunk_rows
        rows[r0: r0 + cnt] += 1
        nxt = r0 + cnt
        ks = np.zeros(cpad, dtype=int)
        assert split >= 1 and kstep % 16 == 0
        for s in range(split):
            k0, k1 = s * kstep, min((s + 1) * kstep, cpad)
            assert k0 < k1                                   # ascending, no empty split
            ks[k0: k1] += 1
        assert np.all(ks == 1)
    assert nxt == n and np.all(rows == 1)


def test_plan_splits_where_the_cases_say():
    assert [p[3] for p in ts.plan(1300, 200, 512)] == [2, 2, 1]          # three output tiles: the 512-row chunks split in 2
    assert [p[1] for p in ts.plan(300, 65, 128)] == [128, 128, 44]
    assert all(p[3] == 1 for p in ts.plan(300, 65, 128))
    # the two default-chunk SE cases: an odd stage count (304 / 16 = 19) with a shorter last split; five splits of 18, 18,
    # 18, 18 and 16 stages -- a change of the split rule must not move them off these paths silently
    for name, want in (("se_n800_m65_d3_c0", (0, 800, 896, 3, 304)), ("se_n1300_m260_c0", (0, 1300, 1408, 5, 288))):
        _, N, M, _, chunk = ts.CASES[name][:5]
        assert chunk == 0 and ts.plan(N, M, chunk) == [want], name
    assert [min(304, 896 - s * 304) // 16 for s in range(3)] == [19, 19, 18]
    assert [min(288, 1408 - s * 288) // 16 for s in range(5)] == [18, 18, 18, 18, 16]
    assert ts.plan(1000, 130, 896) == [(0, 896, 896, 3, 304), (896, 104, 128, 1, 128)]


# ------------------------------------------------------------------ beyond one test tile (tests/test_gpu_sparse_wide.py)
WIDE = [(name, nt) for name in ts.WIDE_NAMES for nt in ts.WIDE_NTS]
_WIDE_RATIOS = {}


def wide_standin_ratios(name, nt):
    if (name, nt) not in _WIDE_RATIOS:
        c, w = ts.case(name), ts.wide_case(name, nt)
        out = ts.standin(c["cov"], c["X"], c["y"], c["Z"], w["Xt"], c["chunk"])
        _WIDE_RATIOS[name, nt] = ts.wide_ratios(c, w, out[2], out[3])
    return _WIDE_RATIOS[name, nt]


@pytest.mark.parametrize("name, nt", WIDE)
def test_wide_points_yardstick_and_standin(name, nt):
    """At 129, 200 and 257 test points: the training row and the inducing input are where the GPU test needs them, the
    yardstick is sane under truth_sparse.assert_yardstick_is_sane's two conditions, and the stand-in stays within the
    family's factor."""
    c, w = ts.case(name), ts.wide_case(name, nt)
    Xt = w["Xt"]
    assert Xt.shape == (nt, c["X"].shape[1]) and ts.WIDE_Z_ROW >= 128
    assert np.array_equal(Xt[ts.WIDE_Z_ROW], c["Z"][0]) and np.array_equal(Xt[nt - 2], c["X"][len(c["X"]) // 2])
    for q in ("mean", "var"):
        assert w["first"][q] <= c["cov"].F * max(w["rest"][q], c["floor"][q]), (name, nt, q, w["first"][q], w["rest"][q])
        assert w["noise"][q] <= truth.YARDSTICK_CAP * c["floor"][q] / truth.U4, (name, nt, q, w["noise"][q])
    r = wide_standin_ratios(name, nt)
    print("STANDIN-WIDE %-24s nt %-3d " % (name, nt) + "  ".join("%s %.2f (yardstick %.2e)" % (q, v, w["noise"][q])
                                                                for q, v in r.items()))
    assert max(r.values()) <= ts.F_SPARSE[c["family"]], r


def test_wide_factors_follow_the_rule():
    worst = {}
    for name, nt in WIDE:
        fam = ts.CASES[name][0]
        worst[fam] = max(worst.get(fam, 0.0), max(wide_standin_ratios(name, nt).values()))
    for fam, w in worst.items():
        rule = truth.factor_rule(w)
        print("F_SPARSE wide %-12s largest stand-in ratio %.2f  factor_rule %d  F_SPARSE %d" % (fam, w, rule, ts.F_SPARSE[fam]))
        assert rule <= ts.F_SPARSE[fam], (fam, w, rule)


def test_two_pass_prediction_yardstick_and_standin():
    """The prediction that takes two passes (tests/test_gpu_sparse_wide.py): nt = P + 129 with P cugp_sparse_predict_plan's
    first pass; the row behind the pass boundary is Z[0], the one before it a data row; yardstick and stand-in on ALL rows."""
    import cugp_amd.gp as gp
    name = ts.TWO_PASS_NAME
    c = ts.case(name)
    P = gp.sparse_predict_plan(ts.CASES[name][2], 1 << 30)[0][1]
    nt = P + 129
    assert P == 349440 and gp.sparse_predict_plan(ts.CASES[name][2], nt) == [(0, P), (P, 129)]
    w = ts.wide_case(name, nt, z_row=P, data_row=P - 1)
    assert np.array_equal(w["Xt"][P], c["Z"][0]) and np.any(np.all(c["X"] == w["Xt"][P - 1], axis=1))
    for q in ("mean", "var"):
        assert w["first"][q] <= c["cov"].F * max(w["rest"][q], c["floor"][q]), (q, w["first"][q], w["rest"][q])
        assert w["noise"][q] <= truth.YARDSTICK_CAP * c["floor"][q] / truth.U4, (q, w["noise"][q])
    out = ts.standin(c["cov"], c["X"], c["y"], c["Z"], w["Xt"], c["chunk"])
    r = ts.wide_ratios(c, w, out[2], out[3])
    print("STANDIN-TWO-PASS %s nt %d " % (name, nt) + "  ".join("%s %.2f (yardstick %.2e)" % (q, v, w["noise"][q])
                                                               for q, v in r.items()))
    assert truth.factor_rule(max(r.values())) <= ts.F_SPARSE[c["family"]], r
