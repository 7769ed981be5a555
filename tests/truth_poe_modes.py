"""Truth, yardstick, stand-in and bound of the combination rules on latent expert distributions (include/cugp.h:
CUGP_COMBINE_*) -- TEST INFRASTRUCTURE, CPU, numpy only; a plain module beside tests/truth.py and tests/accuracy.py,
which it imports and leaves as they are.

Per test point, experts k = 0..K-1 over truth.bcm_rows' split, p_k = 1 / var_f,k, pm_k = m_k / var_f,k:

    beta_k = 1 (poe, bcm) | 1 / K (gpoe) | 1/2 log(sf2 p_k) (rbcm)
    prec   = sum beta_k p_k  (+ (1 - sum beta_k) / sf2 for bcm, rbcm)
    var_f  = 1 / prec,  mean = var_f sum beta_k pm_k

  truth      every expert's truth.Truth, its latent variance computed DIRECTLY as sf2 - sum Wt^2 from Truth._cross, the
             rule in numpy.longdouble (`combine` at longdouble inputs)
  yardstick  the family's own fp64 evaluator per expert (SE: the CPU oracle; ARD: the oracle on the scaled copy; Matern:
             its fp64 K through the oracle's factorisation), combined in fp64 in expert order, over the data as given and
             the 7 permutations inside each expert's rows (truth.noise_level with `parts`).  The evaluator returns the
             NOISY variance, so the yardstick's latent variance is that minus sn2 in fp64: a subtraction the library never
             makes (it forms sf2 - |W_t|^2 directly).  This OVER-estimates the rounding the library can be held to, it
             does not under-estimate it: the yardstick carries the rounding of sf2 + sn2 - q and of the subtraction on top
             of everything the direct form has.
  stand-in   a CPU fp64 restatement of exactly the library's formulation (LAPACK / BLAS order per expert as
             truth.standin, the latent variance direct, rows 1 / v and (1 / v) m, then the sums above one operation at a
             time) -- what sets the factor, never the GPU
  bound      err <= F_family max(yardstick, floor), floors as truth.floors (4 ulp of max|mean| and of sf2 + sn2)

The factor: truth.F, F_MATERN, F_ARD as they stand where the stand-in stays at or below half of them on every case of the
GPU list; tests/test_truth_poe_modes_cpu.py measures that and docs/ACCURACY.md records the ratios.  F_COMBINE (None: not
needed) would replace them by truth.factor_rule of the largest ratio.
"""
import numpy as np

import truth
from conftest import synth

LD = truth.LD
MODES = ("poe", "gpoe", "bcm", "rbcm")
F_COMBINE = None                  # a factor of its own is not needed: the largest stand-in ratio is below F / 2 (docs/ACCURACY.md)

HP = truth.HP_BCM_WIDE            # [0.9, 0.2, -1.0]
HP_ARD = [0.9, 0.3, 1.6, 0.2, -1.0]
D = 3
SCALE = 3.0
NTS = (1, 255, 256, 257)          # the 256-thread boundary of the reduce; the second 128-row test tile
NT_FAMILY = truth.WIDE_NT_FAMILY  # 200

# name -> (family, rows, experts, test-point counts): the GPU case list (tests/test_gpu_poe_modes.py) and the CPU
# counterpart's.  truth.WIDE_BCM: three equal experts, and the uneven split (experts padded to a common size).
CASES = {
    "se_3x300": ("se", truth.WIDE_BCM[0][0], truth.WIDE_BCM[0][1], NTS),
    "se_5x261p2": ("se", truth.WIDE_BCM[1][0], truth.WIDE_BCM[1][1], NTS),
    "se_1x257": ("se", 257, 1, (1, 257)),
    "matern52_3x300": ("matern52", 900, 3, (NT_FAMILY,)),
    "ard_3x300": ("ard", 900, 3, (NT_FAMILY,)),
}
CASE_LIST = [(name, nt) for name, c in CASES.items() for nt in c[3]]


def descriptor(family):
    if family == "ard":
        return truth.ARD(HP_ARD)
    return truth.FAMILIES[family][1](HP)


def factor(cov):
    return cov.F if F_COMBINE is None else F_COMBINE


def inputs(name, nt):
    """-> (X, y, Xt, cov, K): synth data in the box, nt test points in it (the last but one a training row, nt > 1)."""
    family, N, K, _ = CASES[name]
    X, y = synth(N, d=D, seed=N + K, scale=SCALE)
    Xt = synth(nt, d=D, seed=7, scale=SCALE)[0]
    if nt > 1:
        Xt[truth.WIDE_TRAINING_ROW] = X[N // 2]
    return X, y, np.ascontiguousarray(Xt), descriptor(family), K


def rows_of(c):
    """The experts' [(offset, rows)] of a case: its own "parts" (explicit rows: tests/truth_small_bcm.py), else the
    reference's split of len(y) into K."""
    return c["parts"] if "parts" in c else truth.bcm_rows(len(c["y"]), c["K"])


def combine(m, v, mode, sf2, half=True, prior=True):
    """The rule `mode` on per-expert latent means m[K][nt] and variances v[K][nt], in the arrays' own precision, experts
    in order, one operation at a time -> (mean, var_f).  half / prior: the mutations of the CPU test (beta without the
    1/2; the prior term dropped)."""
    m, v = np.asarray(m), np.asarray(v)
    one = v.dtype.type(1)
    sf2 = v.dtype.type(sf2)
    K = len(v)
    sp = spm = sb = np.zeros(v.shape[1], dtype=v.dtype)
    for k in range(K):
        p = one / v[k]
        pm = p * m[k]
        if mode == "gpoe":
            beta = np.full_like(p, one / v.dtype.type(K))
        elif mode == "rbcm":
            beta = (v.dtype.type(0.5) if half else one) * np.log(sf2 * p)
        else:
            beta = np.ones_like(p)
        sp, spm, sb = sp + beta * p, spm + beta * pm, sb + beta
    prec = sp + (one - sb) / sf2 if (mode in ("bcm", "rbcm") and prior) else sp
    tv = one / prec
    return tv * spm, tv


# ------------------------------------------------------------------ truth
_EXPERTS = {}


def expert_truths(name):
    """The experts' truth.Truth of a case, computed once (they do not depend on the test points)."""
    if name not in _EXPERTS:
        X, y, _, cov, K = inputs(name, 1)
        _EXPERTS[name] = [truth.Truth(X[o: o + r], y[o: o + r], cov, keep=False) for o, r in truth.bcm_rows(len(y), K)]
    return _EXPERTS[name]


def latent(t, Xt):
    """(mean, var_f) of one expert's truth: var_f = sf2 - sum Wt^2, directly."""
    _, Ks, Wt = t._cross(Xt)
    return Ks @ t.alpha, t.sf2 - (Wt * Wt).sum(1)


def truth_case(name, nt):
    """-> dict(X, y, Xt, cov, K, experts=[(m_k, v_k)] in longdouble, modes={mode: (mean, var_f)} in longdouble)."""
    X, y, Xt, cov, K = inputs(name, nt)
    ex = [latent(t, Xt) for t in expert_truths(name)]
    m, v = np.array([e[0] for e in ex], dtype=LD), np.array([e[1] for e in ex], dtype=LD)
    return dict(X=X, y=y, Xt=Xt, cov=cov, K=K, experts=ex, modes={mode: combine(m, v, mode, cov.sf2) for mode in MODES})


# ------------------------------------------------------------------ yardstick
def yardsticks(oracle, c):
    """-> {mode: {"mean": ., "var": .}}: truth.noise_level of the fp64 evaluator per expert, latent variance = noisy - sn2
    in fp64, combined in fp64 in expert order, the rows permuted inside their own expert."""
    cov, K = c["cov"], c["K"]
    parts = rows_of(c)
    Xe, ev = cov.evaluator(oracle, c["X"], c["Xt"])
    c64 = cov.fp64()
    nh = len(cov.hp)
    seen = {}

    def experts(Xp, yp):
        key = hash(Xp.tobytes())
        if key not in seen:
            out = [ev(np.ascontiguousarray(Xp[o: o + r]), np.ascontiguousarray(yp[o: o + r]))[2:4] for o, r in parts]
            seen[key] = (np.array([o[0] for o in out]), np.array([o[1] - c64.sn2 for o in out]))
        return seen[key]

    out = {}
    for mode in MODES:
        def evaluate(Xp, yp, mode=mode):
            m, v = experts(Xp, yp)
            return (1.0, np.ones(nh)) + combine(m, v, mode, c64.sf2)
        tm, tv = c["modes"][mode]
        noise = truth.noise_level(cov, evaluate, Xe, c["y"], LD(1), np.ones(nh, dtype=LD), tm, tv, parts=parts)[0]
        out[mode] = dict(mean=noise["mean"], var=noise["var"])
    # every expert's own latent prediction under the same evaluations: the yardstick of cugp_predict_latent
    out["experts"] = [truth.errors_pred(*[np.array([s[i][k] for s in seen.values()]) for i in (0, 1)],
                                        c["experts"][k][0][None, :], c["experts"][k][1][None, :]) for k in range(K)]
    return out


_CASES = {}


def case(oracle, name, nt):
    """truth_case with its yardsticks under "yard", computed once per process."""
    if (name, nt) not in _CASES:
        c = truth_case(name, nt)
        c["yard"] = yardsticks(oracle, c)
        _CASES[name, nt] = c
    return _CASES[name, nt]


def expert_floors(c, k):
    cov = c["cov"]
    return dict(mean=truth.U4 * float(np.max(np.abs(c["experts"][k][0]))),
                var=truth.U4 * float(np.exp(2 * cov.hp[-2]) + np.exp(2 * cov.hp[-1])))


def floors(c, mode):
    cov = c["cov"]
    sc = truth.scales(cov, 1.0, np.ones(len(cov.hp)), c["modes"][mode][0])
    fl = truth.floors(cov, sc)
    return dict(mean=fl["mean"], var=fl["var"])


# ------------------------------------------------------------------ stand-in
def standin_experts(c, noisy_rows=False):
    """Per expert (m, var_f) in fp64, LAPACK / BLAS order (truth.standin's), the latent variance direct; noisy_rows: the
    mutation that leaves sn2 in the experts' variances."""
    import scipy.linalg as sl
    c64 = c["cov"].fp64()
    Xt = np.asarray(c["Xt"], dtype=np.float64)
    ms, vs = [], []
    for o, r in rows_of(c):
        X, y = c["X"][o: o + r], c["y"][o: o + r]
        Kf, _ = c64.train(X)
        L = np.linalg.cholesky(Kf + c64.sn2 * np.eye(r))
        T = sl.solve_triangular(L, np.eye(r), lower=True)
        a = (T.T @ T) @ y
        Ks = c64.k(Xt, X)
        Wt = Ks @ T.T
        ms.append(Ks @ a)
        vs.append((c64.sf2 + c64.sn2 if noisy_rows else c64.sf2) - (Wt * Wt).sum(1))
    return np.array(ms), np.array(vs)


def standin(c, mode, half=True, prior=True, noisy_rows=False):
    m, v = standin_experts(c, noisy_rows)
    return combine(m, v, mode, c["cov"].fp64().sf2, half, prior)


MUTATIONS = {"beta_without_half": dict(half=False), "prior_term_dropped": dict(prior=False),
             "sn2_left_in_rows": dict(noisy_rows=True)}


def ratios(c, yard, mode, mean, var):
    """err / max(yardstick, floor) of a (mean, var_f) against the truth of `mode`, per quantity."""
    e = truth.errors_pred(mean, var, *c["modes"][mode])
    fl = floors(c, mode)
    return {q: e[q] / max(yard[mode][q], fl[q]) for q in ("mean", "var")}
