"""The cases, the yardstick and the float32 restatement of the matrix-free GP's fp32 product (cugp_iter_apply32; DESIGN.md
section 36, docs/ACCURACY.md "The fp32 product").  The truth is K V in numpy.longdouble from truth.py's evaluators; the
yardstick of output row i is  Y_i = u32 sum_j (1 + |log g_ij| + sqrt(s_ij) m_ij) |k_ij| |v_j|  with u32 = 2^-24, g = k / sf2,
s the weighted squared distance and m_ij = max over the two rows and the features of |x_c w_c|; the bound is F_MIX Y_i."""
import functools

import numpy as np

import truth
import truth_ard_matern as tam
import truth_rq as trq
from conftest import synth

LD, U32 = truth.LD, 2.0 ** -24
# The largest |restate32 - truth| / Y over PRODUCT below is 1.32 (test_iter_mixed_api.py computes it on the CPU); the next
# power of two, times 2.  The largest ratio an MI355X showed over the same cases: see docs/ACCURACY.md.
F_MIX = 4.0


def _ls(d):
    return np.linspace(0.7, 1.3, d).tolist()


# family -> (kernel=, one length scale per dimension, d -> theta, theta -> truth descriptor)
FAMILIES = {
    "se": ("se", False, lambda d: [0.9, 0.2, -1.0], truth.SE),
    "se_ard": ("se", True, lambda d: _ls(d) + [0.2, -1.0], truth.ARD),
    "matern32": ("matern32", False, lambda d: [0.9, 0.2, -1.0], lambda hp: truth.Matern(hp, 1)),
    "matern32_ard": ("matern32_ard", True, lambda d: _ls(d) + [0.2, -1.0], lambda hp: tam.ARDMatern(hp, 1)),
    "matern52": ("matern52", False, lambda d: [0.9, 0.2, -1.0], lambda hp: truth.Matern(hp, 2)),
    "matern52_ard": ("matern52_ard", True, lambda d: _ls(d) + [0.2, -1.0], lambda hp: tam.ARDMatern(hp, 2)),
    "rq": ("rq", False, lambda d: [0.9, 0.4, 0.2, -1.0], lambda hp: trq.RQ(hp, tied=True)),
    "rq_ard": ("rq_ard", True, lambda d: _ls(d) + [0.4, 0.2, -1.0], trq.RQ),
}
# (family, n, d, t, split): the eight names at one shape; the shapes on SE and RQ-ARD -- n below a wave's 16 rows, ragged
# against the 64-row workgroup and the 32-row stage, one j past the 128-term fold, several workgroups; d = 17: the second
# feature chunk; t across the two column-tile forms; one forced split
PRODUCT = ([(f, 129, 3, 17, 0) for f in sorted(FAMILIES)]
           + [(f, n, d, t, s) for f in ("se", "rq_ard")
              for n, d, t, s in ((1, 1, 1, 0), (63, 3, 16, 0), (65, 17, 64, 0), (200, 3, 17, 0), (200, 1, 1, 3))])


def weights(family, hp, d):
    """The d weights 1 / l_c in fp64, as the handle forms them."""
    hp = np.asarray(hp, dtype=np.float64)
    return np.exp(-(hp[:d] if FAMILIES[family][1] else np.repeat(hp[0], d)))


@functools.lru_cache(maxsize=None)
def case(family, n, d, log_sn=-1.0):
    """-> (X, y, theta, K = Kf + sn2 I in longdouble, M = (1 + |log g| + sqrt(s) m) |Kf|): computed once, never changed."""
    truth.require_extended()
    X, y = synth(n, d=d, seed=3 * n + d, scale=4.0 if d <= 3 else 1.8)
    hp = FAMILIES[family][2](d)[:-1] + [log_sn]
    cov = FAMILIES[family][3](hp)
    Kf = cov.k(X.astype(LD), X.astype(LD))
    w = weights(family, hp, d).astype(LD)
    S = truth.wsqdist(X, X, w)
    m = np.abs(X.astype(LD) * w).max(1)
    with np.errstate(divide="ignore"):
        M = (1 + np.abs(np.log(Kf / cov.sf2)) + np.sqrt(S) * np.maximum(m[:, None], m[None, :])) * np.abs(Kf)
    return X, y, hp, Kf + cov.sn2 * np.eye(n, dtype=LD), M


def vectors(t, n):
    """Standard normals; with several columns, a column of magnitude 1e6 beside one of 1e-6 (columns must not leak)."""
    V = np.random.default_rng(100 * t + n).standard_normal((t, n))
    if t > 2:
        V[1] *= 1e6
        V[2] *= 1e-6
    return V


def yardstick(M, V):
    return U32 * (np.abs(V).astype(LD) @ M.T)


def restate32(family, X, hp, V):
    """k_cov_apply32's arithmetic in numpy.float32: coordinates, weights and scalars rounded to fp32, differences before
    squares in feature order, the family's exp2 / log2 / sqrt form, fp32 sums over at most 128 j folded into fp64."""
    f = np.float32
    kernel, ard = FAMILIES[family][:2]
    n, d = X.shape
    hp = np.asarray(hp, dtype=np.float64)
    route = ard or kernel.startswith("rq")
    w, X32, log2e = weights(family, hp, d).astype(f), X.astype(f), f(1.4426950408889634)
    S = np.zeros((n, n), dtype=f)
    for c in range(d):
        D = X32[:, c][:, None] - X32[:, c][None, :]
        D = D * w[c] if route else D
        S += D * D
    if not route:
        S = S * f(1.0 / np.exp(2 * hp[0]))
    sf2 = f(np.exp(2 * hp[-2]))
    if kernel.startswith("se"):
        Kf = sf2 * np.exp2(S * (f(-0.5) * log2e))
    elif kernel.startswith("rq"):
        alpha = np.exp(hp[-3])
        Kf = sf2 * np.exp2(-(f(alpha) * np.log2(f(1) + S * f(0.5 / alpha))))
    else:
        a = f(np.sqrt(3.0) if "32" in kernel else np.sqrt(5.0)) * np.sqrt(S)
        p = f(1) + a
        p = p + (a * a) * f(1.0 / 3.0) if "52" in kernel else p
        Kf = sf2 * (p * np.exp2(-(a * log2e)))
    assert Kf.dtype == f
    out, V32 = np.zeros(V.shape), V.astype(f)
    for j0 in range(0, n, 128):
        out += (V32[:, j0:j0 + 128] @ Kf[:, j0:j0 + 128].T).astype(np.float64)
    return out + np.exp(2 * hp[-1]) * V


def handle(family, n, d, log_sn=-1.0, split=0):
    from cugp_amd import gp
    X, y, hp = case(family, n, d, log_sn)[:3]
    kernel, ard = FAMILIES[family][:2]
    g = gp.IterativeGP(n, d, kernel=kernel, ard=ard and kernel == "se")
    g.set_data(X, y)
    g.set_loghyper(hp)
    g.set_split(split)
    return g
