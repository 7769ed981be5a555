"""The launch plan's alternatives on the GPU: every branch that a launch-shape key (kernels.h TUNE_*) selects, held to a
plain fp64 reference or to the bits of the branch it replaces.

The defaults send each shape down one branch only, so these tests set the keys per handle (cugp_set_handle_tuning; a
group runs on its lead expert's keys) and never touch the process defaults:
  - the two-speed Cholesky (near window + k_syrk_wide far passes) at small tile counts, every panel width, near window
    and sub-panel size, including the smallest default two-speed shape (48 tiles);
  - the fused finalize in k_trace against the separate k_finalize, the 64x64 against the 128x128 product forms, the
    K^-1 share on its own stream, grouped against single experts, a refused group: the same bits;
  - captured graphs after a handle or a group switches configuration.

References: the CPU oracle (the reference's serial arithmetic) up to ~1600 rows; above, numpy fp64 (Cholesky,
explicit inverse, the gradient as 1/2 tr((K^-1 - alpha alpha^T) dK/dtheta)), checked against the oracle here first.
The data are chosen so that K is far from diagonal (d = 3 in a box of 16: cond(K) 5e2 .. 3e3), so a tile that misses
an update or receives one twice moves L, K^-1 and the log-likelihood far beyond the bounds.
"""
import numpy as np
import pytest

from conftest import synth
from test_gpu_parity import ll_close, rows_close, vec_close

pytestmark = pytest.mark.gpu

(LAUUM_WM2, TRTRI_WM2, SYRK_REM, PIPE_BLOCK, BORDER_WM2, GRAPHS, GROUP_OVERLAP, GROUP_MAX_TILES, PANEL, NEAR,
 PANEL_MIN_NT, LAUUM_STREAM, FINALIZE_FUSE_MAX, SPLIT_REM, STEP_QUARTER, _STREAM_PRIO, _BARRIER_SPIN, SUBPANEL,
 ZFUSE) = range(19)
KIND_WIDE, KIND_BORDER4, KIND_BORDER2, KIND_LAUUM4, KIND_LAUUM2, KIND_LEVEL4, KIND_LEVEL2 = 1, 2, 3, 4, 5, 6, 7
WIDTH_KEYS = (LAUUM_WM2, TRTRI_WM2, SYRK_REM, BORDER_WM2, SPLIT_REM, STEP_QUARTER)

D, SCALE = 3, 8.0
HP = np.array([0.9, 0.2, -1.0])
HP_OTHER = HP + np.array([0.3, -0.2, 0.25])      # evaluated before every checked evaluation: nothing is cached
ORACLE_MAX_ROWS = 1600


@pytest.fixture(scope="module")
def gp_mod():
    import cugp_amd.gp as gp
    return gp


def data(n, seed=None):
    return synth(n, d=D, seed=n if seed is None else seed, scale=SCALE)


# ------------------------------------------------------------------ references (each computed once per module)
_REF = {}


def numpy_ref(oracle, X, y, hp):
    """LL, gradient of -LL, y' K^-1 y, log|K|, L, K^-1 in plain numpy fp64 on the oracle's K.  The conventions are the
    reference's (oracle.loglik_grad): log(2 pi) truncated to 1.83787, theta = log hyper-parameters with the
    hyper-scalars exp(2 theta), the gradient of the NEGATIVE log-likelihood."""
    n = len(y)
    K = oracle.K_train(X, hp)
    L = np.linalg.cholesky(K)
    Ki = np.linalg.inv(K)
    alpha = Ki @ y
    quad = float(y @ alpha)
    logdet = 2.0 * float(np.sum(np.log(np.diag(L))))
    ll = -0.5 * (quad + logdet + n * 1.83787)
    sn2 = np.exp(2.0 * hp[2])
    W = Ki - np.outer(alpha, alpha)
    WK = W * K
    trW = float(np.trace(W))
    S = oracle.sqdist(X, np.exp(2.0 * hp[0]))               # |xi - xj|^2 / l^2 = d(log k_ij)/d(theta0)
    g = np.array([0.5 * float(np.sum(WK * S)),             # dK/dtheta0 = K o S
                  float(np.sum(WK)) - sn2 * trW,           # dK/dtheta1 = 2 (K - sn2 I)
                  sn2 * trW])                              # dK/dtheta2 = 2 sn2 I
    return dict(ll=ll, g=g, quad=quad, logdet=logdet, L=L, Ki=Ki)


def reference(oracle, n, seed=None):
    """The oracle's LL, gradient, quadratic form and log-determinant up to ORACLE_MAX_ROWS rows (L and K^-1 from numpy
    at every size), numpy's above."""
    key = (n, D, tuple(HP), seed)
    if key not in _REF:
        X, y = data(n, seed)
        r = numpy_ref(oracle, X, y, HP)
        if n <= ORACLE_MAX_ROWS:
            r["ll"], r["g"] = oracle.loglik_grad(X, y, HP)
            r["quad"], r["logdet"] = oracle.chol_and_det(oracle.K_train(X, HP), y)
        _REF[key] = r
    return _REF[key]


# ------------------------------------------------------------------ evaluations
def record(g):
    """Everything one configuration produces at HP, each evaluation behind one at HP_OTHER: gradient evaluation
    (LL, gradient, quadratic form, log-determinant, L, K^-1), then LL-only with z inside the factorisation (key 18 = 1)
    and behind it (key 18 = 0)."""
    g.set_loghyperparam(HP_OTHER)
    g.loglik_grad()
    g.set_loghyperparam(HP)
    ll, gr = g.loglik_grad()
    q, ld = g.last_quad_logdet()
    r = dict(ll=ll, g=np.asarray(gr), quad=q, logdet=ld, L=g.get_cholesky(), Ki=g.get_K_inverse())
    zfuse = g.get_tuning(ZFUSE)
    try:
        for z in (1, 0):
            g.set_tuning(ZFUSE, z)
            g.set_loghyperparam(HP_OTHER)
            g.compute_loglikelihood()
            g.set_loghyperparam(HP)
            r["ll_z%d" % z] = g.compute_loglikelihood()
            r["quad_z%d" % z], r["logdet_z%d" % z] = g.last_quad_logdet()
    finally:
        g.set_tuning(ZFUSE, zfuse)
    return r


def check_ref(r, ref, what):
    assert ll_close(r["ll"], ref["ll"]), (what, r["ll"], ref["ll"])
    assert vec_close(r["g"], ref["g"]), (what, r["g"], ref["g"])
    assert abs(r["quad"] - ref["quad"]) <= 1e-11 * abs(ref["quad"]), (what, r["quad"], ref["quad"])
    assert abs(r["logdet"] - ref["logdet"]) <= 1e-11 * max(1.0, abs(ref["logdet"])), (what, r["logdet"], ref["logdet"])
    assert rows_close(r["L"], ref["L"], 1e-12), (what, "L", np.max(np.abs(r["L"] - ref["L"])))
    assert rows_close(r["Ki"], ref["Ki"], 1e-11), (what, "K^-1", np.max(np.abs(r["Ki"] - ref["Ki"])))
    for z in (1, 0):
        assert ll_close(r["ll_z%d" % z], ref["ll"]), (what, "key 18 = %d" % z, r["ll_z%d" % z], ref["ll"])
        assert abs(r["quad_z%d" % z] - ref["quad"]) <= 1e-11 * abs(ref["quad"]), (what, "key 18 = %d" % z)
        assert r["logdet_z%d" % z] == r["logdet"], (what, "key 18 = %d: not the same factor" % z)


def same_bits(a, b, what, keys=None):
    for k in keys or a.keys():
        assert np.array_equal(a[k], b[k]), (what, k, np.max(np.abs(np.asarray(a[k]) - np.asarray(b[k]))))


def set_keys(g, cfg):
    for k, v in cfg.items():
        g.set_tuning(k, v)


def launches(g, kinds):
    """Launches of each timed kernel kind in one gradient evaluation (profiling level 3: every launch is timed; the
    evaluation is launch by launch)."""
    g.set_profiling(3)
    try:
        for k in kinds:
            g.kernel_stats(reset=True, kind=k)
        g.set_loghyperparam(HP_OTHER)
        g.loglik_grad()
        return {k: g.kernel_stats(kind=k)["launches"] for k in kinds}
    finally:
        g.set_profiling(0)


def single(gp_mod, n, cfg=None, seed=None, npad_min=0):
    X, y = data(n, seed)
    g = gp_mod.Covsum(n, D, npad_min=npad_min)
    g.set_data(X, y)
    set_keys(g, cfg or {})
    return g


def group(gp_mod, K, n, cfg=None):
    """K experts of n rows each (BCM.split); cfg goes on the lead expert, whose keys the group runs on."""
    X, y = data(K * n)
    b = gp_mod.BCM.split(X, y, K)
    set_keys(b.expert(0), cfg or {})
    return b


def record_group(b, inverse=True):
    b.set_BCM_log_hyperparam(HP_OTHER)
    b.loglik_grad_rows()
    b.set_BCM_log_hyperparam(HP)
    r = {"rows": b.loglik_grad_rows()}
    for k in range(len(b.rows)):
        e = b.expert(k)
        r["L%d" % k] = e.get_cholesky()
        if inverse:
            r["Ki%d" % k] = e.get_K_inverse()
    return r


def experts_alone(gp_mod, b, cfg):
    """Every expert of the group b evaluated alone, at the group's common padded size
    (as test_gpu_parity.test_grouped_experts_equal_single_experts builds them)."""
    X, y = data(sum(b.rows))
    out, lo = [], 0
    for k, m in enumerate(b.rows):
        g = gp_mod.Covsum(m, D, npad_min=max(b.rows))
        g.set_data(X[lo:lo + m], y[lo:lo + m])
        set_keys(g, cfg)
        g.set_loghyperparam(HP_OTHER)
        g.loglik_grad()
        g.set_loghyperparam(HP)
        ll, gr = g.loglik_grad()
        out.append(dict(row=np.concatenate([[ll], gr]), L=g.get_cholesky(), Ki=g.get_K_inverse()))
        g.close()
        lo += m
    return out


# ------------------------------------------------------------------ the numpy reference itself
@pytest.mark.parametrize("n", [300, 769])
def test_numpy_reference_matches_the_oracle(oracle, n):
    X, y = data(n)
    r = numpy_ref(oracle, X, y, HP)
    llo, go = oracle.loglik_grad(X, y, HP)
    qo, ldo = oracle.chol_and_det(oracle.K_train(X, HP), y)
    assert abs(r["ll"] - llo) <= 1e-10 * abs(llo), (r["ll"], llo)
    assert vec_close(r["g"], go, rel=1e-8, floor=1e-12), (r["g"], go)
    assert abs(r["quad"] - qo) <= 1e-10 * abs(qo) and abs(r["logdet"] - ldo) <= 1e-10 * abs(ldo)
    assert rows_close(r["L"], oracle.cholesky(oracle.K_train(X, HP)), 1e-12)


# ------------------------------------------------------------------ T1: the two-speed schedule at small tile counts
@pytest.mark.parametrize("n,P,subpanels", [
    (769, 2, (1, 2)),          # nt = 7
    (1100, 3, (1,)),           # nt = 9
    (1537, 4, (1, 2, 4)),      # nt = 13
    (3001, 8, (1, 2, 4)),      # nt = 24
    (2400, 6, (3,)),           # nt = 19: sub-panels of 3 (plan_step and diag_update_tile_nk<3>)
    (1100, 1, (2, 4)),         # classic form with sub-panels: the plan keeps S where P = 1
])
def test_two_speed_schedule_vs_reference(gp_mod, oracle, n, P, subpanels):
    """Key 10 = 1 allows a panel from nt >= 3P on, so the near window + far pass form runs at 7 .. 24 tiles, with the
    near window from one tile to the whole trailing matrix and every sub-panel size that divides the panel.  Against
    the reference; each configuration twice (another point between): the same bits."""
    ref = reference(oracle, n)
    g = single(gp_mod, n, {PANEL_MIN_NT: 1, PANEL: P})
    nears = (1, 12, 60, 10 ** 6) if P > 1 else (500,)
    for near in nears:
        for S in subpanels:
            cfg = "n=%d key8(P)=%d key9(near)=%d key17(S)=%d key10=1" % (n, P, near, S)
            set_keys(g, {NEAR: near, SUBPANEL: S})
            r = record(g)
            check_ref(r, ref, cfg)
            same_bits(record(g), r, cfg + ": repeated")
    if P > 1:                  # (near = 10^6 puts every column in the window: no far pass, the classic form)
        set_keys(g, {NEAR: 12})
        assert launches(g, [KIND_WIDE])[KIND_WIDE] > 0, "n=%d P=%d: no far pass ran (not the two-speed form)" % (n, P)
    g.close()


# ------------------------------------------------------------------ T2 / T3: default keys at the switch sizes
@pytest.mark.parametrize("S", [1, 2, 4])
def test_smallest_default_two_speed_shape(gp_mod, oracle, S):
    """6100 rows = 48 tiles = 3 x 16: the first size the default keys (P = 16, from 32 tiles) factor in two speeds."""
    g = single(gp_mod, 6100, {SUBPANEL: S} if S > 1 else {})
    check_ref(record(g), reference(oracle, 6100), "n=6100 default keys, key17(S)=%d" % S)
    assert launches(g, [KIND_WIDE])[KIND_WIDE] > 0
    g.close()


def test_classic_schedule_at_33_tiles(gp_mod, oracle):
    """4200 rows = 33 tiles: the classic right-looking form (33 < 3 x 16), whose first step launches hold >= 512
    tiles, so the split last round (keys 2, 13) runs."""
    g = single(gp_mod, 4200)
    check_ref(record(g), reference(oracle, 4200), "n=4200 default keys")
    assert launches(g, [KIND_WIDE])[KIND_WIDE] == 0
    g.close()


# ------------------------------------------------------------------ B1: fused vs separate finalize
@pytest.mark.parametrize("n", [1500, 4200])
def test_fused_finalize_equals_separate_launch(gp_mod, n):
    """Key 12: the last block of k_trace takes the final sums (1 << 30: always) or k_finalize does (0): the same sums
    in the same order (eval_gfx950.h finalize_sums), so the same bits -- replayed from a captured graph (key 5 = 1; the
    inverse after the factorisation, key 3 = 0, so the evaluation is one stream) and launch by launch."""
    g = single(gp_mod, n, {PIPE_BLOCK: 0})
    for graphs in (1, 0):
        res = {}
        for fuse in (0, 1 << 30):
            set_keys(g, {GRAPHS: graphs, FINALIZE_FUSE_MAX: fuse})
            res[fuse] = record(g)
        same_bits(res[0], res[1 << 30], "n=%d key5(graphs)=%d key12 0 vs 1<<30" % (n, graphs))
    g.close()


def test_fused_finalize_equals_separate_launch_in_a_group(gp_mod):
    b = group(gp_mod, 3, 1500)
    res = {}
    for graphs in (1, 0):
        for fuse in (0, 1 << 30):
            set_keys(b.expert(0), {GRAPHS: graphs, FINALIZE_FUSE_MAX: fuse})
            res[(graphs, fuse)] = record_group(b)
    for k in res:
        same_bits(res[k], res[(1, 0)], "3 x 1500 key5(graphs), key12 = %s against (1, 0)" % (k,))
    b.close()


# ------------------------------------------------------------------ B2: 64x64 vs 128x128 tile forms
WIDTHS = {"128-wide": {k: 0 for k in WIDTH_KEYS}, "64-wide": {k: 1 << 30 for k in WIDTH_KEYS}, "default": {}}


@pytest.mark.parametrize("n", [1100, 2049, 4200])
def test_tile_widths_give_the_same_bits(gp_mod, n):
    """Keys 0, 1, 2, 4, 13, 14 choose between the 64x64 and the 128x128 form of k_lauum, k_trtri_level,
    k_trtri_border, the step kernel's tiles and the split last round.  Both forms give every output element its k
    terms in the same order (tile_nt: one MFMA chain per 16x16 sub-tile, k ascending), so the bits agree."""
    res = {}
    for name, cfg in WIDTHS.items():
        g = single(gp_mod, n, cfg)
        res[name] = record(g)
        if name != "default":
            c = launches(g, [KIND_LAUUM4, KIND_LAUUM2, KIND_LEVEL4, KIND_LEVEL2, KIND_BORDER4, KIND_BORDER2])
            wide, narrow = c[KIND_LAUUM4] + c[KIND_LEVEL4] + c[KIND_BORDER4], c[KIND_LAUUM2] + c[KIND_LEVEL2] + c[KIND_BORDER2]
            assert (narrow == 0 and wide > 0) if name == "128-wide" else (wide == 0 and narrow > 0), (n, name, c)
        g.close()
    same_bits(res["128-wide"], res["64-wide"], "n=%d keys 0,1,2,4,13,14 = 0 vs 1<<30" % n)
    same_bits(res["default"], res["64-wide"], "n=%d keys 0,1,2,4,13,14 default vs 1<<30" % n)


def test_tile_widths_give_the_same_bits_in_a_group(gp_mod):
    res = {}
    for name, cfg in WIDTHS.items():
        b = group(gp_mod, 4, 1100, cfg)
        res[name] = record_group(b)
        b.close()
    same_bits(res["128-wide"], res["64-wide"], "4 x 1100 keys 0,1,2,4,13,14 = 0 vs 1<<30")
    same_bits(res["default"], res["64-wide"], "4 x 1100 keys 0,1,2,4,13,14 default vs 1<<30")


# ------------------------------------------------------------------ B3: the K^-1 share's stream
@pytest.mark.parametrize("n", [2049, 4200])
def test_inverse_share_stream_gives_the_same_bits(gp_mod, n):
    """Key 11: the K^-1 share of an inverse block on a stream of its own (2) or behind its block's bordering (0, and 1
    for a single matrix): the shares are added in block order whichever stream carries them."""
    res = {}
    for v in (0, 1, 2):
        g = single(gp_mod, n, {LAUUM_STREAM: v})
        res[v] = record(g)
        g.close()
    same_bits(res[0], res[1], "n=%d key11 0 vs 1" % n)
    same_bits(res[0], res[2], "n=%d key11 0 vs 2" % n)


def test_inverse_share_stream_gives_the_same_bits_in_a_group(gp_mod):
    res = {}
    for v in (0, 1, 2):
        b = group(gp_mod, 3, 1500, {LAUUM_STREAM: v})
        res[v] = record_group(b)
        b.close()
    same_bits(res[0], res[1], "3 x 1500 key11 0 vs 1")
    same_bits(res[0], res[2], "3 x 1500 key11 0 vs 2")


# ------------------------------------------------------------------ B4: sub-panels that do not divide the panel
def test_subpanel_not_dividing_the_panel_falls_back(gp_mod):
    """P = 3 at 9 tiles (two-speed with key 10 = 1): S = 2 does not divide P, the plan takes S = 1."""
    base = {PANEL_MIN_NT: 1, PANEL: 3}
    g = single(gp_mod, 1100, {**base, SUBPANEL: 1})
    r1 = record(g)
    set_keys(g, {SUBPANEL: 2})
    same_bits(record(g), r1, "n=1100 key8(P)=3 key10=1: key17 2 vs 1")
    g.close()


# ------------------------------------------------------------------ B5: grouped vs alone beyond the default schedule
SCHED = {PANEL_MIN_NT: 1, PANEL: 4, NEAR: 12, SUBPANEL: 2}


@pytest.mark.parametrize("K,n,cfg", [(3, 1537, SCHED), (2, 6100, {})])
def test_grouped_equals_alone_under_two_speed(gp_mod, K, n, cfg):
    """A group runs the two-speed factorisation with blockIdx.y = expert: every expert's LL, gradient, L and K^-1 are
    the bits of the same expert alone at the group's padded size.  3 x 1537 under P = 4, near 12, S = 2 (13 tiles);
    2 x 6100 at the default keys (48 tiles); the non-default group twice: the same bits."""
    b = group(gp_mod, K, n, cfg)
    r = record_group(b)
    if cfg:
        same_bits(record_group(b), r, "%d x %d %s: repeated" % (K, n, cfg))
    alone = experts_alone(gp_mod, b, cfg)
    for k, a in enumerate(alone):
        what = "%d x %d %s expert %d" % (K, n, cfg, k)
        assert np.array_equal(r["rows"][k], a["row"]), (what, r["rows"][k], a["row"])
        assert np.array_equal(r["L%d" % k], a["L"]), what
        assert np.array_equal(r["Ki%d" % k], a["Ki"]), what
    b.close()


# ------------------------------------------------------------------ B6: a refused group
@pytest.mark.parametrize("K,n", [(3, 1100), (16, 1500)])
def test_refused_group_equals_the_group(gp_mod, K, n):
    """Key 7 = 1 on the lead: the group is refused and the experts run one by one.  An expert of a BCM has its own
    overlap off, so alone it builds K^-1 after its factorisation: the bits of the group with key 6 = 0, and the default
    group's (K^-1 beside the factorisation: the same terms summed in another order) to the reference tolerance."""
    b = group(gp_mod, K, n)
    r = record_group(b, inverse=False)
    set_keys(b.expert(0), {GROUP_OVERLAP: 0})
    r_after = record_group(b, inverse=False)
    set_keys(b.expert(0), {GROUP_MAX_TILES: 1})
    alone = record_group(b, inverse=False)
    same_bits(alone, r_after, "%d x %d key7 = 1 vs the group with key6 = 0" % (K, n))
    for k in range(K):
        assert ll_close(alone["rows"][k, 0], r["rows"][k, 0]), (K, n, k)
        assert vec_close(alone["rows"][k, 1:], r["rows"][k, 1:]), (K, n, k)
        assert np.array_equal(alone["L%d" % k], r["L%d" % k]), (K, n, k)
    b.close()


# ------------------------------------------------------------------ B7: switching configurations
def test_switching_back_and_forth_follows_the_configuration(gp_mod):
    """A handle (captured graphs: at most 24 tiles, the inverse after the factorisation) switched from the classic form
    A to the two-speed form B and back gives A's bits again, and at B a fresh handle's bits: a graph captured under one
    configuration is not replayed under another (cfg_epoch)."""
    n, A = 1537, {PIPE_BLOCK: 0}
    B = {**SCHED, PIPE_BLOCK: 0}
    g = single(gp_mod, n, A)
    ra = record(g)
    set_keys(g, B)
    rb = record(g)
    assert not np.array_equal(ra["L"], rb["L"]), "A and B give the same factor: the test could not see a stale graph"
    for k in B:
        g.set_tuning(k, A.get(k, g.get_tuning(k)), own=k in A)
    same_bits(record(g), ra, "n=%d back from B to A" % n)
    g.close()
    fresh = single(gp_mod, n, B)
    same_bits(record(fresh), rb, "n=%d B on a fresh handle" % n)
    fresh.close()


def test_switching_back_and_forth_in_a_group(gp_mod):
    """The same for a group (replayed from its lead's captured graph): A = the inverse beside the factorisation (key 6 =
    1), B = after it (key 6 = 0, which only changes the order K^-1 is summed in: the reference tolerance between them)."""
    b = group(gp_mod, 3, 1100)
    ra = record_group(b)
    set_keys(b.expert(0), {GROUP_OVERLAP: 0})
    rb = record_group(b)
    for k in range(3):
        assert ll_close(rb["rows"][k, 0], ra["rows"][k, 0]) and vec_close(rb["rows"][k, 1:], ra["rows"][k, 1:]), k
        assert np.array_equal(rb["L%d" % k], ra["L%d" % k]), k
        assert rows_close(rb["Ki%d" % k], ra["Ki%d" % k], 1e-11), k
    set_keys(b.expert(0), {GROUP_OVERLAP: 1})
    same_bits(record_group(b), ra, "3 x 1100 key6 back to 1")
    b.close()
    fresh = group(gp_mod, 3, 1100, {GROUP_OVERLAP: 0})
    same_bits(record_group(fresh), rb, "3 x 1100 key6 = 0 on a fresh group")
    fresh.close()
