"""The 8-wave geometry of the 128x128 tile product (kernels.h TUNE_WAVES8: k_syrk_wide8, k_lauum8, k_trtri_border8 and
the four-wave launches of the last round's quarters behind them) gives the bits of the 4-wave product: log-likelihood,
gradient and K^-1 with the key on and off, at the default hand-over block and with it forced to 1, 3 and 5.

The defaults send shapes this small down the 64x64 forms and the classic factorisation, so the keys that select the
128x128 launches and the two-speed factorisation (wide far passes) are set per handle, as in test_gpu_launch_paths:
  1664 rows, 13 tiles: ragged launches, first-touch and accumulate shares of K^-1, plain and accumulate bordering stores
  3200 rows, 25 tiles: several hand-over blocks at every forced size
  4224 rows, 33 tiles: the K^-1 shares pass 512 tiles, so a last round runs as quarters in the launch behind (default block)
"""
import numpy as np
import pytest

from conftest import synth

pytestmark = pytest.mark.gpu

LAUUM_WM2, TRTRI_WM2, PIPE_BLOCK, BORDER_WM2, PANEL, NEAR, PANEL_MIN_NT, WAVES8 = 0, 1, 3, 4, 8, 9, 10, 22   # kernels.h TUNE_*
D, SCALE = 3, 8.0
HP = np.array([0.9, 0.2, -1.0])
HP_OTHER = HP + np.array([0.3, -0.2, 0.25])


def evaluate(g):
    g.set_loghyperparam(HP_OTHER)                           # nothing is answered from what the handle holds
    g.loglik_grad()
    g.set_loghyperparam(HP)
    ll, gr = g.loglik_grad()
    return ll, np.asarray(gr), g.get_K_inverse()


@pytest.mark.parametrize("n,blocks", [(1664, (-1, 1, 3, 5)), (3200, (-1, 1, 3, 5)), (4224, (-1,))])
def test_eight_waves_give_the_bits_of_four(n, blocks):
    import cugp_amd.gp as gp
    X, y = synth(n, d=D, seed=n, scale=SCALE)
    g = gp.Covsum(n, D)
    try:
        g.set_data(X, y)
        for key, value in ((LAUUM_WM2, 0), (TRTRI_WM2, 0), (BORDER_WM2, 0), (PANEL, 4), (NEAR, 8), (PANEL_MIN_NT, 0)):
            g.set_tuning(key, value)
        for w in blocks:
            g.set_tuning(PIPE_BLOCK, w)
            g.set_tuning(WAVES8, 0)
            four = evaluate(g)
            g.set_tuning(WAVES8, 1)
            eight = evaluate(g)
            assert np.isfinite(four[0]) and np.all(np.isfinite(four[1])), (w, four[:2])
            assert eight[0] == four[0], (w, eight[0], four[0])
            assert np.array_equal(eight[1], four[1]), (w, eight[1], four[1])
            assert np.array_equal(eight[2], four[2]), (w, "K^-1")
    finally:
        g.close()
