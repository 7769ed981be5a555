"""The vector kernels of the matrix-free GP (cugp_amd/csrc/iter_device.h: the t conjugate-gradient recurrences and
k_iter_cross_rhs) on the CPU, without a GPU: the kernels' own text in a lock-step host emulation (tools/iter_host_check.cpp)
built as a stand-alone program with -fsanitize=address,undefined.  The program compares every output BIT FOR BIT with plain
loops in the same order of summation (exit code 4 on a mismatch); this script checks the arithmetic of one sweep against
numpy and the right-hand sides against tests/truth_rq.py's fp64 entry.  Columns: random, one zero (done at once), one NaN
(broken), one whose q makes p'q negative (broken), and with q = b the recurrence residual vanishes after one step (a
candidate whose true residual passes); columns 8 and up stay active and meet the closing pass.  The mixed mode's
one-workgroup kernels (k_iter_goal_init, k_iter_step_b_mx, k_iter_step_v_mx) run two cycles and a closing pass on a table of
the program's own, a scenario per column: the tolerance reached, the goal reached (and exactly met), r'r grown 2^20-fold, a
stall flagged, a last leg close above the tolerance flagged and not flagged, NaN in r'r, in a true residual and in b, final = 1.
k_cov_xgrad and k_cov_xgrad_finish (iter_xgrad_device.h) run once, on data of the program's own: ragged nt and n, d = 17, two
ranges, the mean-and-variance and the mean-only forms, bit for bit against plain loops in the kernel's order of summation.
The Lanczos quadrature's k_iter_record and k_slq_quad run eight sweeps of a scenario per column -- logs
that stay open, close as candidates and never reopen after a restart, break down, or never open -- and every log's quadrature,
bit for bit against plain loops, with the quadrature's first two moments checked beside the bits.

    python tools/iter_host_check.py          # builds into a temporary directory; about a minute
"""
import os
import struct
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import host_check  # noqa: E402  (also puts the repository root and tests/ on the path)

XGRAD, SLQ = ("--xgrad",), ("--slq",)   # the program's modes of their own for k_cov_xgrad and the Lanczos quadrature: no input file
CASES = ((1, 16, 3, 1), (65, 16, 3, 5), (513, 16, 17, 16), (1100, 64, 3, 33), XGRAD, SLQ)      # (n, tp, d, test points)
MODES = {XGRAD[0]: "k_cov_xgrad, four instantiations", SLQ[0]: "k_iter_record and k_slq_quad, a scenario per column, tp 16 and 64"}


def run_xgrad(exe, mode=XGRAD[0]):
    import subprocess
    r = subprocess.run([exe, mode], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    ok = r.returncode == 0 and not r.stderr.strip()
    print("%s: bits equal the plain loops  %s" % (MODES[mode], "ok" if ok else "BAD"), r.stdout[-2000:], r.stderr[-3000:])
    return ok


def run(exe, tmp, n, tp=0, d=0, count=0):
    if n in MODES:
        return run_xgrad(exe, n)
    import truth_ard_matern as tam
    import truth_rq as trq
    rng = np.random.default_rng(n + tp)
    X, Xt = rng.uniform(-2, 2, (n, d)), rng.uniform(-2, 2, (count, d))
    Xt[0] = X[n // 2]
    hp = list(np.linspace(0.4, 1.1, d)) + [0.4, 0.3, -0.8]
    alpha, h2a = trq.host_shape(hp[-3])
    w = np.exp(-np.asarray(hp[:d]))
    sf2 = float(np.exp(2 * hp[-2]))
    b = rng.standard_normal((n, tp))
    q = 2.0 * b + 0.1 * rng.standard_normal((n, tp))
    q[:, 8:] += 3.0 * rng.standard_normal((n, tp - 8))     # far from a multiple of b: these columns stay active
    q[:, 0] = b[:, 0]                                 # x = b solves it: candidate, then done
    if tp > 4:
        b[:, 1] = 0.0
        b[0, 2] = np.nan
        q[:, 3] = -b[:, 3]
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("4i", n, tp, d, count))
        for arr in ([2.25, sf2, 0.2], w, [alpha, h2a], X, Xt, b, q):
            f.write(np.ascontiguousarray(arr, dtype=np.float64).tobytes())
    if not host_check.execute(exe, fin, fout, n, tp, d, count):
        return False
    out = np.fromfile(fout)
    cnt = n * tp
    x, sc = out[:cnt].reshape(n, tp), out[3 * cnt: 3 * cnt + 8 * 64].reshape(8, 64)
    Rs, Rq = (out[3 * cnt + 512 + k * cnt: 3 * cnt + 512 + (k + 1) * cnt].reshape(n, tp) for k in (0, 1))
    state = sc[4, :tp]
    ok = state[0] == 2 and np.allclose(x[:, 0], b[:, 0], rtol=1e-14)
    if tp > 4:
        ok = ok and list(state[1:4]) == [2, 3, 3] and np.all(x[:, 1] == 0) and np.all(np.isnan(x[:, 2:4]))
        pq = (b * q).sum(0)
        live = np.array([c for c in range(4, tp) if pq[c] > 0], dtype=int)      # (p'q <= 0, possible at n = 1: broken)
        ok = ok and all(state[c] == 3 for c in range(4, tp) if not pq[c] > 0)
        a = (b[:, live] ** 2).sum(0) / pq[live]
        ok = ok and np.allclose(x[:, live], a * b[:, live], rtol=1e-12) and np.allclose(sc[2, live], a, rtol=1e-12)
    want = trq.entry_fp64(tam.wsqdist64(X, Xt, w), sf2, alpha, h2a)[0]
    se = sf2 * np.exp(-0.5 * ((X[:, None, :] - Xt[None, :, :]) ** 2).sum(2) / 2.25)
    ok = ok and np.allclose(Rq[:, :count], want, rtol=1e-13) and np.allclose(Rs[:, :count], se, rtol=1e-13)
    ok = ok and np.all(Rq[:, count:] == 0) and np.all(Rs[:, count:] == 0) and Rq[n // 2, 0] == sf2
    # the mixed mode's cycle kernels (check_mixed's table): the state and the stall flag each scenario must end in
    scm = out[-13 * 64:].reshape(13, 64)
    ok = ok and list(scm[4, :11]) == [2, 2, 0, 3, 3, 2, 3, 2, 4, 4, 3] and np.all(scm[4, 11:tp] == 0)
    ok = ok and list(scm[12, :11]) == [0, 1, 1, 0, 0, 0, 0, 0, 0, 1, 0] and np.all(scm[12, 11:tp] == 0)
    ok = ok and scm[6, 2] == 0.5 * scm[1, 2] and scm[11, 8] == 1.5 * scm[7, 8] and np.all(scm[:, tp:] == -7) and np.all(scm[8:10] == -7)
    print("n %-4d tp %-2d d %-2d test points %-2d  bits equal the plain loops; one sweep, the right-hand sides and the mixed cycles against numpy  %s"
          % (n, tp, d, count, "ok" if ok else "BAD"))
    return bool(ok)


if __name__ == "__main__":
    sys.exit(host_check.main("iter_host_check", CASES, run))
