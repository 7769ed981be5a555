"""tests/rank_children.run_ranks without a GPU: what the two-rank GPU tests rely on when a rank fails.  The ranks here are
plain Python one-liners; the surviving rank would run for two minutes if it were left alone, and is gone within moments."""
import os
import sys
import time

import rank_children


def gone(pid):
    """No such process, or only its unreaped remains."""
    try:
        os.kill(pid, 0)
    except ProcessLookupError:
        return True
    try:
        with open("/proc/%d/stat" % pid) as f:
            return f.read().rsplit(")", 1)[1].split()[0] == "Z"
    except OSError:
        return True


def wait_gone(pid, seconds=10.0):
    end = time.monotonic() + seconds
    while time.monotonic() < end:
        if gone(pid):
            return True
        time.sleep(0.02)
    return gone(pid)


def test_all_ranks_succeed(tmp_path):
    cmds = [[sys.executable, "-c", "print('rank %d fine')" % r] for r in range(2)]
    failed, texts = rank_children.run_ranks(cmds, dict(os.environ), tmp_path, 60)
    assert failed is None and [t.strip() for t in texts] == ["rank 0 fine", "rank 1 fine"]


def test_the_first_failure_ends_the_other_rank_and_its_children(tmp_path):
    pidfile = tmp_path / "pids"
    # rank 1 starts a child of its own (as a rank's helpers would), records both pids and then waits "in a collective"
    waiter = ("import os, subprocess, sys, time\n"
              "c = subprocess.Popen([sys.executable, '-c', 'import time; time.sleep(120)'])\n"
              "open(%r + '.tmp', 'w').write('%%d %%d' %% (os.getpid(), c.pid)); os.rename(%r + '.tmp', %r)\n"
              "print('rank 1 waiting', flush=True); time.sleep(120)\n" % (str(pidfile), str(pidfile), str(pidfile)))
    # rank 0 fails once rank 1 is surely up
    failer = ("import os, sys, time\n"
              "while not os.path.exists(%r): time.sleep(0.01)\n"
              "print('rank 0 failing', flush=True); sys.exit(3)\n" % str(pidfile))
    t0 = time.monotonic()
    failed, texts = rank_children.run_ranks([[sys.executable, "-c", failer], [sys.executable, "-c", waiter]], dict(os.environ),
                                            tmp_path, 100)
    took = time.monotonic() - t0
    assert failed == (0, 3) and "rank 0 failing" in texts[0] and "rank 1 waiting" in texts[1]
    assert took < 30.0, took                                          # (not rank 1's two minutes, not the time limit)
    rank, child = (int(v) for v in pidfile.read_text().split())
    assert wait_gone(rank) and wait_gone(child), (rank, child)

