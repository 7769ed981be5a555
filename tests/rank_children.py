"""Child processes that stand for the ranks of a multi-GPU test -- TEST INFRASTRUCTURE, no GPU import; a plain module beside
tests/accuracy.py.  run_ranks starts one command per rank, each under its own `timeout` and in a session of its own, ends
ALL of them on the first failure and starts nothing after it: a rank whose peer is gone would otherwise wait in a collective
with the GPU open.  `timeout` cannot hand SIGKILL on, and killing it alone would orphan the rank without its time limit, so
the whole session -- `timeout` and everything below it -- is killed by process group.  Output goes to files, not pipes: a
survivor cannot hold the parent in a read, and a chatty rank cannot block on a full pipe.  tests/test_rank_children_cpu.py
exercises the failure path without a GPU."""
import os
import signal
import subprocess


def run_ranks(cmds, env, logdir, limit):
    """cmds: one argv per rank; limit: seconds each rank may take (`timeout -k 10 limit`).  -> (failed, texts): failed is
    None, or (rank, exit status) of the first rank that ended with a nonzero status; texts[r] is rank r's stdout and stderr.
    When it returns no process of any rank's session is left."""
    procs, logs = [], []
    try:
        for r, cmd in enumerate(cmds):
            logs.append(open(os.path.join(str(logdir), "rank%d.log" % r), "w"))
            procs.append(subprocess.Popen(["timeout", "-k", "10", str(int(limit))] + [str(a) for a in cmd], stdout=logs[-1],
                                          stderr=subprocess.STDOUT, env=env, start_new_session=True))
        live, failed = set(range(len(procs))), None
        while live and failed is None:                                # the first failure ends all
            for r in sorted(live):
                try:
                    rc = procs[r].wait(timeout=0.2)
                except subprocess.TimeoutExpired:
                    continue
                live.discard(r)
                if rc != 0:
                    failed = (r, rc)
                    break
    finally:
        for p in procs:                                               # the session: `timeout` and the rank below it
            try:
                os.killpg(p.pid, signal.SIGKILL)
            except (ProcessLookupError, PermissionError):
                pass                                                  # (ended by itself, nothing of it left)
        for p in procs:
            p.wait()
        for f in logs:
            f.close()
    texts = []
    for r in range(len(procs)):
        with open(os.path.join(str(logdir), "rank%d.log" % r)) as f:
            texts.append(f.read())
    return failed, texts
