#!/usr/bin/env python3
"""Levels/s of BatchedPcgrlEnv.solve() (pcgrl_get_solution) next to evaluate() (pcgrl_get_stats) on the same M seeded random 5 x 5
sokoban levels, and of solve() on a handle's own levels (M environments after a reset, the map buffer read in place), on the GPU box.
Method of tools/evaluate_bench.py -- wall clock around the call with a device synchronisation, after a warm-up, every child process under
a time limit so that a hang ends there, a child that fails ends the session -- but a call is 2-4 ms and the box is shared, so evaluate()
and solve() run in ONE process on one handle, alternating, 30 rounds: minimum, median and maximum of each.  Their statistics rows must
agree.  One JSON line at the end.

    python tools/solve_bench.py [M]          (default: 65536)
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
ROUNDS = 30
LIMIT_S = 240


def timed(call, sync):
    t0 = time.perf_counter()
    r = call()
    sync()
    return time.perf_counter() - t0, r


def child(route, m):
    import torch
    from evaluate_bench import levels
    from gym_pcgrl_amd.envs import BatchedPcgrlEnv
    out = {"route": route, "M": m}
    sync = torch.cuda.synchronize
    if route == "own":
        env = BatchedPcgrlEnv(prob="sokoban", rep="wide", num_envs=m, seed=0)
        env.reset()
        calls = {"solve_own": lambda: env.solve()}
    else:       # the two calls on one handle and the same maps, alternating: what the box does meanwhile meets both alike
        maps = torch.as_tensor(levels("sokoban", m)).cuda()
        env = BatchedPcgrlEnv(prob="sokoban", rep="wide", num_envs=1, seed=0)
        calls = {"evaluate": lambda: env.evaluate(maps), "solve": lambda: env.solve(maps)}
    last = {}
    for k, c in calls.items():                  # warm-up: the handle, the workspace, the kernels' code objects
        last[k] = c()
    sync()
    t = {k: [] for k in calls}
    for _ in range(ROUNDS):
        for k, c in calls.items():
            dt, last[k] = timed(c, sync)
            t[k].append(dt)
    out["s"] = t
    out["checksum"] = {k: int(r.rows[:, :env._layout.nstats].to(torch.int64).sum().item()) for k, r in last.items()}
    for k, r in last.items():
        if k != "evaluate":
            out["solved"] = int((r.length > 0).sum().item())
            out["moves"] = int(r.length.to(torch.int64).sum().item())
            out["longest"] = int(r.length.max().item())
    assert env.check_status() == 0
    print("RESULT " + json.dumps(out), flush=True)


def main():
    args = sys.argv[1:]
    m = int(args[0]) if args else 65536
    res = {}
    for route in ("pair", "own"):
        p = subprocess.run(["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.abspath(__file__), "--child", route, str(m)],
                           capture_output=True, text=True)
        if p.returncode != 0:                    # a fault, an abort or the time limit: nothing more is started on the GPU
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            sys.exit("solve_bench: %s ended with status %d" % (route, p.returncode))
        r = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
        res[route] = r
        for k, ts in r["s"].items():
            ts = sorted(ts)
            med = ts[len(ts) // 2]
            print("%-10s M=%d  %d rounds  ms: min %.3f  median %.3f  max %.3f   M levels/s at the median: %.2f%s" % (
                k, m, len(ts), ts[0] * 1e3, med * 1e3, ts[-1] * 1e3, m / med / 1e6,
                ("   solved %d, %d moves, longest %d" % (r["solved"], r["moves"], r["longest"])) if k != "evaluate" else ""), flush=True)
    assert res["pair"]["checksum"]["evaluate"] == res["pair"]["checksum"]["solve"], "solve() and evaluate() disagree on the statistics rows"
    print(json.dumps(res))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], int(sys.argv[3]))
    else:
        main()
