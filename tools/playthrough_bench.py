#!/usr/bin/env python3
"""Levels/s of BatchedPcgrlEnv.playthrough() (pcgrl_get_playthrough) next to evaluate() (pcgrl_get_stats) on the same M seeded random
7 x 11 levels of mdungeon or ddave (the problem's own tile probabilities), and of playthrough() on a handle's own levels (M environments
after a reset, the map buffer read in place), on the GPU box.  Method of tools/solve_bench.py: wall clock around the call with a device
synchronisation, after a warm-up, every child process under a time limit so that a hang ends there, a child that fails ends the session;
evaluate() and playthrough() run in ONE process on one handle, alternating, 30 rounds: minimum, median and maximum of each.  Their
statistics rows must agree.  One JSON line at the end.

    python tools/playthrough_bench.py [--prob mdungeon|ddave] [M]          (default: mdungeon, 65536)
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
ROUNDS = 30
LIMIT_S = 240
H, W = 7, 11


def levels(prob, m):
    """M seeded random levels with the problem's own tile probabilities (what reset() draws)."""
    import numpy as np
    from gym_pcgrl_amd.envs.problems import PROBLEMS
    p = np.array(list(PROBLEMS[prob]()._prob.values()), dtype=np.float64)
    return np.random.RandomState(7).choice(len(p), size=(m, H, W), p=p / p.sum()).astype(np.uint8)


def timed(call, sync):
    t0 = time.perf_counter()
    r = call()
    sync()
    return time.perf_counter() - t0, r


def child(route, prob, m):
    import torch
    from gym_pcgrl_amd.envs import BatchedPcgrlEnv
    out = {"route": route, "prob": prob, "M": m}
    sync = torch.cuda.synchronize
    if route == "own":
        env = BatchedPcgrlEnv(prob=prob, rep="wide", num_envs=m, seed=0)
        env.adjust_param(width=W, height=H)
        env.reset()
        calls = {"playthrough_own": lambda: env.playthrough()}
    else:       # the two calls on one handle and the same maps, alternating: what the box does meanwhile meets both alike
        maps = torch.as_tensor(levels(prob, m)).cuda()
        env = BatchedPcgrlEnv(prob=prob, rep="wide", num_envs=1, seed=0)
        env.adjust_param(width=W, height=H)
        calls = {"evaluate": lambda: env.evaluate(maps), "playthrough": lambda: env.playthrough(maps)}
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
            out["ran"] = int((r.agent > -2).sum().item())
            out["won"] = int((r.agent >= 0).sum().item())
            out["moves"] = int(r.length.to(torch.int64).sum().item())
            out["longest"] = int(r.length.max().item())
    assert env.check_status() == 0
    print("RESULT " + json.dumps(out), flush=True)


def main():
    args = sys.argv[1:]
    prob = "mdungeon"
    if args and args[0] == "--prob":
        prob, args = args[1], args[2:]
    if prob not in ("mdungeon", "ddave"):
        sys.exit("playthrough_bench: --prob mdungeon|ddave")
    m = int(args[0]) if args else 65536
    res = {}
    for route in ("pair", "own"):
        p = subprocess.run(["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.abspath(__file__), "--child", route, prob, str(m)],
                           capture_output=True, text=True)
        if p.returncode != 0:                    # a fault, an abort or the time limit: nothing more is started on the GPU
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            sys.exit("playthrough_bench: %s ended with status %d" % (route, p.returncode))
        r = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
        res[route] = r
        for k, ts in r["s"].items():
            ts = sorted(ts)
            med = ts[len(ts) // 2]
            print("%-16s %s M=%d  %d rounds  ms: min %.3f  median %.3f  max %.3f   M levels/s at the median: %.2f%s" % (
                k, prob, m, len(ts), ts[0] * 1e3, med * 1e3, ts[-1] * 1e3, m / med / 1e6,
                ("   planner ran %d, won %d, %d moves, longest %d" % (r["ran"], r["won"], r["moves"], r["longest"])) if k != "evaluate" else ""), flush=True)
    assert res["pair"]["checksum"]["evaluate"] == res["pair"]["checksum"]["playthrough"], "playthrough() and evaluate() disagree on the statistics rows"
    print(json.dumps(res))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3], int(sys.argv[4]))
    else:
        main()
