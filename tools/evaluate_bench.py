#!/usr/bin/env python3
"""Maps/s of BatchedPcgrlEnv.evaluate() (pcgrl_get_stats) at M levels, next to the route there was before it -- a handle of M
environments: reset(); set_maps(maps); stats -- on the same box in the same session (GPU box).  Per problem three runs of each
route, wall-clock around the call with a device synchronisation; the handle route is timed with and without building the handle
(allocation + seeding + reset), which that route needs once per batch size.  Every route runs in a child process of its own under a
time limit, so that a hang ends there; a child that fails ends the session.  One JSON line at the end.

    python tools/evaluate_bench.py [M] [problem ...]          (default: 65536 binary zelda sokoban)
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
SHAPES = {"binary": (14, 14), "zelda": (11, 16), "sokoban": (5, 5), "mdungeon": (11, 7), "ddave": (7, 11)}      # rows, columns
RUNS = 3
LIMIT_S = 240


def levels(prob, m):
    """M seeded random levels with the problem's own tile probabilities (what reset() draws)."""
    import numpy as np
    from gym_pcgrl_amd.envs.problems import PROBLEMS
    p = np.array(list(PROBLEMS[prob]()._prob.values()), dtype=np.float64)
    h, w = SHAPES[prob]
    return np.random.RandomState(7).choice(len(p), size=(m, h, w), p=p / p.sum()).astype(np.uint8)


def child(route, prob, m):
    import torch
    from gym_pcgrl_amd.envs import BatchedPcgrlEnv
    h, w = SHAPES[prob]
    maps = torch.as_tensor(levels(prob, m)).cuda()
    out = {"route": route, "prob": prob, "M": m}
    sync = torch.cuda.synchronize
    if route == "evaluate":
        env = BatchedPcgrlEnv(prob=prob, rep="wide", num_envs=1, seed=0)
        env.adjust_param(width=w, height=h)
        rows = env.evaluate(maps).rows          # warm-up: the handle, the workspace, the kernels' code objects
        sync()
        t = []
        for _ in range(RUNS):
            t0 = time.perf_counter()
            rows = env.evaluate(maps).rows
            sync()
            t.append(time.perf_counter() - t0)
        out["s"] = t
        out["checksum"] = int(rows[:, :env._layout.nstats].to(torch.int64).sum().item())
    else:
        t, tb = [], []
        for _ in range(RUNS + 1):               # (the first pass is the warm-up)
            t0 = time.perf_counter()
            env = BatchedPcgrlEnv(prob=prob, rep="wide", num_envs=m, seed=0)
            env.adjust_param(width=w, height=h)
            env.reset()
            sync()
            t1 = time.perf_counter()
            env.set_maps(maps)
            rows = env._bufs["stats"]
            sync()
            t2 = time.perf_counter()
            tb.append(t2 - t0)
            t.append(t2 - t1)
            out["checksum"] = int(rows[:, :env._layout.nstats].to(torch.int64).sum().item())
            env.close()
        out["s"] = t[1:]
        out["s_with_handle"] = tb[1:]
    print("RESULT " + json.dumps(out), flush=True)


def main():
    args = sys.argv[1:]
    m = int(args[0]) if args and args[0].isdigit() else 65536
    probs = [a for a in args if not a.isdigit()] or ["binary", "zelda", "sokoban"]
    res = {}
    for prob in probs:
        for route in ("evaluate", "handle"):
            p = subprocess.run(["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.abspath(__file__), "--child", route, prob, str(m)],
                               capture_output=True, text=True)
            if p.returncode != 0:                # a fault, an abort or the time limit: nothing more is started on the GPU
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                sys.exit("evaluate_bench: %s / %s ended with status %d" % (prob, route, p.returncode))
            r = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
            res.setdefault(prob, {})[route] = r
            rate = lambda ts: " ".join("%9.3f" % (m / s / 1e6) for s in ts)
            print("%-8s %-8s M=%d  M maps/s: %s%s" % (prob, route, m, rate(r["s"]),
                                                      ("   with the handle built: " + rate(r["s_with_handle"])) if "s_with_handle" in r else ""), flush=True)
        assert res[prob]["evaluate"]["checksum"] == res[prob]["handle"]["checksum"], (prob, "the two routes disagree")
    print(json.dumps(res))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3], int(sys.argv[4]))
    else:
        main()
