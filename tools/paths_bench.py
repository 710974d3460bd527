#!/usr/bin/env python3
"""Maps/s of BatchedPcgrlEnv.paths() (pcgrl_get_paths) next to evaluate() (pcgrl_get_stats) on the same seeded random levels with the
problem's own tile probabilities (the levels of tools/evaluate_bench.py), on the GPU box: binary 14 x 14, zelda 11 x 16, binary 64 x 64.
Method of tools/solve_bench.py -- wall clock around the call with a device synchronisation, after a warm-up of each call, every child
process under a time limit so that a hang ends there, a child that fails ends the session; the box is shared, so evaluate() and paths()
run in ONE process on one handle, alternating, ROUNDS rounds: minimum, median and maximum of each.  paths() runs twice: with the default
max_len (H * W: every leg whole) and with max_len 64 (the rows a drawing loop of short legs would ask for).  The statistics rows of the
calls must agree, and the lengths must be the statistics' (path-length; key + door = path-length, enemy = nearest-enemy).  One JSON
line at the end.

    python tools/paths_bench.py [M14 [M11x16 [M64]]]          (defaults: 65536 65536 4096)
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
CASES = (("binary", 14, 14), ("zelda", 11, 16), ("binary", 64, 64))


def levels(prob, m, h, w):
    """M seeded random levels with the problem's own tile probabilities (what reset() draws)."""
    import numpy as np
    from gym_pcgrl_amd.envs.problems import PROBLEMS
    p = np.array(list(PROBLEMS[prob]()._prob.values()), dtype=np.float64)
    return np.random.RandomState(7).choice(len(p), size=(m, h, w), p=p / p.sum()).astype(np.uint8)


def timed(call, sync):
    t0 = time.perf_counter()
    r = call()
    sync()
    return time.perf_counter() - t0, r


def child(prob, h, w, m):
    import torch
    from gym_pcgrl_amd.envs import BatchedPcgrlEnv
    out = {"prob": prob, "h": h, "w": w, "M": m}
    sync = torch.cuda.synchronize
    maps = torch.as_tensor(levels(prob, m, h, w)).cuda()
    env = BatchedPcgrlEnv(prob=prob, rep="wide", num_envs=1, seed=0)
    env.adjust_param(width=w, height=h)
    short = min(64, h * w)
    calls = {"evaluate": lambda: env.evaluate(maps), "paths": lambda: env.paths(maps), "paths_%d" % short: lambda: env.paths(maps, max_len=short)}
    last = {}
    for k, c in calls.items():                  # warm-up: the handle, the workspace, the kernels' code objects, the allocator's blocks
        last[k] = c()
    sync()
    t = {k: [] for k in calls}
    for _ in range(ROUNDS):
        for k, c in calls.items():
            dt, last[k] = timed(c, sync)
            t[k].append(dt)
    out["s"] = t
    out["checksum"] = {k: int(r.rows[:, :env._layout.nstats].to(torch.int64).sum().item()) for k, r in last.items()}
    p, rows = last["paths"], last["paths"].rows
    ln = p.length.to(torch.int64)
    if prob == "binary":
        assert torch.equal(ln[ln[:, 0] >= 0, 0], rows[ln[:, 0] >= 0, 1].to(torch.int64))
    else:
        both = ln[:, 0] >= 0
        assert torch.equal(ln[both, 0] + ln[both, 1], rows[both, 6].to(torch.int64)) and torch.equal(ln[ln[:, 2] >= 0, 2], rows[ln[:, 2] >= 0, 5].to(torch.int64))
    assert torch.equal(p.cells[:, :, :short], last["paths_%d" % short].cells)
    out["legs"] = [int(v) for v in (ln >= 0).sum(0).tolist()]
    out["cells"] = int((ln + 1).clamp(min=0).sum().item())
    out["longest"] = int(ln.max().item())
    out["bytes_cells"] = {k: int(r.cells.numel() * 2) for k, r in last.items() if k != "evaluate"}
    assert env.check_status() == 0
    print("RESULT " + json.dumps(out), flush=True)


def main():
    args = [int(a) for a in sys.argv[1:]]
    ms = args + [65536, 65536, 4096][len(args):]
    res = []
    for (prob, h, w), m in zip(CASES, ms):
        p = subprocess.run(["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.abspath(__file__), "--child", prob, str(h), str(w), str(m)],
                           capture_output=True, text=True)
        if p.returncode != 0:                    # a fault, an abort or the time limit: nothing more is started on the GPU
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            sys.exit("paths_bench: %s %dx%d ended with status %d" % (prob, h, w, p.returncode))
        r = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
        res.append(r)
        assert len(set(r["checksum"].values())) == 1, "paths() and evaluate() disagree on the statistics rows"
        for k, ts in r["s"].items():
            ts = sorted(ts)
            med = ts[len(ts) // 2]
            print("%-7s %2dx%-2d %-9s M=%d  %d rounds  ms: min %.3f  median %.3f  max %.3f   M maps/s at the median: %.3f%s" % (
                prob, h, w, k, m, len(ts), ts[0] * 1e3, med * 1e3, ts[-1] * 1e3, m / med / 1e6,
                ("   legs %s, %d cells, longest %d, %.1f MB of rows" % (r["legs"], r["cells"], r["longest"], r["bytes_cells"][k] / 1e6)) if k != "evaluate" else ""), flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]))
    else:
        main()
