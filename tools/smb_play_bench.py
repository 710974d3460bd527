#!/usr/bin/env python3
"""Levels/s of BatchedPcgrlEnv.playthrough_smb() (pcgrl_get_smb_play: k_smb_play) next to evaluate() (for smb the scratch-environment
route: set_maps() of a private environment, that is k_smb) on the same maps: the 14 x 114 levels of tests/golden/stats_smb_14x114_p1500.npz
tiled to M maps, on the GPU box.  Method of tools/playthrough_bench.py: wall clock around the call with a device synchronisation, after a
warm-up, the child process under a time limit so that a hang ends there; the two calls run in ONE process on one handle, alternating,
20 rounds: minimum, median and maximum of each.  Their statistics rows must agree.  One JSON line at the end.

    python tools/smb_play_bench.py [M] [max_len]          (default: 4096 maps, max_len 255)
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
ROUNDS = 20
LIMIT_S = 240
FIXTURE = os.path.join(ROOT, "tests", "golden", "stats_smb_14x114_p1500.npz")


def child(m, max_len):
    import numpy as np
    import torch
    from gym_pcgrl_amd.envs import BatchedPcgrlEnv
    d = np.load(FIXTURE)
    base, power = d["maps"], int(d["solver_power"])
    maps = torch.as_tensor(np.ascontiguousarray(base[np.arange(m) % base.shape[0]])).cuda()
    env = BatchedPcgrlEnv(prob="smb", rep="wide", num_envs=1, seed=0)
    env._prob._solver_power = power
    env.adjust_param(width=base.shape[2], height=base.shape[1])
    sync = torch.cuda.synchronize
    calls = {"evaluate": lambda: env.evaluate(maps, chunk=m), "playthrough_smb": lambda: env.playthrough_smb(maps, max_len=max_len)}
    last = {k: c() for k, c in calls.items()}           # warm-up: the handles, the workspace, the kernels' code objects
    sync()
    t = {k: [] for k in calls}
    for _ in range(ROUNDS):
        for k, c in calls.items():
            t0 = time.perf_counter()
            last[k] = c()
            sync()
            t[k].append(time.perf_counter() - t0)
    pt = last["playthrough_smb"]
    assert torch.equal(pt.rows, last["evaluate"].rows), "playthrough_smb() and evaluate() disagree on the statistics rows"
    assert env.check_status() == 0
    out = {"M": m, "max_len": max_len, "power": power, "s": t, "won": int((pt.agent >= 0).sum().item()), "second_agent": int((pt.agent != 0).sum().item()),
           "moves": int(pt.length.to(torch.int64).sum().item()), "longest": int(pt.length.max().item()),
           "pops": [int(d["agents"][np.arange(m) % base.shape[0], k].sum()) for k in (0, 1)]}
    print("RESULT " + json.dumps(out), flush=True)


def main():
    m = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    max_len = int(sys.argv[2]) if len(sys.argv) > 2 else 255
    p = subprocess.run(["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.abspath(__file__), "--child", str(m), str(max_len)], capture_output=True, text=True)
    if p.returncode != 0:                    # a fault, an abort or the time limit: nothing more is started on the GPU
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        sys.exit("smb_play_bench: ended with status %d" % p.returncode)
    r = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    for k, ts in r["s"].items():
        ts = sorted(ts)
        med = ts[len(ts) // 2]
        print("%-16s M=%d  %d rounds  ms: min %.3f  median %.3f  max %.3f   levels/s at the median: %.0f" % (k, m, len(ts), ts[0] * 1e3, med * 1e3, ts[-1] * 1e3, m / med), flush=True)
    print("won %d of %d, the second agent played %d, %d moves, longest %d; pops of the two agents %s" % (r["won"], m, r["second_agent"], r["moves"], r["longest"], r["pops"]))
    print(json.dumps(r))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(int(sys.argv[2]), int(sys.argv[3]))
    else:
        main()
