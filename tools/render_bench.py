#!/usr/bin/env python3
"""Store rate of the picture kernel (GPU box): k_render (pcgrl_render) at 4 096 pictures of binary 14 x 14 levels (196 608 B each,
0.8 GB) and as a 32 x 32 contact sheet of the same, next to k_obs (pcgrl_observe) and a plain device fill in the same session --
how close the picture writer is to what the memory system takes.  Device events around `iters` launches after five warm-up
launches; bytes = the size of the output tensor.  One JSON line at the end.

    python tools/render_bench.py [iters]
"""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch

from gym_pcgrl_amd import _lib
from gym_pcgrl_amd.envs import BatchedPcgrlEnv

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 200


def timed(fn, n=iters):
    for _ in range(5):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3     # us


def line(name, out, us, res):
    mb = out.numel() * out.element_size() / 1e6
    res[name] = {"MB": round(mb, 1), "us": round(us, 1), "TB/s": round(mb / us, 3)}
    print("%-34s %8.1f MB  %8.1f us  %5.2f TB/s" % (name, mb, us, mb / us), flush=True)


res = {}
env = BatchedPcgrlEnv(prob="binary", rep="narrow", num_envs=4096, seed=0)
env.reset()
stacked = torch.empty((4096, 256, 256, 3), dtype=torch.uint8, device="cuda")
line("k_render 4096 stacked", stacked, timed(lambda: env.render_batch(out=stacked)), res)
idx = torch.arange(1024, dtype=torch.int32, device="cuda")
sheet = torch.empty((32 * 256, 32 * 256, 3), dtype=torch.uint8, device="cuda")
line("k_render 32x32 sheet", sheet, timed(lambda: env.render_batch(idx, out=sheet, grid=(32, 32))), res)
line("fill (same 0.8 GB)", stacked, timed(lambda: stacked.fill_(1)), res)
line("fill (sheet)", sheet, timed(lambda: sheet.fill_(1)), res)
env.close()
del stacked, sheet

# k_obs in the same session: the crops the trainer takes (tools/obs_bench.py has the other shapes)
for prob, rep, n, oh, ow, onehot in (("binary", "narrow", 65536, 28, 28, 0), ("zelda", "narrow", 65536, 22, 22, 1)):
    env = BatchedPcgrlEnv(prob=prob, rep=rep, num_envs=n, seed=0)
    env.reset()
    out = torch.empty((n, oh, ow, env.get_num_tiles() if onehot else 1), dtype=torch.uint8, device="cuda")
    pad, L = env.get_border_tile(), env._lib
    us = timed(lambda: _lib.check(L.pcgrl_observe(env._handle, C.c_void_p(out.data_ptr()), oh, ow, 1, pad, onehot, env._stream()), "pcgrl_observe"))
    line("k_obs %s %dx%d d%d" % (prob, oh, ow, out.shape[-1]), out, us, res)
    line("fill (same bytes)  %s" % prob, out, timed(lambda: out.fill_(1)), res)
    env.close()
print(json.dumps(res))
