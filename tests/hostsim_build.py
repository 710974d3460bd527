"""The CPU simulators under tests/hostsim, built when they are older than their sources: a shared library for ctypes, or -- a file
with a main() of its own behind a define -- a stand-alone program with the address and undefined-behaviour sanitizers."""
import ctypes as C
import glob
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
HOSTSIM = os.path.join(HERE, "hostsim")
CSRC = os.path.join(os.path.dirname(HERE), "gym_pcgrl_amd", "csrc")


def _build(out, src, flags):
    """(a simulator may include another one: every simulator source and header and every kernel header counts as a source of each)"""
    deps = glob.glob(os.path.join(HOSTSIM, "*.cpp")) + glob.glob(os.path.join(HOSTSIM, "*.h")) + glob.glob(os.path.join(CSRC, "*.h"))
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++"] + list(flags) + ["-o", out, os.path.join(HOSTSIM, src)])
    return out


def build_so(src, extra_flags=()):
    """tests/hostsim/sim_x.cpp -> libsim_x.so beside it, loaded."""
    so = os.path.join(HOSTSIM, "lib" + os.path.splitext(src)[0] + ".so")
    return C.CDLL(_build(so, src, ["-O2", "-std=c++17", "-fPIC", "-shared"] + list(extra_flags)))


def build_sanitized(src, main_define):
    """tests/hostsim/sim_x.cpp with -D<main_define> -> the path of the sanitized program sim_x_san beside it."""
    exe = os.path.join(HOSTSIM, os.path.splitext(src)[0] + "_san")
    return _build(exe, src, ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-D" + main_define])
