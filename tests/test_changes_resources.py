"""Register / scratch budget of k_get_changes (csrc/kernels_changes.h), read off the compiler's assembly like tests/test_kernel_resources.py
-- no GPU needed.  The kernel keeps a level's planes and rows across the statistics of every changed level: it must not spill, and for every
(problem, lane group, mask width) it is built for its vector registers must allow the wavefronts per SIMD that k_get_stats has for the same
form -- a wavefront of gfx950 may use 512 / waves-per-SIMD registers, allocated in steps of 8."""
import os, re, subprocess, sys
import pytest
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gym_pcgrl_amd import _lib

PART_UPDATE = 2      # csrc/pcgrl_abi.hip: the part that holds the launchers of k_get_stats and k_get_changes


def waves_per_simd(vgpr):
    alloc = (vgpr + 7) // 8 * 8
    return min(8, 512 // alloc)


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    out = os.path.join(str(tmp_path_factory.mktemp("asm")), "part%d.s" % PART_UPDATE)
    hipcc = os.environ.get("HIPCC", "hipcc")
    subprocess.check_call([hipcc] + [f for f in _lib.HIPCC_FLAGS if f != "-shared"] + ["-DPCGRL_PART=%d" % PART_UPDATE, "--cuda-device-only", "-S", _lib.SOURCES[0], "-o", out],
                          stderr=subprocess.DEVNULL)
    res = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", open(out).read(), re.S):
        name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip().split("(")[0]
        g = lambda k: int(re.search(k + r"\s+(\d+)", m.group(2)).group(1))
        res[name] = (g("next_free_vgpr"), g("private_segment_fixed_size"))
    return res


def test_changes_kernel_does_not_spill_and_keeps_the_occupancy_of_get_stats(resources):
    changes = {k: v for k, v in resources.items() if k.startswith("void k_get_changes<")}
    # binary, zelda, sokoban, mdungeon, ddave x the forms the launcher takes: sixteen lanes with 32-bit masks, a wavefront with either
    assert len(changes) == 15, sorted(changes)
    for name, (vgpr, scratch) in changes.items():
        form = name[len("void k_get_changes"):]
        stats_vgpr, _ = resources["void k_get_stats" + form]
        print(name, vgpr, scratch, "k_get_stats:", stats_vgpr)
        assert scratch == 0, (name, scratch)
        assert waves_per_simd(vgpr) >= waves_per_simd(stats_vgpr), (name, vgpr, stats_vgpr)
