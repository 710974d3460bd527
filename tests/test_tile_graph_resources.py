"""Register / scratch budget of k_tile_graph (csrc/kernels_tile_graph.h), read off the compiler's assembly like
tests/test_changes_resources.py -- no GPU needed.  The kernel keeps up to twelve label or distance planes of a map in registers beside
its pass, source and reach planes: it must not spill, and in every (lane group, mask width) form it must stay within 128 vector
registers -- the line DESIGN section 3 names as deciding occupancy for the 64-bit forms (a wavefront of gfx950 may use
512 / waves-per-SIMD registers: four wavefronts a SIMD at 128).  profiles/tile_graph/NOTES.md has the counts."""
import os, re, subprocess, sys
import pytest
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gym_pcgrl_amd import _lib

PART_UPDATE = 2      # csrc/pcgrl_abi.hip: the part that holds the launchers of k_get_stats, k_get_paths and k_tile_graph


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
        res[name] = (g("next_free_vgpr"), g("next_free_sgpr"), g("private_segment_fixed_size"))
    return res


def test_tile_graph_kernel_does_not_spill_and_stays_within_128_registers(resources):
    kernels = {k: v for k, v in resources.items() if k.startswith("void k_tile_graph<")}
    # the forms with_lanes gives k_get_stats: sixteen lanes or a wavefront, 32- or 64-bit row masks
    assert sorted(kernels) == ["void k_tile_graph<16, unsigned int>", "void k_tile_graph<16, unsigned long>",
                               "void k_tile_graph<64, unsigned int>", "void k_tile_graph<64, unsigned long>"], sorted(kernels)
    for name, (vgpr, sgpr, scratch) in sorted(kernels.items()):
        print(name, "VGPRs", vgpr, "SGPRs", sgpr, "scratch", scratch)
        assert scratch == 0, (name, scratch)
        assert vgpr <= 128, (name, vgpr)
