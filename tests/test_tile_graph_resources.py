"""Register / scratch budget of k_tile_graph (csrc/kernels_tile_graph.h), read off the compiler's assembly like
tests/test_changes_resources.py -- no GPU needed.  The kernel keeps up to twelve label or distance planes of a map in registers beside
its pass, source and reach planes: it must not spill, and in every (lane group, mask width) form it must stay within 128 vector
registers -- the line DESIGN section 3 names as deciding occupancy for the 64-bit forms (a wavefront of gfx950 may use
512 / waves-per-SIMD registers: four wavefronts a SIMD at 128).  profiles/tile_graph/NOTES.md has the counts."""
from host_kit import kernel_resources

PART_UPDATE = 2      # csrc/pcgrl_abi.hip: the part that holds the launchers of k_get_stats, k_get_paths and k_tile_graph


def test_tile_graph_kernel_does_not_spill_and_stays_within_128_registers():
    resources = kernel_resources(PART_UPDATE)
    kernels = {k: v for k, v in resources.items() if k.startswith("void k_tile_graph<")}
    # the forms with_lanes gives k_get_stats: sixteen lanes or a wavefront, 32- or 64-bit row masks
    assert sorted(kernels) == ["void k_tile_graph<16, unsigned int>", "void k_tile_graph<16, unsigned long>",
                               "void k_tile_graph<64, unsigned int>", "void k_tile_graph<64, unsigned long>"], sorted(kernels)
    for name, (vgpr, sgpr, scratch) in sorted(kernels.items()):
        print(name, "VGPRs", vgpr, "SGPRs", sgpr, "scratch", scratch)
        assert scratch == 0, (name, scratch)
        assert vgpr <= 128, (name, vgpr)
