"""Register / scratch budget of k_tile_local (csrc/kernels_tile_local.h), read off the compiler's assembly like
tests/test_tile_graph_resources.py -- no GPU needed.  The kernel indexes the caller's offsets by a loop counter and keeps sixteen packed
tile counters a lane: neither may end up in scratch, and every form must stay within 128 vector registers (four wavefronts a SIMD).
profiles/tile_local/NOTES.md has the counts."""
from host_kit import kernel_resources

PART_UPDATE = 2      # csrc/pcgrl_abi.hip: the part that holds the launchers of k_get_stats, k_tile_graph and k_tile_local


def test_tile_local_kernel_does_not_spill_and_stays_within_128_registers():
    resources = kernel_resources(PART_UPDATE)
    kernels = {k: v for k, v in resources.items() if k.startswith("void k_tile_local<")}
    # sixteen lanes or a wavefront on the LDS stage, a wavefront on the caller's bytes
    assert sorted(kernels) == ["void k_tile_local<16, true>", "void k_tile_local<64, false>", "void k_tile_local<64, true>"], sorted(kernels)
    for name, (vgpr, sgpr, scratch) in sorted(kernels.items()):
        print(name, "VGPRs", vgpr, "SGPRs", sgpr, "scratch", scratch)
        assert scratch == 0, (name, scratch)
        assert vgpr <= 128, (name, vgpr)
