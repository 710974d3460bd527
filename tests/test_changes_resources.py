"""Register / scratch budget of k_get_changes (csrc/kernels_changes.h), read off the compiler's assembly like tests/test_kernel_resources.py
-- no GPU needed.  The kernel keeps a level's planes and rows across the statistics of every changed level: it must not spill, and for every
(problem, lane group, mask width) it is built for its vector registers must allow the wavefronts per SIMD that k_get_stats has for the same
form -- a wavefront of gfx950 may use 512 / waves-per-SIMD registers, allocated in steps of 8."""
from host_kit import kernel_resources

PART_UPDATE = 2      # csrc/pcgrl_abi.hip: the part that holds the launchers of k_get_stats and k_get_changes


def waves_per_simd(vgpr):
    alloc = (vgpr + 7) // 8 * 8
    return min(8, 512 // alloc)


def test_changes_kernel_does_not_spill_and_keeps_the_occupancy_of_get_stats():
    resources = kernel_resources(PART_UPDATE)
    changes = {k: v for k, v in resources.items() if k.startswith("void k_get_changes<")}
    # binary, zelda, sokoban, mdungeon, ddave x the forms the launcher takes: sixteen lanes with 32-bit masks, a wavefront with either
    assert len(changes) == 15, sorted(changes)
    for name, (vgpr, _, scratch) in changes.items():
        form = name[len("void k_get_changes"):]
        stats_vgpr = resources["void k_get_stats" + form][0]
        print(name, vgpr, scratch, "k_get_stats:", stats_vgpr)
        assert scratch == 0, (name, scratch)
        assert waves_per_simd(vgpr) >= waves_per_simd(stats_vgpr), (name, vgpr, stats_vgpr)
