"""Register / scratch budgets of the kernels whose speed hangs on them -- checked on the compiler's assembly, no GPU needed.

A wavefront of gfx950 may use 512 / waves-per-SIMD vector registers: with more than 128, `k_stats_wide` (eight wavefronts a block)
drops from two blocks per CU to one (C5 steady state 49.5 -> 58 us when one extra store in `finalize_item` pushed it to 131, round 4),
and a kernel that spills pays in HBM traffic (`k_stats<sokoban>`: 95 MB of scratch writes a step until its instantiation lost the reset
code, round 4).  The parts of csrc/pcgrl_abi.hip that hold those kernels are compiled to assembly (`hipcc -S --cuda-device-only`, side
by side) and the `.amdhsa_` resource directives of the kernels are read."""
from concurrent.futures import ThreadPoolExecutor
import pytest
from host_kit import kernel_resources


@pytest.fixture(scope="module")
def resources():
    with ThreadPoolExecutor(2) as ex:
        stats, step = ex.map(kernel_resources, (1, 3))      # PART_STATS, PART_STEP_BINARY (csrc/pcgrl_abi.hip)
    return {**stats, **step}


def _find(resources, prefix):
    hits = {k: v for k, v in resources.items() if k.startswith(prefix)}
    assert hits, (prefix, sorted(resources)[:10])
    return hits


def test_wide_kernel_keeps_two_blocks_per_cu(resources):
    for name, (vgpr, _, scratch) in _find(resources, "void k_stats_wide<").items():
        assert vgpr <= 128 and scratch == 0, (name, vgpr, scratch)


def test_fused_step_kernels_fit_without_spills(resources):
    for name, (vgpr, _, scratch) in _find(resources, "void k_step<0,").items():
        assert vgpr <= 128 and scratch == 0, (name, vgpr, scratch)


def test_statistics_kernels_do_not_spill(resources):
    for name, (vgpr, _, scratch) in _find(resources, "void k_stats<").items():
        # (binary on 16-row maps of 33..64 columns through the two-launch pipeline -- cast representations, no_fused -- keeps a few
        #  dwords in scratch: a rarely taken instantiation, known since round 3)
        allowed = 64 if name.startswith("void k_stats<0, 16, unsigned long>") else 0
        assert vgpr <= 128 and scratch <= allowed, (name, vgpr, scratch)
