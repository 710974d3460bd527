"""Every one-cell change of a level, without a GPU: the host side of pcgrl_get_changes_bytes / pcgrl_get_changes, the in-register edit of
k_get_changes (planes_set_cell, csrc/pcgrl_algos.h) on the CPU lane-group simulator (tests/hostsim/sim_changes.cpp), and the expansion
rule of changes()' fallback -- entry order (m, k, t), no-op entries -- against hand levels scored by the oracle alone."""
import ctypes as C
import re

import numpy as np
import pytest

import oracle_lib
from host_kit import config as _config, header, plain_header, prototype, run_sanitized
from hostsim_build import build_so
from oracle_lib import _p

NTILES = {"binary": 2, "zelda": 8, "sokoban": 5, "mdungeon": 8, "ddave": 7, "smb": 7}
# the shapes of tests/test_gpu_changes.py: (problem, rows, columns)
SHAPES = [("binary", 1, 1), ("binary", 3, 5), ("binary", 16, 32), ("binary", 16, 33), ("binary", 17, 32), ("binary", 17, 33), ("binary", 64, 64),
          ("zelda", 7, 11), ("zelda", 17, 33)]


def test_declared_exported_and_mirrored():
    from gym_pcgrl_amd import _lib
    hdr, plain = header(), plain_header()
    assert re.search(prototype("size_t", "pcgrl_get_changes_bytes", ["const pcgrl_config*", "int32_t", "int32_t"]), plain)
    assert re.search(prototype("int", "pcgrl_get_changes", ["pcgrl_env*", "const uint8_t*", "int32_t", "const int32_t*", "int32_t", "const int32_t*", "int32_t*", "int32_t*",
                                                           "double*", "uint8_t*", "void*", "size_t", "void*"]), plain)
    assert "Still 15: + pcgrl_get_changes_bytes / pcgrl_get_changes" in hdr
    L = _lib.load()
    for name in ("pcgrl_get_changes_bytes", "pcgrl_get_changes"):
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert L.pcgrl_abi_version() == _lib.ABI_VERSION == 15
    assert L.pcgrl_get_changes_bytes.argtypes == [C.POINTER(_lib.Config), C.c_int32, C.c_int32] and L.pcgrl_get_changes_bytes.restype == C.c_size_t
    assert L.pcgrl_get_changes.argtypes == [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32] + [C.c_void_p] * 6 + [C.c_size_t, C.c_void_p]
    # refused without a handle, not crashed
    assert L.pcgrl_get_changes(None, None, 1, None, 1, None, None, None, None, None, None, 0, None) == _lib.PCGRL_ESTATE
    # the developer switches of the call are the struct's last two, and the defaults fill them
    assert _lib.TUNING_FIELDS[-2:] == ("changes_grid", "changes_chunk") and re.search(r"int32_t\s+changes_chunk;[^}]*\}\s*pcgrl_tuning;", plain, re.S)
    t = _lib.Tuning()
    L.pcgrl_tuning_defaults(C.byref(t))
    assert t.changes_grid == -1 and t.changes_chunk == -1


def test_workspace_sizes():
    from gym_pcgrl_amd import _lib
    L = _lib.load()
    grid = [("binary", 5, 5, None), ("binary", 64, 64, None), ("binary", 16, 33, None), ("zelda", 7, 11, None), ("zelda", 64, 64, None),
            ("sokoban", 5, 5, None), ("sokoban", 14, 14, None), ("mdungeon", 7, 11, None), ("ddave", 7, 11, None), ("sokoban", 5, 5, 5000),
            # no fast form: smb, 65 x 64, a search level of more than 256 bordered cells, solver_power beyond the searches in LDS
            ("smb", 8, 20, None), ("binary", 65, 64, None), ("zelda", 64, 65, None), ("sokoban", 15, 15, None), ("mdungeon", 15, 15, None),
            ("sokoban", 5, 5, 5001), ("ddave", 7, 11, 5001)]
    zero = {("smb", 8, 20, None), ("binary", 65, 64, None), ("zelda", 64, 65, None), ("sokoban", 15, 15, None), ("mdungeon", 15, 15, None),
            ("sokoban", 5, 5, 5001), ("ddave", 7, 11, 5001)}
    for case in grid:
        prob, h, w, power = case
        cfg = _config(prob, h, w, power)
        T = NTILES[prob]
        for count in (1, 3, 64, 65, 1000):
            for ncells in (1, 2, h * w, 4 * h * w):
                stats = int(L.pcgrl_get_stats_bytes(C.byref(cfg), count))
                n = int(L.pcgrl_get_changes_bytes(C.byref(cfg), count, ncells))
                assert (stats == 0) == (case in zero), case
                assert (n >= 256) if stats else (n == 0), (case, count, ncells, n)
        for count, ncells in ((0, 4), (-1, 4), (4, 0), (4, -1)):
            assert int(L.pcgrl_get_changes_bytes(C.byref(cfg), count, ncells)) == 0, (case, count, ncells)
        if case not in zero:
            # the documented bound: count * ncells * T + count <= 2^31 - 1
            count = 1 << 16
            at = ((1 << 31) - 1 - count) // (count * T)
            assert int(L.pcgrl_get_changes_bytes(C.byref(cfg), count, at)) >= 256, case
            assert int(L.pcgrl_get_changes_bytes(C.byref(cfg), count, at + 1)) == 0, case
            assert int(L.pcgrl_get_changes_bytes(C.byref(cfg), 1 << 30, 4096)) == 0 and int(L.pcgrl_get_changes_bytes(C.byref(cfg), (1 << 31) - 1, 1)) == 0
    assert int(L.pcgrl_get_changes_bytes(None, 4, 4)) == 0


def test_workspace_is_monotone():
    from gym_pcgrl_amd import _lib
    L = _lib.load()
    for prob, h, w in (("binary", 14, 14), ("zelda", 7, 11), ("sokoban", 5, 5), ("mdungeon", 7, 11), ("ddave", 7, 11)):
        cfg = _config(prob, h, w)
        counts, cells = (1, 2, 7, 63, 64, 65, 500, 4096, 100000), (1, 2, 3, h * w - 1, h * w, 2 * h * w)
        size = np.array([[int(L.pcgrl_get_changes_bytes(C.byref(cfg), c, k)) for k in cells] for c in counts], np.int64)
        assert (size >= 256).all() and (np.diff(size, axis=0) >= 0).all() and (np.diff(size, axis=1) >= 0).all(), (prob, size)


# ------------------------------------------------------------------ the in-register edit on the lane-group simulator
@pytest.fixture(scope="module")
def sim():
    L = build_so("sim_changes.cpp")
    L.sim_changes.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    L.sim_changes.restype = C.c_long
    return L


def _levels(prob, h, w):
    """A few seeded random levels, all of the first tile and all of the last."""
    rs = np.random.RandomState(h * 100 + w)
    T = NTILES[prob]
    return [rs.randint(0, T, size=(h, w)).astype(np.uint8) for _ in range(3)] + [np.zeros((h, w), np.uint8), np.full((h, w), T - 1, np.uint8)]


def test_edit_and_restore_on_every_form(sim):
    """Every cell and tile of levels at the GPU tests' shapes, at 16 and 64 lanes and both mask widths where the form holds the map: the
    planes after the edit are those of the edited bytes, only the owning row changed, the kept originals are the level's."""
    seen = set()
    for prob, h, w in SHAPES:
        T = NTILES[prob]
        for m in _levels(prob, h, w):
            for group in (16, 64):
                for bits in (32, 64):
                    n = sim.sim_changes(_p(np.ascontiguousarray(m)), h, w, T, group, bits)
                    if h > group or w > bits:
                        assert n == -1000000000, (prob, h, w, group, bits)
                        continue
                    assert n == h * w * T, (prob, h, w, group, bits, n)
                    seen.add((group, bits))
    assert seen == {(16, 32), (16, 64), (64, 32), (64, 64)}


def test_sanitized_stand_alone_program():
    """sim_changes.cpp with its own main(), built with the address and undefined-behaviour sanitizers and run as a program."""
    run_sanitized("sim_changes.cpp", "SIM_CHANGES_MAIN", 300)


# ------------------------------------------------------------------ the fallback's expansion rule, through the oracle alone
HAND = {
    "binary": np.array([[[0, 1, 0], [0, 0, 1]], [[1, 1, 1], [1, 0, 1]]], np.uint8),
    "zelda": np.array([[[2, 0, 3], [1, 5, 4]], [[0, 0, 0], [7, 2, 2]]], np.uint8),
    "sokoban": np.array([[[2, 3, 4], [0, 0, 1]], [[0, 0, 0], [3, 4, 2]]], np.uint8),
}


@pytest.mark.parametrize("prob", sorted(HAND))
def test_expansion_rule_against_hand_levels(prob):
    import torch
    from gym_pcgrl_amd.envs.batched_env import expand_changes
    maps = HAND[prob]
    M, h, w = maps.shape
    T = NTILES[prob]
    cells = np.array([[5, 0, 0, 3], [1, 4, 2, 2]], np.int64)             # repeats, another list per level
    K = cells.shape[1]
    E = M * K * T
    flat = torch.as_tensor(maps.reshape(M, h * w))
    parts = [expand_changes(flat, torch.as_tensor(cells), i, min(7, E - i), T) for i in range(0, E, 7)]      # (chunks that cut across cells and levels)
    levels = torch.cat([p[0] for p in parts]).numpy().reshape(E, h, w)
    lv, noop = torch.cat([p[1] for p in parts]).numpy(), torch.cat([p[2] for p in parts]).numpy()
    assert np.array_equal(flat.numpy(), maps.reshape(M, h * w))          # the input is left as it was
    base = [oracle_lib.get_stats(prob, maps[m]) for m in range(M)]
    n_noop = 0
    for m in range(M):
        for k in range(K):
            for t in range(T):
                e = (m * K + k) * T + t
                want = maps[m].copy()
                want[cells[m, k] // w, cells[m, k] % w] = t
                assert np.array_equal(levels[e], want) and lv[e] == m, (m, k, t)
                assert bool(noop[e]) == (maps[m].reshape(-1)[cells[m, k]] == t), (m, k, t)
                if noop[e]:
                    assert np.array_equal(oracle_lib.get_stats(prob, levels[e]), base[m])
                    n_noop += 1
    assert n_noop == M * K                                               # one tile per (level, cell)
    # a tile id beyond the last counts as the last one
    bad = flat.clone()
    bad[0, 5] = 200
    _, _, noop_bad = expand_changes(bad, torch.as_tensor(cells), 0, T, T)
    assert noop_bad.numpy().tolist() == [False] * (T - 1) + [True]
