"""The paths behind binary's path-length and zelda's path-length / nearest-enemy, without a GPU: the templates of
gym_pcgrl_amd/csrc/path_trace.h on the CPU lane-group simulator (tests/hostsim/sim_paths.cpp) against the legs that the reference's
run_dikjstra maps define (tests/golden/paths.npz), the host check check_path(), and the host side of pcgrl_get_paths_legs /
pcgrl_get_paths_bytes / pcgrl_get_paths."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from host_kit import config as _config, forms, header, plain_header, prototype, run_sanitized
from hostsim_build import build_so
from oracle_lib import _p

HERE = os.path.dirname(os.path.abspath(__file__))
G = os.path.join(HERE, "golden")
PROB_ID = {"binary": 0, "zelda": 1}
# what a leg may walk on (zelda_prob.py:98, :107, :109; binary_prob.py:84): tile ids
PASSABLE = {"binary": [[0]], "zelda": [[0, 2, 3, 5, 6, 7], [0, 2, 3, 4, 5, 6, 7], [0, 2, 5, 6, 7]]}


def groups(fix):
    """(name, problem, maps, stats) of every group of the fixture, in its order."""
    for name in fix["groups"].tolist():
        prob = name.split("_")[1]
        if name.startswith("stats_"):
            d = np.load(os.path.join(G, name + ".npz"))
            yield name, prob, d["maps"], d["stats"]
        else:
            yield name, prob, fix["maps_" + name], fix["stats_" + name]


@pytest.fixture(scope="module")
def sim():
    L = build_so("sim_paths.cpp")
    L.sim_paths.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


@pytest.fixture(scope="module")
def fix():
    return np.load(os.path.join(G, "paths.npz"))


def _run(L, prob, m, group, bits, max_len):
    m = np.ascontiguousarray(m, np.uint8)
    legs = len(PASSABLE[prob])
    cells = np.full(legs * max_len + 2, 77, np.int16)              # two guard words behind the rows
    length, row = np.full(3, -9, np.int32), np.full(8, -9, np.int32)
    rc = L.sim_paths(PROB_ID[prob], _p(m), m.shape[0], m.shape[1], group, bits, max_len, _p(cells), _p(length), _p(row))
    assert rc == 0 and (cells[legs * max_len:] == 77).all()
    return cells[:legs * max_len].reshape(legs, max_len), length[:legs], row


def test_every_fixture_row_on_every_form(sim, fix):
    """cells, length and the statistics row of every level, with 16 and 64 lanes and both mask widths where the map fits."""
    seen, n = set(), 0
    for name, prob, maps, stats in groups(fix):
        want, wlen = fix["cells_" + name], fix["length_" + name]
        assert want.shape[0] == maps.shape[0] == wlen.shape[0] and want.dtype == np.int16 and wlen.dtype == np.int32
        assert np.array_equal((want >= 0).sum(2), wlen + 1)
        h, w = maps.shape[1:]
        ns = stats.shape[1]
        for group, bits in forms(h, w):
            for i, m in enumerate(maps):
                cells, length, row = _run(sim, prob, m, group, bits, want.shape[2])
                assert np.array_equal(length, wlen[i]), (name, i, group, bits, length, wlen[i])
                assert np.array_equal(cells, want[i]), (name, i, group, bits)
                assert row[:ns].tolist() == stats[i].tolist(), (name, i, group, bits, row)
                n += 1
            seen.add((group, bits))
    assert seen == {(16, 32), (16, 64), (64, 32), (64, 64)} and n > 5000


def test_identities_with_the_statistics(fix):
    for name, prob, maps, stats in groups(fix):
        ln = fix["length_" + name]
        if prob == "binary":
            has = ln[:, 0] >= 0
            assert np.array_equal(ln[has, 0], stats[has, 1]) and np.array_equal(has, (maps == 0).any((1, 2)))
        else:
            both = (stats[:, 0] == 1) & (stats[:, 4] == 1) & (stats[:, 1] == 1) & (stats[:, 2] == 1)
            assert np.array_equal(ln[:, 0] >= 0, both) and (ln[~both, 1] == -1).all()
            assert np.array_equal(ln[both, 0] + ln[both, 1], stats[both, 6])
            en = ln[:, 2] >= 0
            assert np.array_equal(ln[en, 2], stats[en, 5]) and np.array_equal(en, fix["ties_" + name] > 0)


def test_truncated_rows_are_prefixes(sim, fix):
    for name, prob in (("stats_binary_14x14", "binary"), ("stats_zelda_7x11", "zelda"), ("hand_binary_64x64", "binary")):
        _, _, maps, _ = next(g for g in groups(fix) if g[0] == name)
        want, wlen = fix["cells_" + name], fix["length_" + name]
        i = int(np.argmax(wlen.min(1)))                     # (zelda: a level with all three legs)
        assert wlen[i].min() >= 1
        h, w = maps.shape[1:]
        for full in sorted(set(wlen[i].tolist())):
            for max_len in (1, 2, full, full + 1, full + 2):
                for group, bits in forms(h, w):
                    cells, length, _ = _run(sim, prob, maps[i], group, bits, max_len)
                    assert np.array_equal(length, wlen[i])
                    for leg in range(len(length)):
                        k = min(length[leg] + 1, max_len)
                        assert np.array_equal(cells[leg, :k], want[i, leg, :k]) and (cells[leg, k:] == -1).all(), (name, max_len, leg)


def test_fixture_covers_what_the_issue_lists(fix):
    names = fix["groups"].tolist()
    for g in ("stats_binary_14x14", "stats_binary_5x5"):
        assert int((fix["ties_" + g] >= 2).sum()) >= 10, g              # several regions reach the maximum
    ln, ties = fix["length_stats_zelda_7x11"], fix["ties_stats_zelda_7x11"]
    assert int(((ln[:, 0] >= 0) & (ln[:, 1] == -1)).sum()) >= 10         # the door walled off
    assert int((ties >= 2).sum()) >= 10                                  # two or more nearest enemies
    none = 0
    for name, prob, maps, stats in groups(fix):
        if prob == "zelda":
            none += int(((stats[:, 0] == 1) & (stats[:, 4] == 1) & (stats[:, 3] > 0) & (fix["length_" + name][:, 2] == -1)).sum())
    assert none >= 1                                                     # enemies, none reachable
    # a level with a leg in every (lane group, mask width) corner the library takes
    corners = {("binary", 5, 40), ("zelda", 5, 40), ("binary", 16, 33), ("zelda", 16, 33), ("binary", 16, 32), ("binary", 17, 9),
               ("zelda", 17, 9), ("binary", 17, 33)}
    for name, prob, maps, _ in groups(fix):
        if (fix["length_" + name] >= 0).any():
            corners.discard((prob, maps.shape[1], maps.shape[2]))
    assert not corners, corners
    # the hand-made levels
    assert "hand_binary_64x64" in names and int(fix["length_hand_binary_64x64"][0, 0]) == 2079 and int(fix["length_hand_binary_64x64"][1, 0]) == 126
    twin = fix["cells_hand_binary_3x7"][0, 0]
    assert int(fix["ties_hand_binary_3x7"][0]) == 2 and (twin[twin >= 0] % 7 < 3).all()      # the first of two equal regions
    hz, ht = fix["length_hand_zelda_7x11"], fix["ties_hand_zelda_7x11"]
    assert hz[0, 0] > 0 and hz[0, 1] == -1                               # the door walled off
    assert ht[1] == 2 and hz[1, 2] > 0                                   # two enemies at the nearest distance
    assert hz[2, 2] == -1 and fix["stats_hand_zelda_7x11"][2, 3] == 2 and fix["stats_hand_zelda_7x11"][2, 5] == 77      # only through the key
    assert os.path.getsize(os.path.join(G, "paths.npz")) < 300 * 1024


def test_sanitized_stand_alone_program():
    """sim_paths.cpp with its own main(), built with the address and undefined-behaviour sanitizers and run as a program: built-in
    levels through every leg on every (lane group, mask width) form, with guard words behind the rows."""
    run_sanitized("sim_paths.cpp", "SIM_PATHS_MAIN", 120)


# ------------------------------------------------------------------ check_path(): the check that owes nothing to a fixture
def test_check_path_rules():
    from gym_pcgrl_amd import check_path
    lv = np.array([[0, 0, 1],
                   [1, 0, 0]], np.uint8)
    r = check_path(lv, [0, 1, 4, 5], [0])
    assert r.ok and r.legal.tolist() == [True] * 4
    assert check_path(lv, [0, 1, 4, 5, -1, 2], [0]).legal.shape == (4,)                 # a negative entry ends the list
    r = check_path(lv, [0, 4], [0])                                                     # a diagonal step
    assert not r.ok and r.legal.tolist() == [True, False]
    r = check_path(lv, [1, 2], [0])                                                     # a cell on a wall
    assert not r.ok and r.legal.tolist() == [True, False]
    assert check_path(lv, [1, 2], [0, 1]).ok
    r = check_path(lv, [0, 1, 0], [0])                                                  # a repeat
    assert not r.ok and r.legal.tolist() == [True, True, False]
    r = check_path(lv, [5, 6], [0])                                                     # out of range
    assert not r.ok and r.legal.tolist() == [True, False]
    assert not check_path(lv, [2, 3], [0, 1]).ok                                        # the end of a row is not next to the start of the next
    assert check_path(lv, [], [0]).ok and check_path(lv, [-1, 3], [0]).legal.shape == (0,)
    with pytest.raises(ValueError):
        check_path(np.zeros(4, np.uint8), [0], [0])


def test_check_path_accepts_every_fixture_leg(fix):
    from gym_pcgrl_amd import check_path
    n = 0
    for name, prob, maps, _ in groups(fix):
        cells, ln = fix["cells_" + name], fix["length_" + name]
        for i, leg in zip(*np.nonzero(ln >= 0)):
            r = check_path(maps[i], cells[i, leg], PASSABLE[prob][leg])
            assert r.ok and r.legal.shape == (ln[i, leg] + 1,), (name, i, leg)
            n += 1
    assert n > 1500


# ------------------------------------------------------------------ the ABI, without a device
def test_declared_exported_and_mirrored():
    from gym_pcgrl_amd import _lib
    hdr, plain = header(), plain_header()
    assert re.search(prototype("int32_t", "pcgrl_get_paths_legs", ["const pcgrl_config*"]), plain)
    assert re.search(prototype("size_t", "pcgrl_get_paths_bytes", ["const pcgrl_config*", "int32_t", "int32_t"]), plain)
    assert re.search(prototype("int", "pcgrl_get_paths", ["pcgrl_env*", "const uint8_t*", "int32_t", "int32_t", "int16_t*", "int32_t*", "int32_t*", "void*", "size_t", "void*"]), plain)
    for cited in ("helper.py:222-237", "helper.py:250-264", "zelda_prob.py:91-110", "Still 15: + pcgrl_get_paths_legs / pcgrl_get_paths_bytes / pcgrl_get_paths"):
        assert cited in hdr, cited
    L = _lib.load()
    for name in ("pcgrl_get_paths_legs", "pcgrl_get_paths_bytes", "pcgrl_get_paths"):
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert L.pcgrl_abi_version() == _lib.ABI_VERSION == 15
    assert L.pcgrl_get_paths_legs.argtypes == [C.POINTER(_lib.Config)] and L.pcgrl_get_paths_legs.restype == C.c_int32
    assert L.pcgrl_get_paths_bytes.argtypes == [C.POINTER(_lib.Config), C.c_int32, C.c_int32] and L.pcgrl_get_paths_bytes.restype == C.c_size_t
    assert L.pcgrl_get_paths.argtypes == [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    # refused without a handle, not crashed
    assert L.pcgrl_get_paths(None, None, 1, 1, None, None, None, None, 0, None) == _lib.PCGRL_ESTATE


def test_legs_and_workspace_sizes():
    from gym_pcgrl_amd import _lib
    L = _lib.load()
    want_legs = {"binary": 1, "zelda": 3, "sokoban": 0, "mdungeon": 0, "ddave": 0, "smb": 0}
    for prob, legs in want_legs.items():
        cfg = _config(prob, 5, 5) if prob != "smb" else _config(prob, 8, 20)
        assert int(L.pcgrl_get_paths_legs(C.byref(cfg))) == legs, prob
        n = int(L.pcgrl_get_paths_bytes(C.byref(cfg), 64, 16))
        assert (n >= 256) if legs else (n == 0), (prob, n)
    assert int(L.pcgrl_get_paths_legs(None)) == 0 and int(L.pcgrl_get_paths_bytes(None, 4, 4)) == 0
    for prob in ("binary", "zelda"):
        cfg = _config(prob, 64, 64)
        assert int(L.pcgrl_get_stats_bytes(C.byref(cfg), 10)) > 0
        for count in (1, 63, 64, 65, 4096, 1 << 20):
            for max_len in (1, 2, 4096, 100000):
                assert int(L.pcgrl_get_paths_bytes(C.byref(cfg), count, max_len)) >= 256
        assert int(L.pcgrl_get_paths_bytes(C.byref(cfg), 0, 16)) == 0 and int(L.pcgrl_get_paths_bytes(C.byref(cfg), -1, 16)) == 0
        assert int(L.pcgrl_get_paths_bytes(C.byref(cfg), 16, 0)) == 0 and int(L.pcgrl_get_paths_bytes(C.byref(cfg), 16, -1)) == 0
        for h, w in ((65, 64), (64, 65)):                                    # beyond the row-bitboard kernels
            big = _config(prob, h, w)
            assert int(L.pcgrl_get_stats_bytes(C.byref(big), 10)) == 0 and int(L.pcgrl_get_paths_bytes(C.byref(big), 10, 16)) == 0
            assert int(L.pcgrl_get_paths_legs(C.byref(big))) == want_legs[prob]
