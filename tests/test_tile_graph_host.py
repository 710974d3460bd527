"""helper.py for any tile set, without a GPU: the templates of gym_pcgrl_amd/csrc/tile_graph.h on the CPU lane-group simulator
(tests/hostsim/sim_tile_graph.cpp) against what the unmodified reference gives under the set rule (tests/golden/helper.npz), the host
side of pcgrl_tile_graph_bytes / pcgrl_tile_graph, the argument normalisation of gym_pcgrl_amd/helper.py and its get_range_reward."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from host_kit import config as _config, forms, header, plain_header, prototype, run_sanitized, struct_fields
from hostsim_build import build_so
from oracle_lib import _p

HERE = os.path.dirname(os.path.abspath(__file__))
G = os.path.join(HERE, "golden")
COLS = ("passable", "source_tiles", "reach_tiles", "sources", "regions", "longest", "reach", "source")      # levels_<g>


@pytest.fixture(scope="module")
def sim():
    L = build_so("sim_tile_graph.cpp")
    L.sim_tile_graph.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int] + [C.c_void_p] * 7
    return L


@pytest.fixture(scope="module")
def fix():
    return np.load(os.path.join(G, "helper.npz"))


def _run(L, m, group, bits, passable, source_tiles, reach_tiles, source):
    m = np.ascontiguousarray(m, np.uint8)
    h, w = m.shape
    lab, dist = np.full(h * w + 2, 77, np.int16), np.full(h * w + 2, 77, np.int16)      # a guard word at either end
    out, status = np.full(4, -9, np.int32), np.zeros(1, np.int32)
    rc = L.sim_tile_graph(_p(m), h, w, group, bits, int(passable), int(source_tiles), int(reach_tiles), int(source), _p(out[0:]), _p(out[1:]),
                          _p(lab[1:]), _p(dist[1:]), _p(out[2:]), _p(out[3:]), _p(status))
    assert rc == 0 and lab[0] == lab[-1] == dist[0] == dist[-1] == 77
    return out, lab[1:-1].reshape(h, w), dist[1:-1].reshape(h, w), int(status[0])


def test_every_fixture_level_on_every_form(sim, fix):
    """All six outputs of every level, with 16 and 64 lanes and both mask widths where the map fits."""
    seen, n = set(), 0
    for name in fix["groups"].tolist():
        maps, lv = fix["maps_" + name], fix["levels_" + name]
        h, w = maps.shape[1:]
        for group, bits in forms(h, w):
            for i, m in enumerate(maps):
                out, lab, dist, status = _run(sim, m, group, bits, *lv[i, :4])
                assert out.tolist() == lv[i, 4:].tolist(), (name, i, group, bits, out, lv[i])
                assert np.array_equal(lab, fix["labels_" + name][i]), (name, i, group, bits)
                assert np.array_equal(dist, fix["dist_" + name][i]), (name, i, group, bits)
                assert status == 0
                n += 1
            seen.add((group, bits))
    assert seen == {(16, 32), (16, 64), (64, 32), (64, 64)} and n > 600


def test_fixture_is_consistent_and_covers_what_the_issue_lists(fix):
    names = fix["groups"].tolist()
    shapes = set()
    for name in names:
        maps, lv, lab, dist = fix["maps_" + name], fix["levels_" + name], fix["labels_" + name], fix["dist_" + name]
        assert lv.shape == (len(maps), len(COLS)) and lab.dtype == dist.dtype == np.int16 and lab.shape == dist.shape == maps.shape
        shapes.add(maps.shape[1:])
        for i, m in enumerate(maps):
            p = ((int(lv[i, 0]) >> np.minimum(m, 31).astype(np.int64)) & 1).astype(bool)
            assert np.array_equal(lab[i] > 0, p) and (lab[i][~p] == -1).all() and lab[i].max() == (int(lv[i, 4]) if p.any() else -1)
            assert (dist[i][~p] == -1).all()
            src = int(lv[i, 7])
            assert ((dist[i] == 0).sum() == 1 and dist[i].flat[src] == 0) if (src >= 0 and p.flat[src]) else (dist[i] == -1).all()
            r = ((int(lv[i, 2]) >> np.minimum(m, 31).astype(np.int64)) & 1).astype(bool)
            assert int(((dist[i] >= 0) & r).sum()) == lv[i, 6]
    assert shapes >= {(1, 1), (1, 9), (8, 1), (5, 5), (16, 32), (16, 33), (17, 32), (17, 9), (14, 14), (9, 64), (64, 64)}
    tiles = {len(np.unique(m)) for name in names if name.startswith("rand_") for m in fix["maps_" + name]}
    assert {2, 3, 5, 8} <= tiles
    big, lvb = fix["maps_hand_64x64"], fix["levels_hand_64x64"]
    assert (big[0] == 0).all() and lvb[0, 4:6].tolist() == [1, 126]                      # all open
    assert (big[1] == 1).all() and lvb[1, 4:].tolist() == [0, 0, 0, -1]                  # all blocked
    assert lvb[2, 4] == 2048 and fix["labels_hand_64x64"][2].max() == 2048               # the checkerboard
    assert lvb[3, 4] == 1 and fix["dist_hand_64x64"][3].max() > 2000                     # the spiral
    assert big[4].max() == 31 and (lvb[4, 0] >> 30) & 1                                  # tiles 30 and 31 in use
    small, lvs = fix["maps_hand_7x9"], fix["levels_hand_7x9"]
    assert lvs[1, 3] == 9 and small[1].flat[9] == 1 and lvs[1, 7] == 9 and (fix["dist_hand_7x9"][1] == -1).all()      # a source on an impassable cell
    assert lvs[2, 3] == -1 and lvs[2, 7] == -1                                           # source -1
    assert lvs[3, 3] == -2 and lvs[3, 7] == -1                                           # no cell of source_tiles
    assert (small[4] == 2).sum() == 2 and lvs[4, 7] == int(np.flatnonzero(small[4] == 2)[0])     # two of them: the first is taken
    assert small[6].max() == 31 and lvs[6, 0] == (3 << 30)
    assert fix["order_dependent"].shape == (len(names),)
    assert os.path.getsize(os.path.join(G, "helper.npz")) <= os.path.getsize(os.path.join(G, "paths.npz"))


def test_status_bits_and_optional_outputs_on_the_simulator(sim):
    m = np.zeros((3, 7), np.uint8)
    m[1, 2] = 32
    m[2, 3] = 255
    out, lab, dist, status = _run(sim, m, 16, 32, 1, 1, 1, -2)
    assert status == 4 and lab[1, 2] == lab[2, 3] == -1 and (out[0], out[2], out[3]) == (1, 19, 0)     # a byte >= 32 is in no set
    out, lab, dist, status = _run(sim, np.zeros((3, 7), np.uint8), 16, 32, 1, 1, 1, 21)
    assert status == 2 and out[3] == -1 and (dist == -1).all() and out[2] == 0                   # a cell outside the map: none
    out, _, _, status = _run(sim, np.zeros((3, 7), np.uint8), 16, 32, 1, 1, 1, -7)
    assert status == 2 and out[3] == -1
    # only the scalars: no map is written
    one = np.full(1, -9, np.int32)
    st = np.zeros(1, np.int32)
    assert sim.sim_tile_graph(_p(np.zeros((3, 7), np.uint8)), 3, 7, 64, 64, 1, 0, 0, -2, _p(one), None, None, None, None, None, _p(st)) == 0 and one[0] == 1


def test_sanitized_stand_alone_program():
    """sim_tile_graph.cpp with its own main(), built with the address and undefined-behaviour sanitizers and run as a program: built-in
    levels on every (lane group, mask width) form, with guard words around the maps."""
    run_sanitized("sim_tile_graph.cpp", "SIM_TILE_GRAPH_MAIN", 300)


# ------------------------------------------------------------------ the ABI, without a device
def test_declared_exported_and_mirrored():
    from gym_pcgrl_amd import _lib
    hdr, plain = header(), plain_header()
    assert re.search(prototype("size_t", "pcgrl_tile_graph_bytes", ["const pcgrl_config*", "int32_t"]), plain)
    assert re.search(prototype("int", "pcgrl_tile_graph", ["pcgrl_env*", "const pcgrl_tile_graph_desc*", "void*", "size_t", "void*"]), plain)
    for cited in ("helper.py:170-296", "Still 15: + pcgrl_tile_graph_desc / pcgrl_tile_graph_bytes / pcgrl_tile_graph", "renamed to one single value"):
        assert cited in hdr, cited
    # the struct mirror: field order, types and size against the header
    ptr = C.c_void_p
    fields = struct_fields("pcgrl_tile_graph_desc", {"const uint8_t*": ptr, "const int32_t*": ptr, "int32_t*": ptr, "int16_t*": ptr, "int32_t": C.c_int32, "uint32_t": C.c_uint32})
    assert fields == list(_lib.TileGraphDesc._fields_)
    assert [n for n, _ in fields] == ["maps", "count", "passable", "source_tiles", "reach_tiles", "sources", "regions_out", "longest_out",
                                      "labels_out", "dist_out", "reach_out", "source_out"]
    assert C.sizeof(_lib.TileGraphDesc) == 80 and _lib.TileGraphDesc.sources.offset == 24 and _lib.TileGraphDesc.source_out.offset == 72
    L = _lib.load()
    for name in ("pcgrl_tile_graph_bytes", "pcgrl_tile_graph"):
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert L.pcgrl_abi_version() == _lib.ABI_VERSION == 15
    assert L.pcgrl_tile_graph_bytes.argtypes == [C.POINTER(_lib.Config), C.c_int32] and L.pcgrl_tile_graph_bytes.restype == C.c_size_t
    assert L.pcgrl_tile_graph.argtypes == [C.c_void_p, C.POINTER(_lib.TileGraphDesc), C.c_void_p, C.c_size_t, C.c_void_p]
    # refused without a handle, not crashed
    assert L.pcgrl_tile_graph(None, None, None, 0, None) == _lib.PCGRL_ESTATE
    assert L.pcgrl_tile_graph(None, C.byref(_lib.TileGraphDesc()), None, 0, None) == _lib.PCGRL_ESTATE


def test_workspace_sizes():
    from gym_pcgrl_amd import _lib
    L = _lib.load()
    for prob in ("binary", "zelda", "sokoban", "mdungeon", "ddave"):             # whatever problem the handle has
        for h, w in ((1, 1), (5, 5), (16, 33), (64, 64)):
            if prob in ("sokoban", "mdungeon", "ddave") and (h, w) == (1, 1):
                continue
            cfg = _config(prob, h, w)
            for count in (1, 63, 64, 65, 1 << 20):
                assert int(L.pcgrl_tile_graph_bytes(C.byref(cfg), count)) >= 256, (prob, h, w, count)
            assert int(L.pcgrl_tile_graph_bytes(C.byref(cfg), 0)) == 0 and int(L.pcgrl_tile_graph_bytes(C.byref(cfg), -1)) == 0
    for h, w in ((65, 64), (64, 65)):                                            # beyond the row-bitboard kernels
        assert int(L.pcgrl_tile_graph_bytes(C.byref(_config("binary", h, w)), 10)) == 0
    assert int(L.pcgrl_tile_graph_bytes(C.byref(_config("smb", 8, 20)), 10)) == 0
    assert int(L.pcgrl_tile_graph_bytes(None, 4)) == 0


# ------------------------------------------------------------------ gym_pcgrl_amd/helper.py on the host
def test_argument_normalisation():
    import gym_pcgrl_amd
    from gym_pcgrl_amd import helper
    assert gym_pcgrl_amd.helper is helper
    names = ["empty", "solid", "player", "key"]
    assert helper.tile_set(0) == 1 and helper.tile_set([0, 2]) == 5 and helper.tile_set((31,)) == 1 << 31 and helper.tile_set(None) == 0
    assert helper.tile_set("empty", names) == 1 and helper.tile_set(["empty", "key", 1], names) == 0b1011 and helper.tile_set({2, 2}) == 4
    assert helper.tile_set(np.int64(3)) == 8 and helper.tile_set(np.array([1, 3])) == 10 and helper.tile_set([]) == 0
    for bad in (32, -1, [0, 40], "lava", ["empty", "lava"], 1.5, [True]):
        with pytest.raises(ValueError):
            helper.tile_set(bad, names)
    with pytest.raises(ValueError):
        helper.tile_set("empty")                                                         # a name without the problem's names
    assert helper.source_arg(None, 7, 3) == ("none", None)
    assert helper.source_arg(10, 7, 3) == ("cells", 10) and helper.source_arg(-1, 7, 3) == ("cells", -1)
    assert helper.source_arg((6, 2), 7, 3) == ("cells", 20) and helper.source_arg((np.int32(1), 1), 7, 3) == ("cells", 8)
    assert helper.source_arg("player", 7, 3, names) == ("tiles", 4) and helper.source_arg([2, "key"], 7, 3, names) == ("tiles", 12)
    kind, cells = helper.source_arg((np.array([1, 2]), np.array([0, 2])), 7, 3)
    assert kind == "cells" and cells.tolist() == [1, 16]
    kind, cells = helper.source_arg(np.array([5, -1]), 7, 3)
    assert kind == "cells" and cells.tolist() == [5, -1]
    for bad in (21, -2, (7, 0), (0, 3), (1, 2, 3), 1.5):
        with pytest.raises(ValueError):
            helper.source_arg(bad, 7, 3, names)
    # calc_certain_tile needs no kernel
    m = np.array([[[0, 1, 2], [2, 31, 40]]], np.uint8)
    assert helper.calc_certain_tile(m, [2]).tolist() == [2] and helper.calc_certain_tile(m, [0, 31]).tolist() == [2]
    import torch
    assert helper.calc_certain_tile(torch.as_tensor(m), [1, 2, 31]).tolist() == [4]


def test_get_range_reward_on_tensors():
    import torch
    from gym_pcgrl_amd import helper
    tab = np.load(os.path.join(G, "range_reward.npz"))["table"]                          # (low, high, new, old, reward), +-inf bounds
    lo, hi, nv, ov, r = (torch.as_tensor(tab[:, k]) for k in range(5))
    got = helper.get_range_reward(nv, ov, lo, hi)
    assert got.dtype == torch.int64 and torch.equal(got.to(torch.float64), r) and len(tab) > 1000
    # scalars and broadcasting
    assert helper.get_range_reward(3, 1, 2, float("inf")).item() == 1 and helper.get_range_reward(torch.tensor([0, 5, 9]), 5, 4, 6).tolist() == [-4, 0, -3]
