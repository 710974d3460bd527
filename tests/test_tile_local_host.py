"""The local half of helper.py for any tile set, without a GPU: gym_pcgrl_amd/csrc/tile_local.h on the CPU (tests/hostsim/
sim_tile_local.cpp) in every form the kernel has against what the unmodified reference gives (tests/golden/helper_local.npz), the
fixture against the definitions, the host side of pcgrl_tile_local_bytes / pcgrl_tile_local and the argument normalisation of
gym_pcgrl_amd/helper.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from host_kit import config as _config, header, plain_header, prototype, run_sanitized, struct_fields
from hostsim_build import build_so
from oracle_lib import _p

HERE = os.path.dirname(os.path.abspath(__file__))
G = os.path.join(HERE, "golden")
FORMS = ((16, 1), (64, 1), (64, 0))          # (lanes, staged): kernels_tile_local.h
GUARD = 8


def load_fixture():
    """helper_local.npz as a list of levels: dicts of name (the group), map [h, w], the query, the four scalars, floor_map, group_map."""
    fix = np.load(os.path.join(G, "helper_local.npz"))
    names, out, at = fix["groups"].tolist(), [], 0
    for i, row in enumerate(fix["levels"]):
        g, h, w, frm, floor, group, lo, hi, noff, fd, gr, ch, cv = (int(v) for v in row)
        n = h * w
        out.append(dict(name=names[g], map=fix["maps"][at:at + n].reshape(h, w), from_tiles=frm, floor_tiles=floor, group_tiles=group, group_min=lo,
                        group_max=hi, offsets=fix["offsets"][i, :noff], floor_dist=fd, grouping=gr, changes=(ch, cv),
                        floor_map=fix["floor_map"][at:at + n].reshape(h, w), group_map=fix["group_map"][at:at + n].reshape(h, w)))
        at += n
    assert at == len(fix["maps"]) == len(fix["floor_map"]) == len(fix["group_map"])
    return out, names


def in_set(mask, m):
    return (((int(mask) >> np.minimum(m, 31).astype(np.int64)) & 1) == 1) & (m < 32)


def counts_of(m):
    return np.bincount(m.reshape(-1), minlength=256)[:32].astype(np.int32)


@pytest.fixture(scope="module")
def sim():
    from gym_pcgrl_amd import _lib
    L = build_so("sim_tile_local.cpp")
    L.sim_tile_local.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_lib.TileLocalDesc), C.c_void_p]
    return L


@pytest.fixture(scope="module")
def levels():
    return load_fixture()


def _run(L, lv, lanes, staged, pick=None, m=None):
    """One level on one form, every output (pick: only those named) between guard elements -> (dict of outputs, status)."""
    from gym_pcgrl_amd import _lib
    m = np.ascontiguousarray(lv["map"] if m is None else m, np.uint8)
    h, w = m.shape
    fields = dict(counts=(np.int32, 32), floor_dist=(np.int32, 1), floor_map=(np.int16, h * w), grouping=(np.int32, 1), group_map=(np.int8, h * w),
                  changes=(np.int32, 2))
    bufs = {f: np.full(n + 2 * GUARD, 77, dt) for f, (dt, n) in fields.items()}
    d = _lib.TileLocalDesc(None, 1, lv["from_tiles"], lv["floor_tiles"], lv["group_tiles"], lv["group_min"], lv["group_max"], len(lv["offsets"]))
    for k, (dx, dy) in enumerate(lv["offsets"]):
        d.offsets[k][0], d.offsets[k][1] = int(dx), int(dy)
    for f in fields:
        if pick is None or f in pick:
            setattr(d, f + "_out", bufs[f][GUARD:].ctypes.data)
    status = np.zeros(1, np.int32)
    assert L.sim_tile_local(_p(m), h, w, lanes, staged, C.byref(d), _p(status)) == 0
    out = {}
    for f, b in bufs.items():
        assert (b[:GUARD] == 77).all() and (b[-GUARD:] == 77).all(), f
        if pick is None or f in pick:
            out[f] = b[GUARD:-GUARD]
        else:
            assert (b == 77).all(), f                                        # not asked for: untouched
    return out, int(status[0])


def _check(out, lv, what):
    h, w = lv["map"].shape
    assert out["floor_dist"][0] == lv["floor_dist"] and out["grouping"][0] == lv["grouping"] and tuple(out["changes"]) == lv["changes"], what
    assert np.array_equal(out["floor_map"].reshape(h, w), lv["floor_map"]), what
    assert np.array_equal(out["group_map"].reshape(h, w), lv["group_map"]), what
    assert np.array_equal(out["counts"], counts_of(lv["map"])), what


def test_every_fixture_level_on_every_form(sim, levels):
    """All six outputs of every level: sixteen lanes and a wavefront on a stage where the map fits one, a wavefront on the caller's bytes."""
    seen, n = set(), 0
    for i, lv in enumerate(levels[0]):
        h, w = lv["map"].shape
        for lanes, staged in FORMS:
            if staged and (h > 64 or w > 64):
                continue
            out, status = _run(sim, lv, lanes, staged)
            _check(out, lv, (lv["name"], i, lanes, staged))
            assert status == 0
            seen.add((lanes, staged))
            n += 1
    assert seen == set(FORMS) and n > 400


def test_fixture_is_consistent_and_covers_what_the_issue_lists(levels):
    lvs, names = levels
    shapes, by_group = set(), {}
    for lv in lvs:
        m, fm, gm = lv["map"], lv["floor_map"], lv["group_map"]
        h, w = m.shape
        shapes.add((h, w))
        by_group.setdefault(lv["name"], []).append(lv)
        # the scalars are what their definition says over the per-cell maps
        assert lv["floor_dist"] == int(fm[in_set(lv["from_tiles"], m)].sum())
        own = in_set(lv["group_tiles"], m)
        assert lv["grouping"] == int((own & (gm >= lv["group_min"]) & (gm <= lv["group_max"])).sum())
        assert lv["changes"] == (int((m[:, 1:] != m[:, :-1]).sum()), int((m[1:] != m[:-1]).sum()))
        assert fm.min() >= -1 and fm.max() <= h - 1 and gm.min() >= 0 and gm.max() <= len(lv["offsets"])
        assert np.array_equal(fm == -1, in_set(lv["floor_tiles"], m))
    assert shapes >= {(1, 1), (1, 9), (8, 1), (5, 5), (14, 14), (17, 9), (3, 7), (16, 32), (16, 33), (17, 32), (9, 64), (64, 64), (9, 16), (9, 17),
                      (65, 2), (2, 65), (65, 64), (64, 65), (14, 114), (3, 255), (6, 8)}
    for name, group in by_group.items():
        h, w = group[0]["map"].shape
        if h < 2:
            continue
        # the three floor cases: a floor cell, a floor found below, no floor at or below
        below = any(((lv["floor_map"] >= 0) & ~_no_floor_below(lv)).any() for lv in group)
        assert any((lv["floor_map"] == -1).any() for lv in group) and below and any(_no_floor_below(lv).any() for lv in group), name
    tiles = {len(np.unique(lv["map"])) for lv in lvs if lv["name"].startswith("rand_")}
    assert {2, 3, 5, 8} <= tiles
    queries = {(lv["from_tiles"], lv["floor_tiles"], lv["group_tiles"], lv["group_min"], lv["group_max"], len(lv["offsets"])) for lv in lvs if lv["name"].startswith("rand_")}
    assert queries == {(4, 0x5A, 0x40, 1, 1, 2), (3, 2, 1, 2, 5, 8), (255, 0, 6, 0, 0, 6), (0, 255, 0, 0, 0, 0), (1, 1, 1, 3, 1, 4)}
    assert any(lv["floor_dist"] < 0 for lv in lvs) and any(lv["group_min"] > lv["group_max"] and lv["grouping"] == 0 and (lv["group_map"] > 0).any() for lv in lvs)
    hand = by_group["hand_6x8"]
    a, b, c, d, e, e2 = hand
    assert a["map"][5, 1] == 2 and a["floor_map"][5, 1] == 5 and a["floor_map"][2, 3] == 0 and a["floor_map"][0, 5] == 3 and a["floor_dist"] == 8
    assert b["floor_dist"] == -2 and (b["floor_map"][[1, 4], 2] == -1).all()                 # a from tile that is a floor tile
    assert (c["map"] != 1).sum() == 47 and (c["floor_map"][:, :6] == 5).all() and c["floor_map"][:, 6].tolist() == [2, 1, 0, -1, 5, 5]
    assert set(np.unique(d["map"])) == {29, 30, 31} and d["from_tiles"] == (1 << 30) | (1 << 29) and d["grouping"] > 0
    assert len(e["offsets"]) == 16 and e["group_map"][0, 0] == 4 and e["group_map"][5, 7] == 4 and e["group_map"][0, 7] == 5 and e["group_map"][5, 0] == 5
    assert e2["group_map"][0, 0] == e2["group_map"][0, 7] == e2["group_map"][5, 0] == e2["group_map"][5, 7] == 2 and e2["group_map"][0, 2] == 3
    assert os.path.getsize(os.path.join(G, "helper_local.npz")) <= os.path.getsize(os.path.join(G, "helper.npz"))


def _no_floor_below(lv):
    """The cells without a floor tile at or below (their floor_map is H - 1 whatever the row)."""
    f = in_set(lv["floor_tiles"], lv["map"])
    return ~(np.cumsum(f[::-1], 0)[::-1] > 0)


def test_status_bit_and_optional_outputs_on_the_simulator(sim, levels):
    lv = next(l for l in levels[0] if l["name"] == "rand_5x5" and l["from_tiles"] == 3)
    clean = lv["map"].copy()
    clean[1, 2] = clean[4, 4] = 31
    bad = clean.copy()
    bad[1, 2], bad[4, 4] = 32, 255
    for lanes, staged in FORMS:
        ref, status = _run(sim, lv, lanes, staged, m=clean)
        assert status == 0
        got, status = _run(sim, lv, lanes, staged, m=bad)
        assert status == 4                                                   # a byte >= 32 is in no set and in no counts column
        for f in ("floor_dist", "floor_map", "grouping", "group_map"):
            assert np.array_equal(got[f], ref[f]), f
        assert got["counts"][31] == 0 and ref["counts"][31] == 2 and np.array_equal(got["counts"][:31], ref["counts"][:31])
        assert tuple(got["changes"]) == (int((bad[:, 1:] != bad[:, :-1]).sum()), int((bad[1:] != bad[:-1]).sum()))      # the raw bytes
        for f in ("counts", "floor_dist", "floor_map", "grouping", "group_map", "changes"):      # each output alone, the others untouched
            one, status = _run(sim, lv, lanes, staged, pick=(f,), m=bad)
            assert np.array_equal(one[f], got[f]) and status == 4, f


def test_sanitized_stand_alone_program():
    """sim_tile_local.cpp with its own main(), built with the address and undefined-behaviour sanitizers and run as a program: built-in
    levels up to 255 x 255 on every form against a plain restatement of the rules, each output alone and all together between guards."""
    run_sanitized("sim_tile_local.cpp", "SIM_TILE_LOCAL_MAIN", 300)


# ------------------------------------------------------------------ the ABI, without a device
def test_declared_exported_and_mirrored(sim):
    from gym_pcgrl_amd import _lib
    hdr, plain = header(), plain_header()
    assert re.search(prototype("size_t", "pcgrl_tile_local_bytes", ["const pcgrl_config*", "int32_t"]), plain)
    assert re.search(prototype("int", "pcgrl_tile_local", ["pcgrl_env*", "const pcgrl_tile_local_desc*", "void*", "size_t", "void*"]), plain)
    for cited in ("helper.py:37-137", "Still 15: + pcgrl_tile_local_desc / pcgrl_tile_local_bytes / pcgrl_tile_local"):
        assert cited in hdr, cited
    assert re.search(r"#define\s+PCGRL_MAX_OFFSETS\s+16\b", plain) and _lib.MAX_OFFSETS == 16
    ptr = C.c_void_p
    fields = struct_fields("pcgrl_tile_local_desc", {"const uint8_t*": ptr, "int32_t*": ptr, "int16_t*": ptr, "int8_t*": ptr, "int32_t": C.c_int32,
                                                     "uint32_t": C.c_uint32, "int8_t": (C.c_int8 * 2) * 16})
    fields = [(n.split("[")[0], t) for n, t in fields]
    assert fields == list(_lib.TileLocalDesc._fields_)
    assert [n for n, _ in fields] == ["maps", "count", "from_tiles", "floor_tiles", "group_tiles", "group_min", "group_max", "noffsets", "offsets",
                                      "counts_out", "floor_dist_out", "floor_map_out", "grouping_out", "group_map_out", "changes_out"]
    D = _lib.TileLocalDesc
    assert C.sizeof(D) == 120 == sim.sim_tile_local_desc_bytes() and D.offsets.offset == 36 and D.counts_out.offset == 72 and D.changes_out.offset == 112
    L = _lib.load()
    for name in ("pcgrl_tile_local_bytes", "pcgrl_tile_local"):
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert L.pcgrl_abi_version() == _lib.ABI_VERSION == 15
    assert L.pcgrl_tile_local_bytes.argtypes == [C.POINTER(_lib.Config), C.c_int32] and L.pcgrl_tile_local_bytes.restype == C.c_size_t
    assert L.pcgrl_tile_local.argtypes == [C.c_void_p, C.POINTER(_lib.TileLocalDesc), C.c_void_p, C.c_size_t, C.c_void_p]
    # refused without a handle, not crashed
    assert L.pcgrl_tile_local(None, None, None, 0, None) == _lib.PCGRL_ESTATE
    assert L.pcgrl_tile_local(None, C.byref(_lib.TileLocalDesc()), None, 0, None) == _lib.PCGRL_ESTATE


def test_workspace_sizes():
    from gym_pcgrl_amd import _lib
    L = _lib.load()
    cfgs = [(prob, h, w) for prob in ("binary", "zelda", "sokoban", "mdungeon", "ddave", "smb") for h, w in ((5, 5), (64, 64), (65, 64), (64, 65))]
    for prob, h, w in cfgs + [("smb", 14, 114), ("binary", 40, 300)]:
        cfg = _config(prob, h, w)
        for count in (1, 63, 64, 65, 1 << 20):
            assert int(L.pcgrl_tile_local_bytes(C.byref(cfg), count)) >= 256, (prob, h, w, count)
        assert int(L.pcgrl_tile_local_bytes(C.byref(cfg), 0)) == 0 and int(L.pcgrl_tile_local_bytes(C.byref(cfg), -1)) == 0
    assert int(L.pcgrl_tile_local_bytes(None, 4)) == 0
    bad = _config("binary", 5, 5)
    bad.width = 0
    assert int(L.pcgrl_tile_local_bytes(C.byref(bad), 4)) == 0                 # an invalid configuration


# ------------------------------------------------------------------ gym_pcgrl_amd/helper.py on the host
def test_argument_normalisation():
    from gym_pcgrl_amd import helper
    from gym_pcgrl_amd.envs import BatchedPcgrlEnv
    assert helper.offsets_arg([]) == [] and helper.offsets_arg(()) == []
    assert helper.offsets_arg([(-1, 0), (1, 0)]) == [(-1, 0), (1, 0)] and helper.offsets_arg(np.array([[0, -128], [127, 5]])) == [(0, -128), (127, 5)]
    assert helper.offsets_arg([[2, 0], (2, 0)]) == [(2, 0), (2, 0)]            # listed twice: kept twice
    assert len(helper.offsets_arg([(0, 1)] * 16)) == 16
    for bad in ([(0, 1)] * 17, [(128, 0)], [(0, -129)], [(1, 2, 3)], [(1,)], [1, 2], 5, [(0.5, 1)], [(True, 0)]):
        with pytest.raises(ValueError):
            helper.offsets_arg(bad)
    assert helper._listed(None) == [] and helper._listed([2]) == [2] and helper.tile_set([]) == 0
    for f in ("get_floor_dist", "get_type_grouping", "get_changes", "floor_dist_map", "group_value_map", "count_tiles"):
        assert callable(getattr(helper, f)), f
    assert "get_tile_locations" in helper.__doc__ and "in types" in helper.__doc__ and not hasattr(helper, "get_tile_locations")
    with pytest.raises(ValueError):
        helper.get_changes(np.zeros((5, 5), np.uint8))                         # not a stack
    # tile_stats() refuses on the host what it can: no handle is made for these
    env = BatchedPcgrlEnv(prob="smb", rep="wide", num_envs=1, seed=0)
    m = np.zeros((1, 14, 114), np.uint8)
    for kw in (dict(), dict(floor_from=["enemy"]), dict(floor_map=True), dict(group_map=True), dict(group=["tube"], offsets=[(0, 1)] * 17),
               dict(group=["tube"], offsets=[(200, 0)]), dict(group=["tube"], offsets=[(1, 2, 3)]), dict(floor=["lava"], floor_map=True),
               dict(floor=["solid"])):
        with pytest.raises(ValueError):
            env.tile_stats(m, **kw)
    assert env._handle is None
    env.close()
