"""The wrapped observation without a GPU: the routines of gym_pcgrl_amd/csrc/kernels_obs.h compiled for the CPU
(tests/hostsim/sim_obs.cpp) against the rule of the wrappers (tests/obs_cases.py expected_image, itself held against the np.pad form of
tests/test_gpu_parity.py) on every case of the table and every cursor cell of the map; the Python restatement of the route rule pinned
against the C obs_lean_mode; the in-place update of the wide representation for every one-cell change; the sanitized stand-alone
program."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import obs_cases as oc
from host_kit import ROOT, run_sanitized
from hostsim_build import build_so
from oracle_lib import _p

FORM_BLOCK, FORM_BLOCK_LEAN, FORM_ENV_LEAN = 0, 1, 2


@pytest.fixture(scope="module")
def sim():
    L = build_so("sim_obs.cpp")
    L.sim_obs.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 13 + [C.c_void_p] * 4
    L.sim_obs_delta.argtypes = [C.c_void_p] + [C.c_int] * 7 + [C.c_void_p] * 2
    L.sim_obs_lean_grid.argtypes = [C.c_int] * 4 + [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.sim_obs_lean_grid.restype = None
    return L


def _aligned(nbytes, fill=0xA5):
    """`nbytes` bytes, 16-byte aligned, between two guards of 64 bytes, all `fill`: (whole buffer, the target inside it)."""
    raw = np.full(nbytes + 64 + 64 + 16, fill, np.uint8)
    off = 64 + (-(raw.ctypes.data + 64)) % 16
    return raw, raw[off:off + nbytes], off


def _source(c):
    """k_obs's source of a case (launch_obs): 0 byte map, 1 / 2 one plane of 32 / 64 bits, 3 three planes of 32 bits."""
    nplanes = oc.prob_planes(c.prob, c.W, c.H)[1]
    depth = oc.depth_of(c)
    if nplanes == 1 and depth == 1:
        return 1 if c.W <= 32 else 2
    if nplanes == 3 and c.W <= 32 and depth == 8:
        return 3
    return 0


def _run(L, m, pos, c, source, form, epb=64, nthreads=256, act=None, changed=None, fresh=None):
    n, H, W = m.shape
    depth = oc.depth_of(c)
    per_env = c.oh * c.ow * depth
    raw, tgt, off = _aligned(n * per_env)
    keep = [np.ascontiguousarray(a) if a is not None else None for a in (act, changed, fresh)]
    rc = L.sim_obs(_p(m), _p(pos), n, H, W, source, 16 if H <= 16 else 64, c.oh, c.ow, depth, c.centered, c.pad, form, epb, nthreads,
                   *[(_p(a) if a is not None else None) for a in keep], C.c_void_p(tgt.ctypes.data))
    assert (raw[:off] == 0xA5).all() and (raw[off + n * per_env:] == 0xA5).all(), "a store outside the target"
    return rc, tgt.reshape(n, c.oh, c.ow, depth)


def _inputs(c, seed=11):
    """Environment i on cell i of its own random map; ten more on the corners and the middle of all-0 and all-max-tile maps.  (A window
    from the origin does not look at the cursor: a sample of the environments is enough.)  Huge windows: three environments."""
    n = c.H * c.W if c.centered else min(c.H * c.W, 70)
    pos = oc.every_cursor(c.H, c.W)
    pos = np.concatenate([pos[:n], pos[c.H * c.W:]])
    m = oc.seeded_maps(n, c.H, c.W, oc.NTILES[c.prob], seed + c.H * 64 + c.W)
    if c.route == "huge":
        m, pos = m[[0, n, n + 5]], pos[[c.H * c.W - 1 if c.centered else 0, n, n + 9]]
    return m, np.ascontiguousarray(pos)


def test_expected_image_is_the_np_pad_form():
    """obs_cases.expected_image (index grids, every environment at once) gives what _expected_image of tests/test_gpu_parity.py gives
    (np.pad, environment by environment) on every case of the table: for the corners, the middle and a stride of the other cursors."""
    from test_gpu_parity import _expected_image
    checked = 0
    for c in oc.CASES:
        m, pos = _inputs(c)
        n = len(m)
        pick = np.unique(np.concatenate([np.arange(0, n, max(1, n // 7)), np.arange(max(0, n - 10), n), [0, min(n, c.W) - 1]]))
        depth = oc.depth_of(c)
        fast = oc.expected_image(m, pos, c.oh, c.ow, c.centered, c.pad, depth)
        assert fast.shape == (n, c.oh, c.ow, depth) and fast.dtype == np.uint8
        slow = _expected_image(m[pick], pos[pick], c.oh, c.ow, c.centered, c.pad, depth)
        assert np.array_equal(fast[pick], slow), oc.case_id(c)
        checked += len(pick)
    assert checked > 5000


def test_case_table_names_every_route_and_what_the_issue_lists():
    routes = {c.route for c in oc.CASES}
    assert routes == set(oc.ROUTES), sorted(set(oc.ROUTES) - routes)
    assert len({oc.case_id(c) for c in oc.CASES}) == len(oc.CASES)
    by = lambda **kw: [c for c in oc.CASES if all(getattr(c, k) == v for k, v in kw.items())]
    # rows: every width on its word size, fused and k_obs heights, every window centred and from the origin with pad 0 and 1
    assert {c.W for c in by(family="rows")} == {5, 16, 31, 32, 33, 48, 63, 64} and {c.H for c in by(family="rows")} == {3, 16, 17, 64}
    for H, W in oc.ROWS_MAPS:
        got = {(c.oh, c.ow, c.centered, c.pad) for c in by(family="rows", H=H, W=W)}
        assert got == {(oh, ow, ce, p) for oh, ow in oc.ROWS_WINDOWS for ce in (0, 1) for p in (0, 1)}
        want = ("fused_rows32" if W <= 32 else "fused_rows64") if H <= 16 else ("k_obs1" if W <= 32 else "k_obs2")
        assert {c.route for c in by(family="rows", H=H, W=W)} == {want} and {c.routine for c in by(family="rows", H=H, W=W)} == {"rows"}
        assert {c.routine for c in by(family="rows_fall", H=H, W=W)} == {"general"} and len(by(family="rows_fall", H=H, W=W)) == 3
    assert max(c.oh * c.ow for c in by(family="rows")) == 4096
    # one-hot over eight tiles
    hot = by(family="hot8")
    assert {c.W for c in hot} == {3, 11, 32} and {(c.oh, c.ow) for c in hot} == set(oc.HOT8_WINDOWS) and {c.pad for c in hot} == set(oc.HOT8_PADS)
    assert {c.route for c in hot if c.prob == "zelda" and (c.oh, c.ow) != (7, 11)} == {"fused_hot8"}
    assert {c.route for c in hot if c.prob == "mdungeon"} == {"k_obs3"}
    assert {c.routine for c in hot if (c.oh, c.ow) == (7, 11)} == {"general"} and {c.routine for c in hot if (c.oh, c.ow) != (7, 11)} == {"hot8"}
    assert {c.oh * c.ow for c in hot} >= {4032, 4096}
    # the general routine, the two sides of the 65 536-byte limit, the in-place update
    gen = by(family="general")
    assert {(c.oh, c.ow) for c in gen} == set(oc.GENERAL_WINDOWS) and {c.prob for c in gen} >= {"sokoban", "smb"} and {c.onehot for c in gen} == {0, 1}
    # one environment per cell: a batch whose one block is partial and whose byte count is no multiple of 16
    assert any((c.H * c.W) % oc.OBS_EPB and (c.H * c.W * c.oh * c.ow * oc.depth_of(c)) % 16 for c in gen)
    assert [(c.oh * c.ow, c.route) for c in by(family="huge")] == [(65536, "huge"), (65535, "k_obs1")]
    assert {(c.oh, c.ow, c.route) for c in by(family="delta", stepping="incremental")} == {(7, 11, "k_obs3"), (8, 12, "fused_delta"), (6, 8, "fused_delta"),
                                                                                          (8, 9, "fused_delta"), (16, 11, "fused_delta")}
    assert {c.route for c in by(family="delta", stepping="step")} == {"k_obs3", "fused_hot8"}
    assert all(c.pad != 0xA5 for c in oc.CASES)


def test_device_plans_reach_what_they_are_for():
    """What tests/test_gpu_obs_windows.py runs, worked out here: pcgrl_observe on the table's map shapes reaches every stand-alone kernel;
    one environment per cell gives the fused kernel batches that fill the groups of four images of obs_write_envs_rows<4> (a multiple of
    4 x the 16 wavefronts of the largest block) and batches that do not (its e < ne tails); the tape of the narrow test makes the
    oracle's cursors -- the cursor sequence the device is held to elsewhere -- stand on the four corners of every map shape."""
    import oracle_lib as ol
    seen = {oc.route(oc.prob_planes(p, W, H), 32 if W <= 32 else 64, W, H, "narrow", c.oh, c.ow, oc.depth_of(c), c.pad, None)
            for p, H, W, _ in oc.OBSERVE_SHAPES for c in oc.CASES if (c.prob, c.H, c.W) == (p, H, W)}
    assert seen == {"huge", "k_obs0", "k_obs1", "k_obs2", "k_obs3"}
    sizes = {H * W for p, H, W in oc.FUSED_SHAPES if p == "binary"}
    assert any(s % 64 == 0 for s in sizes) and any(s % 16 for s in sizes)
    assert {"fused_rows32", "fused_rows64", "fused_hot8"} == {c.route for c in oc.CASES if (c.prob, c.H, c.W) in oc.FUSED_SHAPES and c.rep == "turtle" and c.route.startswith("fused")}
    for prob, H, W in oc.FUSED_SHAPES:
        cases, seed, tape = oc.narrow_plan(prob, H, W)
        assert len(cases) >= 20 and tape.shape == (oc.NARROW_STEPS * len(cases), oc.NARROW_ENVS)
        corners, seen = {(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)}, set()
        for i in range(oc.NARROW_ENVS):
            o = ol.OracleEnv(prob, "narrow")
            o.adjust_param(width=W, height=H)
            o.adjust_param(change_percentage=0.9)
            o.seed(seed + i)
            o.reset()
            seen |= {(int(x), int(y)) for x, y in o.rollout(tape[:, i], want_maps=False, want_heat=False)["pos"]} & corners
            if seen == corners:
                break
        assert seen == corners, (prob, H, W, seen)


def test_route_rule_pinned_against_obs_lean_mode(sim):
    """obs_cases.lean_mode is the C obs_lean_mode on the whole grid: planes {1, 3} x word width x W 1..64 x oh, ow 1..70 x depth
    {1, 2, 5, 8} x pad 0..8; and the struct the simulator declares is worklist.h's."""
    depths = np.array([1, 2, 5, 8], np.int32)
    W, oh, ow, d, pad = np.meshgrid(np.arange(1, 65), np.arange(1, 71), np.arange(1, 71), depths, np.arange(0, 9), indexing="ij", sparse=True)
    seen = set()
    for nplanes in (1, 3):
        for word32 in (1, 0):
            got = np.empty((64, 70, 70, 4, 9), np.uint8)
            sim.sim_obs_lean_grid(nplanes, word32, 64, 70, _p(depths), 4, 8, _p(got))
            want = oc.lean_mode(nplanes, bool(word32), W, oh, ow, d, pad)
            assert np.array_equal(got, want), (nplanes, word32, np.argwhere(got != want)[:3])
            seen |= {(nplanes, word32, int(v)) for v in np.unique(got)}
    assert seen == {(1, 1, 0), (1, 1, 1), (1, 0, 0), (1, 0, 1), (3, 1, 0), (3, 1, 2), (3, 0, 0)}
    assert sim.sim_obs_epb() == oc.OBS_EPB
    assert oc.is_huge(256, 256, 1) and not oc.is_huge(255, 257, 1) and oc.is_huge(128, 128, 8) and not oc.is_huge(64, 64, 8)
    src = lambda rel: open(os.path.join(ROOT, rel)).read()
    field_list = lambda text: re.sub(r"//[^\n]*|\s+", "", re.search(r"struct ObsView\s*\{(.*?)\};", text, re.S).group(1))
    assert field_list(src("gym_pcgrl_amd/csrc/worklist.h")) == field_list(src("tests/hostsim/sim_obs.cpp")) == "uint8_t*out;intoh,ow,depth,centered,pad,W,H;"
    abi = src("gym_pcgrl_amd/csrc/pcgrl_abi.hip")
    assert "(size_t)OBS_EPB * S.oh * S.ow * S.depth >= ((size_t)1 << 24) / 4" in abi              # obs_is_huge, as is_huge restates it
    assert "P.group == 16 && !P.big && P.rep <= PCGRL_REP_TURTLE && P.auto_reset" in abi           # fused_step_applies, as route restates it


@pytest.mark.parametrize("family", ["rows", "rows_fall", "hot8", "general", "huge", "delta"])
def test_every_case_at_every_cursor(sim, family):
    """Every case of the table with environment i on cell i of the map (plus all-0 and all-max-tile maps under the corners): the image
    of k_obs's body (obs_write_block on the case's source, and on the byte map), and for the shapes with a lean routine the two forms of
    the fused step kernel (obs_write_block_lean with full and partial groups of four images, obs_write_env_lean), equals the rule."""
    ran = set()
    for c in (c for c in oc.CASES if c.family == family):
        if c.route == "huge":
            continue                                   # (k_obs_huge is a kernel of its own: tests/test_gpu_obs_windows.py)
        m, pos = _inputs(c)
        want = oc.expected_image(m, pos, c.oh, c.ow, c.centered, c.pad, oc.depth_of(c))
        source = _source(c)
        for s in sorted({source, 0}):
            rc, got = _run(sim, m, pos, c, s, FORM_BLOCK)
            assert rc == 0 and np.array_equal(got, want), (oc.case_id(c), "k_obs<%d>" % s, np.argwhere(got != want)[:3])
            ran.add(("block", s))
        if c.routine == "general":
            assert _run(sim, m, pos, c, source, FORM_ENV_LEAN)[0] == (-2 if source else -3)
            continue
        for form, epb, nthreads in ((FORM_BLOCK_LEAN, 64, 256), (FORM_BLOCK_LEAN, 128, 512), (FORM_BLOCK_LEAN, 256, 1024), (FORM_ENV_LEAN, 64, 256)):
            rc, got = _run(sim, m, pos, c, source, form, epb, nthreads)
            assert rc == 0 and np.array_equal(got, want), (oc.case_id(c), form, epb, np.argwhere(got != want)[:3])
            ran.add((form, source))
    assert ran, family


def test_in_place_update_for_every_cell_and_tile(sim):
    """obs_write_delta_piece: the target holds the full image of map A; one cell changes, every cell and every tile in turn; after the one
    piece is written the target is the full image of the new map -- windows that are the map, smaller, larger, of odd width.  Then
    obs_write_block_lean's delta form: changed environments get the piece, fresh ones the whole image, the others nothing."""
    done = 0
    for c in (c for c in oc.CASES if c.route == "fused_delta"):
        H, W = c.H, c.W
        a = np.random.RandomState(5 + c.ow).randint(0, 8, size=(H, W)).astype(np.uint8)
        n = H * W * 8
        new = np.repeat(a[None], n, 0)
        cells, tiles = np.arange(n) // 8, np.arange(n) % 8
        new[np.arange(n), cells // W, cells % W] = tiles
        zero = np.zeros((n, 2), np.uint8)
        old_img = oc.expected_image(np.repeat(a[None], n, 0), zero, c.oh, c.ow, 0, c.pad, 8)
        want = oc.expected_image(new, zero, c.oh, c.ow, 0, c.pad, 8)
        raw, tgt, off = _aligned(old_img.size)
        tgt[:] = old_img.reshape(-1)
        xy = np.ascontiguousarray(np.stack([cells % W, cells // W], -1).astype(np.int32))
        assert sim.sim_obs_delta(_p(new), n, H, W, 16, c.oh, c.ow, c.pad, _p(xy), C.c_void_p(tgt.ctypes.data)) == 0
        assert (raw[:off] == 0xA5).all() and (raw[off + old_img.size:] == 0xA5).all()
        assert np.array_equal(tgt.reshape(want.shape), want), (oc.case_id(c), np.argwhere(tgt.reshape(want.shape) != want)[:3])
        # a cell outside the map is clamped as update_env clamps it
        far = np.ascontiguousarray(np.stack([np.where(tiles & 1, W + 3, -2), np.where(tiles & 2, H + 5, -1)], -1).astype(np.int32))
        near = np.stack([np.where(tiles & 1, W - 1, 0), np.where(tiles & 2, H - 1, 0)], -1)
        new2 = np.repeat(a[None], n, 0)
        new2[np.arange(n), near[:, 1], near[:, 0]] = tiles
        tgt[:] = old_img.reshape(-1)
        assert sim.sim_obs_delta(_p(new2), n, H, W, 16, c.oh, c.ow, c.pad, _p(far), C.c_void_p(tgt.ctypes.data)) == 0
        assert np.array_equal(tgt.reshape(want.shape), oc.expected_image(new2, zero, c.oh, c.ow, 0, c.pad, 8)), oc.case_id(c)
        # the block form: third of the environments changed, a third fresh (a whole new map), a third untouched (their stale target stays)
        kind = np.arange(n) % 3
        act = np.ascontiguousarray(np.concatenate([xy, tiles[:, None].astype(np.int32)], 1))
        fresh_maps = np.random.RandomState(9).randint(0, 8, size=new.shape).astype(np.uint8)
        state = np.where((kind == 0)[:, None, None], new, np.where((kind == 1)[:, None, None], fresh_maps, np.repeat(a[None], n, 0)))
        changed, fresh = (kind == 0).astype(np.uint8), (kind == 1).astype(np.uint8)
        for epb, nthreads in ((64, 256), (128, 512)):
            raw, tgt, off = _aligned(old_img.size)
            tgt[:] = old_img.reshape(-1)
            rc = sim.sim_obs(_p(state), _p(zero), n, H, W, 3, 16, c.oh, c.ow, 8, 0, c.pad, FORM_BLOCK_LEAN, epb, nthreads, _p(act), _p(changed), _p(fresh),
                             C.c_void_p(tgt.ctypes.data))
            assert rc == 0 and (raw[:off] == 0xA5).all() and (raw[off + old_img.size:] == 0xA5).all()
            assert np.array_equal(tgt.reshape(want.shape), oc.expected_image(state, zero, c.oh, c.ow, 0, c.pad, 8)), (oc.case_id(c), epb)
        done += 1
    assert done == 4


def test_sanitized_stand_alone_program():
    """sim_obs.cpp with its own main(), built with the address and undefined-behaviour sanitizers and run as a program: a built-in
    table of the same shapes, every target a heap block of exactly the images' byte count, so that a store past either end is a report."""
    out = run_sanitized("sim_obs.cpp", "SIM_OBS_MAIN", 600)
    assert int(re.search(r"images (\d+)", out).group(1)) > 20000
