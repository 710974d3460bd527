#!/usr/bin/env python3
"""Generate tests/golden/helper.npz by running the UNMODIFIED reference helper.py (where it is installed next to this repository, like
make_golden_paths.py):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_helper.py

calc_num_regions, calc_longest_path, run_dikjstra and calc_num_reachable_tile (helper.py:170-296) take a LIST of passable values, and
_get_certain_tiles orders cells by list position first: calc_longest_path and the numbering of the color_map depend on the list's
order.  pcgrl_tile_graph (include/pcgrl_hip.h) takes a SET; its rule: every result is the reference's on the level in which every
passable tile has been renamed to one single value.  This file applies that rule by renaming before it calls; everything else is the
reference's -- get_tile_locations, _get_certain_tiles, _flood_fill (calc_num_regions' own loop, with the color_map kept), run_dikjstra,
calc_longest_path, and calc_num_reachable_tile where a level's sets let it be called as it is.  What does not depend on the order
(regions, dist, reach) is also checked against the reference on the level as given, with the values as a sorted list.  Data only:

  groups                          the names of the groups below, in order
  maps_<g>          uint8 [N, h, w]
  levels_<g>        int64 [N, 8]  per level: passable, source_tiles, reach_tiles -- the level's tile sets, bit t = tile t (a few sets per
                                  group, in turn) --, sources (-2: the source is the first cell of source_tiles; else the source cell
                                  given, y * w + x, -1 = none), then the results regions, longest, reach, source (the cell that was
                                  used, -1 if none)
  labels_<g>, dist_<g>            int16 [N, h, w]
  order_dependent   int32 [groups]  the levels of each group whose calc_longest_path changes with the list order (sorted or reversed
                                  against the renamed level): information, not a check

The groups: rand_<h>x<w>, seeded random maps of 2, 3, 5 and 8 tile values in turn, on every (lane group, mask width) corner of the
kernel -- forty levels a shape up to 5 x 5, twenty at 17 x 9 and 14 x 14, eight at about 16 x 32 and four at 64 x 64, which keeps this
file below paths.npz; 3 x 7 is the shape of the grid-stride test -- and hand_64x64 / hand_7x9, the levels named in hand_levels().
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

import gym_shim  # noqa: E402

gym_shim.install()
from gym_pcgrl.envs.helper import (_flood_fill, _get_certain_tiles, calc_longest_path, calc_num_reachable_tile,  # noqa: E402
                                   calc_num_regions, get_tile_locations, run_dikjstra)

SHAPES = [(1, 1, 40), (1, 9, 40), (8, 1, 40), (5, 5, 40), (17, 9, 20), (14, 14, 20), (16, 32, 8), (16, 33, 8), (17, 32, 8), (9, 64, 8), (64, 64, 4), (3, 7, 40)]
NTILES = (2, 3, 5, 8)
MERGED, START = 100, 101          # the single values the passable / the source tiles are renamed to
# (passable, source_tiles, reach_tiles, the source is given as a cell)
CASES = [((0,), (0,), (0,), False),
         ((1, 2, 4, 7), (1, 2), (0, 2, 4), False),
         ((0, 3, 4, 6), (), (1, 3, 6), True),
         ((0, 2, 5), (5, 2), tuple(range(8)), False)]


def bits(tiles):
    return int(sum(1 << t for t in tiles))


def as_lists(a):
    return [[int(v) for v in row] for row in a]


def reference(m, passable, source_tiles, reach_tiles, source):
    """One level by the set rule.  source: -2 = the first cell of source_tiles, else the given cell (-1: none)."""
    h, w = m.shape
    values = list(range(32)) + [MERGED, START]
    merged = as_lists(np.where(np.isin(m, passable), MERGED, m))
    locs = get_tile_locations(merged, values)
    regions = calc_num_regions(merged, locs, [MERGED])
    longest = calc_longest_path(merged, locs, [MERGED])
    # calc_num_regions' loop (helper.py:197-207) with the color_map kept
    labels = np.full((h, w), -1)
    index = 0
    for (x, y) in _get_certain_tiles(locs, [MERGED]):
        if _flood_fill(x, y, labels, merged, index + 1, [MERGED]) > 0:
            index += 1
    assert index == regions
    if source == -2:
        starts = _get_certain_tiles(get_tile_locations(as_lists(np.where(np.isin(m, source_tiles), START, m)), values), [START])
        cell = starts[0][1] * w + starts[0][0] if starts else -1
    else:
        cell = int(source)
    if cell >= 0:
        dist, visited = run_dikjstra(cell % w, cell // w, merged, [MERGED])
        assert np.array_equal(visited > 0, dist >= 0)
    else:
        dist = np.full((h, w), -1)
    reach = int(((dist >= 0) & np.isin(m, reach_tiles)).sum())
    # what does not depend on the order, on the level as given
    plain = as_lists(m)
    plocs = get_tile_locations(plain, values)
    assert calc_num_regions(plain, plocs, sorted(passable)) == regions
    if cell >= 0:
        assert np.array_equal(run_dikjstra(cell % w, cell // w, plain, sorted(passable))[0], dist)
    if source == -2 and len(source_tiles) == 1 and cell >= 0:
        assert calc_num_reachable_tile(plain, plocs, source_tiles[0], sorted(passable), sorted(reach_tiles)) == reach
    order = int(any(calc_longest_path(plain, plocs, lst) != longest for lst in (sorted(passable), sorted(passable, reverse=True)))) if len(passable) > 1 else 0
    return regions, longest, labels, dist, reach, cell, order


def run_group(out, name, maps, sets, sources):
    t0 = time.time()
    res = [reference(m, s[0], s[1], s[2], src) for m, s, src in zip(maps, sets, sources)]
    out["maps_" + name] = np.ascontiguousarray(maps, np.uint8)
    out["levels_" + name] = np.array([[bits(s[0]), bits(s[1]), bits(s[2]), src, r[0], r[1], r[4], r[5]] for s, src, r in zip(sets, sources, res)], np.int64)
    out["labels_" + name] = np.stack([r[2] for r in res]).astype(np.int16)
    out["dist_" + name] = np.stack([r[3] for r in res]).astype(np.int16)
    out.setdefault("order_dependent", []).append(sum(r[6] for r in res))
    out.setdefault("groups", []).append(name)
    print("  %s: %d levels, regions <= %d, longest <= %d, dist <= %d, order-dependent %d, %.1fs" % (
        name, len(maps), out["levels_" + name][:, 4].max(), out["levels_" + name][:, 5].max(), out["dist_" + name].max(),
        out["order_dependent"][-1], time.time() - t0), flush=True)


def random_group(rs, h, w, n):
    maps, sets, sources = [], [], []
    for i in range(n):
        T = NTILES[i % 4]
        p0 = 0.35 + 0.5 * rs.rand()
        maps.append(rs.choice(T, size=(h, w), p=[p0] + [(1 - p0) / (T - 1)] * (T - 1)).astype(np.uint8))
        case = CASES[(i // 4 + i) % 4]
        sets.append(case[:3])
        sources.append((-1 if rs.rand() < 0.1 else int(rs.randint(h * w))) if case[3] else -2)
    return np.stack(maps), sets, sources


def spiral(n):
    """A corridor one cell wide from the corner to the middle."""
    m = np.ones((n, n), np.uint8)
    x = y = 0
    dx, dy = 1, 0
    m[0, 0] = 0
    inside = lambda a, b: 0 <= a < n and 0 <= b < n
    while True:
        for _ in range(2):
            nx, ny, fx, fy = x + dx, y + dy, x + 2 * dx, y + 2 * dy
            if inside(nx, ny) and m[ny, nx] == 1 and (not inside(fx, fy) or m[fy, fx] == 1):
                x, y = nx, ny
                m[y, x] = 0
                break
            dx, dy = -dy, dx
        else:
            return m


def hand_levels():
    one = ((0,), (0,), (0,))
    checker = ((np.arange(64)[:, None] + np.arange(64)[None, :]) % 2).astype(np.uint8)      # 2 048 regions
    high = np.full((64, 64), 30, np.uint8)                                                  # tiles 30 and 31 in use, on the widest form
    high[::3, 5:] = 31
    high[10, 10] = 29
    big = [(np.zeros((64, 64), np.uint8), one, -2),                  # all open
           (np.ones((64, 64), np.uint8), one, -2),                   # all blocked
           (checker, one, -2),
           (spiral(64), one, -2),                                    # the longest distances
           (high, ((30, 29), (29,), (30, 31)), -2)]
    comb = np.ones((7, 9), np.uint8)                                 # a spine with teeth
    comb[0, :] = 0
    comb[:, ::2] = 0
    two = np.zeros((7, 9), np.uint8)
    two[3, :] = 1
    two[5, 2] = two[1, 6] = 2                                        # two cells of source_tiles: the first is taken
    walls = (np.arange(63).reshape(7, 9) % 4 == 1).astype(np.uint8)
    edge = np.zeros((7, 9), np.uint8)
    edge[0, 0] = edge[6, 8] = 31
    edge[0, 1:] = 30
    edge[1:, 4] = 7
    small = [(comb, one, -2),
             (walls, ((0,), (), (0, 1)), 9),                         # a source on an impassable cell
             (walls, ((0,), (), (0, 1)), -1),                        # source -1
             (walls, ((0,), (5,), (0, 1)), -2),                      # no cell of source_tiles
             (two, ((0, 2), (2,), (2,)), -2),
             (two, ((0,), (2,), (0, 2)), -2),                        # the source tile itself is not passable
             (edge, ((30, 31), (31,), (31, 7)), -2),                 # tile values 30 and 31 in use
             (edge, ((0, 31), (), (0,)), 62)]
    return big, small


def main():
    out = {}
    rs = np.random.RandomState(20241021)
    for h, w, n in SHAPES:
        run_group(out, "rand_%dx%d" % (h, w), *random_group(rs, h, w, n))
    for name, levels in zip(("hand_64x64", "hand_7x9"), hand_levels()):
        run_group(out, name, np.stack([l[0] for l in levels]), [l[1] for l in levels], [l[2] for l in levels])
    out["groups"] = np.array(out["groups"])
    out["order_dependent"] = np.array(out["order_dependent"], np.int32)
    path = os.path.join(HERE, "helper.npz")
    np.savez_compressed(path, **out)
    print("wrote helper.npz, %d bytes (paths.npz: %d)" % (os.path.getsize(path), os.path.getsize(os.path.join(HERE, "paths.npz"))))


if __name__ == "__main__":
    main()
