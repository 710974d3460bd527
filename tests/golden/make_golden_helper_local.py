#!/usr/bin/env python3
"""Generate tests/golden/helper_local.npz by running the UNMODIFIED reference helper.py (where it is installed next to this repository,
like make_golden_helper.py):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_helper_local.py

get_floor_dist, get_type_grouping, get_changes (helper.py:56-137) and, for every cell, _calc_dist_floor and _calc_group_value
(helper.py:37-85) -- the reference's own calls, on lists of lists, with the tile arguments as lists.  Data only; to stay below helper.npz
the levels of all groups lie end to end:

  groups            the names of the groups below, in order
  levels  int64 [N, 13]   per level: group (index into groups), h, w, from_tiles, floor_tiles, group_tiles (sets, bit t = tile t),
                          group_min, group_max, noffsets, then the results floor_dist, grouping, changes horizontal, changes vertical
  offsets int8 [N, 16, 2] the level's relLocs (dx, dy), the first noffsets count
  maps    uint8 [cells]   the levels' tiles, each row-major, in order (level i starts at the sum of h * w before it)
  floor_map int16 [cells] _calc_dist_floor(map, x, y, floor) of every cell, laid out like maps
  group_map int8 [cells]  _calc_group_value(map, x, y, group, relLocs) of every cell

The groups: rand_<h>x<w>, seeded random maps of 2, 3, 5 and 8 tile values in turn, each with one of the query sets QUERIES in turn -- the
small shapes, the corners of the kernel's forms (sixteen lanes up to 16 columns, the stage up to 64 x 64), smb's 14 x 114, 3 x 255 -- and
hand_6x8, the levels named in hand_levels().
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

import gym_shim  # noqa: E402

gym_shim.install()
from gym_pcgrl.envs.helper import _calc_dist_floor, _calc_group_value, get_changes, get_floor_dist, get_type_grouping  # noqa: E402

# (h, w, levels)
SHAPES = [(1, 1, 10), (1, 9, 10), (8, 1, 10), (5, 5, 20), (14, 14, 10), (17, 9, 10), (3, 7, 20), (9, 16, 5), (9, 17, 5), (16, 32, 5), (16, 33, 5),
          (17, 32, 5), (9, 64, 5), (64, 64, 3), (65, 2, 5), (2, 65, 5), (65, 64, 3), (64, 65, 3), (14, 114, 5), (3, 255, 5)]
NTILES = (2, 3, 5, 8)
EIGHT = [(-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1)]
# (from, floor, group, relLocs, min, max)
QUERIES = [((2,), (1, 3, 4, 6), (6,), [(-1, 0), (1, 0)], 1, 1),                                       # (a) smb's kind: enemies over solid ground, lone tubes
           ((0, 1), (1,), (0,), EIGHT, 2, 5),                                                         # (b) overlapping sets
           (tuple(range(8)), (), (1, 2), [(0, 0), (2, 0), (2, 0), (0, -3), (-127, 0), (0, 127)], 0, 0),       # (c) no floor; doubled and far offsets
           ((), tuple(range(8)), (), [], 0, 0),                                                       # (d) empty from, group and offsets
           ((0,), (0,), (0,), [(0, -1), (0, 1), (-1, 0), (1, 0)], 3, 1)]                              # (e) min > max


def bits(tiles):
    return int(sum(1 << t for t in tiles))


def reference(m, q):
    """One level: (floor_dist, grouping, changes h, changes v, floor_map, group_map) by the reference's own functions."""
    frm, floor, group, rel, lo, hi = q
    h, w = m.shape
    lists = [[int(v) for v in row] for row in m]
    frm, floor, group, rel = list(frm), list(floor), list(group), [tuple(r) for r in rel]
    fmap = np.array([[_calc_dist_floor(lists, x, y, floor) for x in range(w)] for y in range(h)])
    gmap = np.array([[_calc_group_value(lists, x, y, group, rel) for x in range(w)] for y in range(h)])
    return (get_floor_dist(lists, frm, floor), get_type_grouping(lists, group, rel, lo, hi), get_changes(lists, False), get_changes(lists, True),
            fmap, gmap)


def hand_levels():
    """On 6 rows x 8 columns; tile 2 is the from tile, tile 1 the floor of the first four."""
    a = np.zeros((6, 8), np.uint8)
    a[5, 1] = 2                                     # a from tile on the bottom row, no floor in its column: H - 1
    a[2, 3], a[3, 3] = 2, 1                         # a floor directly below: 0
    a[0, 5], a[4, 5] = 2, 1                         # three cells of air between: 3
    one = ((2,), (1,), (2,), [(0, 1)], 0, 1)
    b = np.zeros((6, 8), np.uint8)
    b[1, 2] = b[4, 2] = 2                           # a from tile that is a floor tile: -1 each, the sum is negative
    both = ((2,), (2, 1), (2,), [(0, 3)], 1, 1)
    c = np.full((6, 8), 2, np.uint8)                # all cells from tiles, a column without floor in every row but column 6's
    c[3, 6] = 1
    d = np.full((6, 8), 30, np.uint8)               # tiles 30 and 31 in use
    d[::2, 1::3] = 31
    d[5, 0] = 29
    high = ((30, 29), (31,), (31, 30), [(1, 0), (0, 1), (-1, -1)], 2, 3)
    e = np.full((6, 8), 3, np.uint8)                # offsets that leave the map at each of the four edges and corners
    e[2, 4] = 0
    ring = ((3,), (0,), (3,), EIGHT + [(0, -6), (8, 0), (-7, 5), (7, -5), (0, 0), (-128, -128), (127, 127), (-8, 0)], 4, 9)
    edges = ((3,), (0,), (3,), [(-1, 0), (1, 0), (0, -1), (0, 1)], 2, 3)
    return [(a, one), (b, both), (c, one), (d, high), (e, ring), (e, edges)]


def main():
    rs = np.random.RandomState(20241022)
    groups, levels, offsets, maps, fmaps, gmaps = [], [], [], [], [], []

    def add(name, m, q):
        if name not in groups:
            groups.append(name)
        r = reference(m, q)
        h, w = m.shape
        levels.append([groups.index(name), h, w, bits(q[0]), bits(q[1]), bits(q[2]), q[4], q[5], len(q[3])] + list(r[:4]))
        off = np.zeros((16, 2), np.int8)
        off[:len(q[3])] = np.array(q[3], np.int64).reshape(-1, 2)
        offsets.append(off)
        maps.append(m.reshape(-1))
        fmaps.append(r[4].reshape(-1))
        gmaps.append(r[5].reshape(-1))

    for h, w, n in SHAPES:
        for i in range(n):
            T = NTILES[i % 4]
            p0 = 0.35 + 0.5 * rs.rand()
            m = rs.choice(T, size=(h, w), p=[p0] + [(1 - p0) / (T - 1)] * (T - 1)).astype(np.uint8)
            add("rand_%dx%d" % (h, w), m, QUERIES[i % 5])
        print("  rand_%dx%d: %d levels" % (h, w, n), flush=True)
    for m, q in hand_levels():
        add("hand_6x8", m, q)
    out = dict(groups=np.array(groups), levels=np.array(levels, np.int64), offsets=np.stack(offsets), maps=np.concatenate(maps).astype(np.uint8),
               floor_map=np.concatenate(fmaps).astype(np.int16), group_map=np.concatenate(gmaps).astype(np.int8))
    assert np.array_equal(out["floor_map"], np.concatenate(fmaps)) and np.array_equal(out["group_map"], np.concatenate(gmaps))
    path = os.path.join(HERE, "helper_local.npz")
    np.savez_compressed(path, **out)
    print("wrote helper_local.npz, %d levels, %d cells, %d bytes (helper.npz: %d)" % (
        len(levels), len(out["maps"]), os.path.getsize(path), os.path.getsize(os.path.join(HERE, "helper.npz"))))


if __name__ == "__main__":
    main()
