#!/usr/bin/env python3
"""Generate tests/golden/paths.npz by running the UNMODIFIED reference (where it is installed next to this repository, like
make_golden.py):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_paths.py

calc_longest_path (helper.py:250-264) and ZeldaProblem.get_stats (zelda_prob.py:91-110) compute run_dikjstra maps (helper.py:222-237),
keep one number of each and throw the maps away.  This file keeps the paths those maps define, by the rule of include/pcgrl_hip.h
(pcgrl_get_paths): the leg to a cell t is built backwards from t, the predecessor of a cell c with D[c] > 0 being the first neighbour
n of c in run_dikjstra's own order -- (dx, dy) = (-1,0), (1,0), (0,-1), (0,1) -- with D[n] == D[c] - 1.  Everything but those few
lines is the reference's: get_tile_locations, run_dikjstra, calc_longest_path, ZeldaProblem.get_stats.  Data only:

  groups                the names of the groups below, in order
  cells_<g>   int16 [N, legs, L]  cell i of each leg as y * W + x, start -> target, -1 beyond it (L = the longest of the group + 1)
  length_<g>  int32 [N, legs]     steps of each leg (cells - 1); -1: the leg does not exist
      binary: one leg ("longest"); zelda: three ("key", "door", "enemy")
  ties_<g>    int32 [N]           binary: the regions whose second map reaches path-length (the first of them has the leg);
                                  zelda: the enemy cells at the distance nearest-enemy (the first of them is the target), 0 = none
  for <g> = stats_<prob>_<h>x<w>: the levels of tests/golden/stats_<prob>_<h>x<w>.npz, in its order
  for the seeded random groups (rand_*) and the hand-made ones (hand_*) also
  maps_<g>    uint8 [N, h, w]     and     stats_<g>   int64 [N, 2 or 7]   the reference's get_stats, in the stats fixtures' key order
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

import gym_shim  # noqa: E402

gym = gym_shim.install()
import gym_pcgrl  # noqa: E402,F401
from gym_pcgrl.envs.helper import calc_longest_path, get_string_map, get_tile_locations, run_dikjstra  # noqa: E402
from gym_pcgrl.envs.probs import PROBLEMS  # noqa: E402

BINARY = ["1x1", "1x9", "8x1", "3x7", "5x5", "14x14", "16x11", "9x32", "64x64"]
ZELDA = ["5x5", "7x11", "11x16", "16x11"]
BINARY_KEYS = ["regions", "path-length"]
ZELDA_KEYS = ["player", "key", "door", "enemies", "regions", "nearest-enemy", "path-length"]
ENEMIES = ["bat", "spider", "scorpion"]


def walk_back(D, tx, ty):
    """The leg that ends on (tx, ty), start -> target, as y * W + x; [] when the cell was not reached."""
    H, W = D.shape
    if D[ty][tx] < 0:
        return -1, []
    cells, x, y = [ty * W + tx], tx, ty
    while D[y][x] > 0:
        for dx, dy in [(-1, 0), (1, 0), (0, -1), (0, 1)]:
            nx, ny = x + dx, y + dy
            if 0 <= nx < W and 0 <= ny < H and D[ny][nx] == D[y][x] - 1:
                x, y = nx, ny
                break
        else:
            raise AssertionError("no predecessor")
        cells.append(y * W + x)
    return int(D[ty][tx]), cells[::-1]


def first_argmax(D):
    y, x = np.unravel_index(np.argmax(D, axis=None), D.shape)
    return int(x), int(y)


def binary_legs(prob, m):
    smap = get_string_map(m, prob.get_tile_types())
    locs = get_tile_locations(smap, prob.get_tile_types())
    st = prob.get_stats(smap)
    path = calc_longest_path(smap, locs, ["empty"])
    assert path == st["path-length"]
    seen = np.zeros(m.shape)
    leg, ties = (-1, []), 0
    for (x, y) in locs["empty"]:                          # calc_longest_path's own loop; the first region with the final value has the leg
        if seen[y][x] > 0:
            continue
        D, vis = run_dikjstra(x, y, smap, ["empty"])
        seen += vis
        mx, my = first_argmax(D)
        D2, _ = run_dikjstra(mx, my, smap, ["empty"])
        if np.max(D2) == path:
            ties += 1
            if ties == 1:
                tx, ty = first_argmax(D2)
                leg = walk_back(D2, tx, ty)
                assert leg[0] == path and leg[1][0] == my * m.shape[1] + mx
    assert (ties == 0) == (not locs["empty"])
    return [st[k] for k in BINARY_KEYS], [leg], ties


def zelda_legs(prob, m):
    smap = get_string_map(m, prob.get_tile_types())
    locs = get_tile_locations(smap, prob.get_tile_types())
    st = prob.get_stats(smap)
    legs, ties = [(-1, []), (-1, []), (-1, [])], 0
    if st["player"] == 1 and st["regions"] == 1:
        px, py = locs["player"][0]
        if st["key"] == 1 and st["door"] == 1:
            kx, ky = locs["key"][0]
            dx, dy = locs["door"][0]
            D, _ = run_dikjstra(px, py, smap, ["empty", "key", "player"] + ENEMIES)
            legs[0] = walk_back(D, kx, ky)
            D, _ = run_dikjstra(kx, ky, smap, ["empty", "player", "key", "door"] + ENEMIES)
            legs[1] = walk_back(D, dx, dy)
            assert legs[0][0] + legs[1][0] == st["path-length"]
        if st["enemies"] > 0:
            D, _ = run_dikjstra(px, py, smap, ["empty", "player"] + ENEMIES)
            near = sorted((y, x) for t in ENEMIES for (x, y) in locs[t] if D[y][x] > 0 and D[y][x] == st["nearest-enemy"])
            ties = len(near)
            if near:
                legs[2] = walk_back(D, near[0][1], near[0][0])
                assert legs[2][0] == st["nearest-enemy"]
            else:
                assert st["nearest-enemy"] == prob._width * prob._height
    return [st[k] for k in ZELDA_KEYS], legs, ties


def pack(legs_of_maps):
    L = max([1] + [len(c) for legs in legs_of_maps for (_, c) in legs])
    cells = np.full((len(legs_of_maps), len(legs_of_maps[0]), L), -1, np.int16)
    length = np.zeros((len(legs_of_maps), len(legs_of_maps[0])), np.int32)
    for i, legs in enumerate(legs_of_maps):
        for j, (n, c) in enumerate(legs):
            assert len(c) == n + 1
            cells[i, j, :len(c)] = c
            length[i, j] = n
    return cells, length


def run_group(out, name, probname, maps, want_stats=None, store=False):
    prob = PROBLEMS[probname]()
    prob._height, prob._width = int(maps.shape[1]), int(maps.shape[2])
    fn = binary_legs if probname == "binary" else zelda_legs
    t0 = time.time()
    stats, legs, ties = [], [], []
    for m in maps:
        s, l, t = fn(prob, m)
        stats.append(s)
        legs.append(l)
        ties.append(t)
    stats = np.array(stats, np.int64)
    if want_stats is not None:
        assert np.array_equal(stats, want_stats), name
    out["cells_" + name], out["length_" + name] = pack(legs)
    out["ties_" + name] = np.array(ties, np.int32)
    if store:
        out["maps_" + name], out["stats_" + name] = np.ascontiguousarray(maps, np.uint8), stats
    out.setdefault("groups", []).append(name)
    ln = out["length_" + name]
    print("  %s: %d levels, legs present %s, longest %d, %.1fs" % (name, len(maps), (ln >= 0).sum(0).tolist(), int(ln.max()), time.time() - t0), flush=True)


def random_binary(rs, n, h, w):
    return np.stack([(rs.rand(h, w) < p).astype(np.uint8) for p in np.linspace(0.15, 0.6, n)])


def random_zelda(rs, n, h, w):
    """Half of the levels playable (one player, key and door, a few enemies, sparse walls), half arbitrary tiles."""
    maps = []
    for i in range(n):
        if i % 2:
            maps.append(rs.choice(8, size=(h, w), p=[0.5, 0.25, 0.03, 0.03, 0.03, 0.06, 0.05, 0.05]).astype(np.uint8))
            continue
        m = (rs.rand(h, w) < 0.08 + 0.02 * (i % 8)).astype(np.uint8)
        at = rs.choice(h * w, size=3 + i % 5, replace=False)
        m.flat[at[0]], m.flat[at[1]], m.flat[at[2]] = 2, 3, 4
        for k, c in enumerate(at[3:]):
            m.flat[c] = 5 + k % 3
        maps.append(m)
    return np.stack(maps)


def hand_levels():
    serp = np.ones((64, 64), np.uint8)                    # the longest leg the form can have: a corridor through every other row
    serp[0::2, :] = 0
    for k, y in enumerate(range(1, 64, 2)):
        serp[y, 63 if k % 2 == 0 else 0] = 0
    twins = np.ones((3, 7), np.uint8)                     # two equal regions: the first must win
    twins[:, 0:3] = 0
    twins[:, 4:7] = 0
    z = np.ones((3, 7, 11), np.uint8)
    z[:, 1:6, 1:10] = 0
    # the door walled off
    z[0, 1, 1], z[0, 3, 4], z[0, 5, 8], z[0, 5, 9], z[0, 4, 9], z[0, 4, 8] = 2, 3, 1, 4, 1, 6
    z[0, 5, 8] = 1
    # two enemies at the nearest distance (left of and below the player: the first in row-major order is the target)
    z[1, 3, 5], z[1, 3, 3], z[1, 5, 5], z[1, 1, 1], z[1, 1, 9], z[1, 2, 5] = 2, 5, 7, 3, 4, 1
    # enemies reachable only through the key
    z[2] = 1
    z[2, 3, 1:8] = [2, 0, 0, 3, 0, 6, 4]
    z[2, 2, 6] = 7
    return np.stack([serp, np.zeros((64, 64), np.uint8)]), twins[None], z


def main():
    out = {}
    for size in BINARY:
        d = np.load(os.path.join(HERE, "stats_binary_%s.npz" % size))
        assert list(d["keys"]) == BINARY_KEYS
        run_group(out, "stats_binary_" + size, "binary", d["maps"], d["stats"])
    for size in ZELDA:
        d = np.load(os.path.join(HERE, "stats_zelda_%s.npz" % size))
        assert list(d["keys"]) == ZELDA_KEYS
        run_group(out, "stats_zelda_" + size, "zelda", d["maps"], d["stats"])
    rs = np.random.RandomState(20240607)
    # the (lane group, mask width) corners the stats fixtures leave out
    for h, w in ((5, 40), (16, 33), (16, 32), (17, 9), (17, 33)):
        run_group(out, "rand_binary_%dx%d" % (h, w), "binary", random_binary(rs, 10, h, w), store=True)
    for h, w in ((5, 40), (16, 33), (17, 9)):
        run_group(out, "rand_zelda_%dx%d" % (h, w), "zelda", random_zelda(rs, 16, h, w), store=True)
    big, twins, z = hand_levels()
    run_group(out, "hand_binary_64x64", "binary", big, store=True)
    run_group(out, "hand_binary_3x7", "binary", twins, store=True)
    run_group(out, "hand_zelda_7x11", "zelda", z, store=True)
    out["groups"] = np.array(out["groups"])
    path = os.path.join(HERE, "paths.npz")
    np.savez_compressed(path, **out)
    print("wrote paths.npz, %d bytes" % os.path.getsize(path))


if __name__ == "__main__":
    main()
