#!/usr/bin/env python3
"""Generate tests/golden/playthroughs_smb.npz by running the UNMODIFIED reference (where it is installed next to this
repository, like make_golden.py):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_playthroughs_smb.py

SMBProblem._run_game (smb_prob.py:90-124) asks AStarAgent with balance 1 and -- if its node does not win -- with balance 0 for a
solution and keeps the game status of the last node returned: the winner's, else the second agent's best node's.  This file keeps
that node's moves, node.getActions() (smb/engine.py:43-49), as indices into the engine's `directions` (0 stay, 1 right, 2 jump,
3 right + jump).  Data only:

  moves_<file>    int8 [N, L]: for every level of stats_smb_<file>.npz, in its order, the moves; -1 beyond the play (L = the
                  longest of the file, at least 1)
  length_<file>   int32 [N]: the number of moves
  edge_<group>_*  generated levels for what those files lack (GROUPS below): _maps uint8 [K, h, w], _power, _stats int64 [K, 8]
                  (the stats fixtures' keys), _agents int64 [K, 5] (pops of A*(1), A*(0), two unused, the winner: 0, 1 or -1 = none),
                  _moves int8 [K, L], _length int32 [K]

The levels of a group are picked from seeded candidates (candidates() below) by index: the picks were chosen, with the repository's
C oracle as a fast sieve, so that every group but height 3 (where the root already wins) has levels won by A*(1), won by A*(0)
only, and won by nobody; this script runs the reference on the picks alone and asserts that tally.

The tally printed by the run that made the committed file (times left out; about 25 s in all):

  4x9_p200: 29 levels, won by A*(1) 28, by A*(0) 1, by nobody 0, longest play 13
  6x12_p10000: 53 levels, won by A*(1) 52, by A*(0) 0, by nobody 1, longest play 18
  8x24_p400: 73 levels, won by A*(1) 62, by A*(0) 1, by nobody 10, longest play 33
  10x30_p10000: 73 levels, won by A*(1) 52, by A*(0) 0, by nobody 21, longest play 40
  14x40_p2500: 31 levels, won by A*(1) 23, by A*(0) 0, by nobody 8, longest play 47
  14x114_p1500: 27 levels, won by A*(1) 14, by A*(0) 5, by nobody 8, longest play 136
  14x114_p10000: 15 levels, won by A*(1) 10, by A*(0) 0, by nobody 5, longest play 122
  the longest play of the files: 136 moves
  edge_w123 (6 x 123, power 1500): 6 levels, won by A*(1) 2, by A*(0) 2, by nobody 2, most pops [1500, 1500], longest play 139
  edge_w250 (4 x 250, power 3200): 5 levels, won by A*(1) 2, by A*(0) 2, by nobody 1, most pops [3200, 3200], longest play 253
  edge_h3 (3 x 9, power 200): 4 levels, won by A*(1) 4, by A*(0) 0, by nobody 0, most pops [1, 0], longest play 0
  edge_p16383 (32 x 250, power 16383): 5 levels, won by A*(1) 2, by A*(0) 2, by nobody 1, most pops [16383, 16383], longest play 290
  edge_q4095 (32 x 122, power 10000): 5 levels, won by A*(1) 2, by A*(0) 2, by nobody 1, most pops [10000, 10000], longest play 153
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
from gym_pcgrl.envs.helper import get_string_map  # noqa: E402
from gym_pcgrl.envs.probs import PROBLEMS  # noqa: E402
from gym_pcgrl.envs.probs.smb import engine  # noqa: E402

FILES = ["4x9_p200", "6x12_p10000", "8x24_p400", "10x30_p10000", "14x40_p2500", "14x114_p1500", "14x114_p10000"]
KEYS = ["dist-floor", "disjoint-tubes", "enemies", "empty", "noise", "jumps", "jumps-dist", "dist-win"]


def candidates(seed, h, w, n):
    """Seeded platformer courses: a floor with gaps, walls, stairs, ledges and loose blocks; every third one has a wall nobody can jump
    or, in a low level, a pit nobody can cross.  (height 3: the engine's grid has no room for a player -- anything goes.)"""
    rs = np.random.RandomState(seed)
    out = []
    for k in range(n):
        m = np.zeros((h, w), np.uint8)
        if h > 3:
            m[h - 2:, :] = 1
            for _ in range(rs.randint(0, 3)):                       # gaps
                x0 = rs.randint(0, w)
                m[h - 2:, x0:x0 + rs.randint(1, 4)] = 0
            top = h - 2
            for _ in range(rs.randint(1, 2 + w // 12)):             # walls and stairs
                x0, hh = rs.randint(2, w), rs.randint(1, min(5, top))
                if rs.randint(2):
                    for i in range(hh):
                        if x0 + i < w:
                            m[top - (i + 1):top, x0 + i] = 3
                else:
                    m[top - hh:top, x0] = rs.choice([1, 3, 4, 6])
            if top > 3:
                for _ in range(rs.randint(0, 2 + w // 10)):         # ledges
                    y, x0 = rs.randint(0, top - 1), rs.randint(0, w)
                    m[y, x0:x0 + rs.randint(1, 8)] = rs.choice([3, 4])
                d = rs.uniform(0.0, 0.12)                           # loose blocks
                m[:top][rs.random_sample((top, w)) < d] = 1
            if k % 3 == 2:
                x0 = rs.randint(w // 2, w - 20)
                if h <= 8:                                          # (a low wall is jumped from above the screen: a pit instead)
                    m[:, x0:x0 + rs.randint(12, 20)] = 0
                else:
                    m[:top, x0] = 1
        else:
            m = rs.randint(0, 7, size=(h, w)).astype(np.uint8)
        for _ in range(rs.randint(0, 4)):
            m[rs.randint(0, h), rs.randint(0, w)] = rs.choice([2, 5])   # enemies, coins
        out.append(m)
    return out


# (group, height, width, solver_power, seed, candidates, picks)
#   w123    the narrowest course without the two-label search (width + 6 > 128)
#   w250    the widest course the library takes
#   h3      no room for a player: the root wins
#   p16383  the largest solver_power (node indices up to 65 535; no two-label search either)
#   q4095   the widest course with the two-label search; pick 59's balance-1 queue reaches 4 557 items, beyond the 4 095 slots its labels
#           cover, so that search is done again by the general one
GROUPS = [
    ("w123", 6, 123, 1500, 1, 150, [2, 8, 66, 11, 106, 42]),
    ("w250", 4, 250, 3200, 2, 150, [2, 28, 106, 18, 24]),
    ("h3", 3, 9, 200, 3, 4, [0, 1, 2, 3]),
    ("p16383", 32, 250, 16383, 10, 150, [20, 2, 8, 23, 62]),
    ("q4095", 32, 122, 10000, 6, 300, [167, 59, 86, 263, 2]),
]


def play(prob, m):
    """(pops of the two agents, two zeros, the winner or -1; the moves; the returned node): _run_game's calls in its order."""
    smap = get_string_map(m, prob.get_tile_types())
    s2c = dict((s, " # ## #"[i]) for i, s in enumerate(prob.get_tile_types()))
    H = prob._height
    lvl = ""
    for i, row in enumerate(smap):
        lvl += "   " if i < H - 3 else (" @ " if i == H - 3 else "###")
        lvl += "".join(s2c[c] for c in row)
        lvl += " | " if i < H - 3 else (" # " if i == H - 3 else "###")
        lvl += "\n"
    state = engine.State()
    state.stringInitialize(lvl.split("\n"))
    iters, win = [0, 0, 0, 0], -1
    for a, bal in enumerate((1, 0)):
        sol, node, it = engine.AStarAgent().getSolution(state, bal, prob._solver_power)
        iters[a] = it
        if node.checkWin():
            win = a
            break
    return iters + [win], [engine.directions.index(d) for d in sol], node


def pad(rows):
    L = max([1] + [len(r) for r in rows])
    out = np.full((len(rows), L), -1, np.int8)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return out


def stats_row(prob, m):
    st = prob.get_stats(get_string_map(m, prob.get_tile_types()))
    return [int(st[k]) for k in KEYS]


def main():
    out = {}
    prob = PROBLEMS["smb"]()
    longest = 0
    for f in FILES:
        d = np.load(os.path.join(HERE, "stats_smb_%s.npz" % f))
        assert [str(k) for k in d["keys"]] == KEYS
        h, w = (int(v) for v in f.split("_")[0].split("x"))
        prob._width, prob._height, prob._solver_power = w, h, int(d["solver_power"])
        assert d["maps"].shape[1:] == (h, w) and f.endswith("_p%d" % prob._solver_power)
        t0 = time.time()
        rows, tally = [], {-1: 0, 0: 0, 1: 0}
        for i, m in enumerate(d["maps"]):
            got, sol, node = play(prob, m)
            ag = d["agents"][i]
            assert (got[0], got[1], got[4]) == (ag[0], ag[1], ag[4]), (f, i, got, ag)
            gs = node.getGameStatus()
            assert gs["jumps"] == d["stats"][i][5] and (0 if got[4] >= 0 else node.getHeuristic()) == d["stats"][i][7] and node.depth == len(sol), (f, i)
            tally[got[4]] += 1
            rows.append(sol)
        out["moves_" + f] = pad(rows)
        out["length_" + f] = np.array([len(r) for r in rows], np.int32)
        longest = max(longest, max(len(r) for r in rows))
        print("  %s: %d levels, won by A*(1) %d, by A*(0) %d, by nobody %d, longest play %d, %.1fs"
              % (f, len(rows), tally[0], tally[1], tally[-1], max(len(r) for r in rows), time.time() - t0), flush=True)
    print("  the longest play of the files: %d moves" % longest)
    for name, h, w, power, seed, ncand, picks in GROUPS:
        prob._width, prob._height, prob._solver_power = w, h, power
        cands = candidates(seed, h, w, ncand)
        t0 = time.time()
        maps, stats, agents, moves, tally = [], [], [], [], {-1: 0, 0: 0, 1: 0}
        for i in picks:
            m = cands[i]
            st = stats_row(prob, m)
            ag, sol, node = play(prob, m)
            assert node.getGameStatus()["jumps"] == st[5] and (0 if ag[4] >= 0 else node.getHeuristic()) == st[7] and node.depth == len(sol), (name, i)
            maps.append(m)
            stats.append(st)
            agents.append(ag)
            moves.append(sol)
            tally[ag[4]] += 1
        agents = np.array(agents, np.int64)
        print("  edge_%s (%d x %d, power %d): %d levels, won by A*(1) %d, by A*(0) %d, by nobody %d, most pops %s, longest play %d, %.1fs"
              % (name, h, w, power, len(maps), tally[0], tally[1], tally[-1], agents[:, :2].max(0).tolist(), max(len(r) for r in moves), time.time() - t0),
              flush=True)
        if h == 3:
            assert tally[0] == len(maps) and all(len(r) == 0 for r in moves)
        else:
            assert min(tally.values()) >= 1, (name, tally)
        out["edge_%s_maps" % name] = np.array(maps, np.uint8)
        out["edge_%s_power" % name] = np.array(power, np.int64)
        out["edge_%s_stats" % name] = np.array(stats, np.int64)
        out["edge_%s_agents" % name] = agents
        out["edge_%s_moves" % name] = pad(moves)
        out["edge_%s_length" % name] = np.array([len(r) for r in moves], np.int32)
    np.savez_compressed(os.path.join(HERE, "playthroughs_smb.npz"), **out)
    print("wrote playthroughs_smb.npz")


if __name__ == "__main__":
    main()
