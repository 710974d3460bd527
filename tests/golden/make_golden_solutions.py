#!/usr/bin/env python3
"""Generate tests/golden/solutions_sokoban.npz by running the UNMODIFIED reference (where it is installed next to this
repository, like make_golden.py):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_solutions.py

SokobanProblem.get_stats(map)["solution"] (sokoban_prob.py:133-145) is the list of moves of the first agent of _run_game
that wins.  The stats fixtures keep only its length (stats[:, 5]); this file keeps the moves.  Data only:

  moves_<h>x<w>   int8 [N, L]: for every level of stats_sokoban_<h>x<w>.npz, in its order, the index of each move in engine.py's
                  `directions` (0..3 = L, R, U, D), -1 beyond the solution (L = the longest of the file, at least 1)
  hand_*          hand-made levels with more than seven crates (the generic search of csrc/sokoban_solver.h):
                  hand_map_<i> uint8 [h, w], hand_power [K], hand_stats [K, 6] (the stats fixtures' keys), hand_agents [K, 5]
                  (pops of BFS, A*(1), A*(0.5), A*(0); the winner, -1 = none), hand_moves int8 [K, L]
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
from gym_pcgrl.envs.probs.sokoban import engine  # noqa: E402

SIZES = ["4x6", "5x5", "5x6", "6x6", "7x7", "7x8", "8x8"]
KEYS = ["player", "crate", "target", "regions", "dist-win", "sol-length"]


def solution_of(prob, m):
    st = prob.get_stats(get_string_map(m, prob.get_tile_types()))
    return st, [engine.directions.index(a) for a in st["solution"]]


def agents_of(prob, m):
    """The agents of _run_game in its order: pops of each one that ran, the winner (-1: none)."""
    chars = " #@$."
    rows = ["#" * (prob._width + 2)] + ["#" + "".join(chars[t] for t in r) + "#" for r in m] + ["#" * (prob._width + 2), ""]
    state = engine.State()
    state.stringInitialize(rows)
    iters, win = [0, 0, 0, 0], -1
    for a, bal in enumerate((None, 1, 0.5, 0)):
        if bal is None:
            sol, st, it = engine.BFSAgent().getSolution(state, prob._solver_power)
        else:
            sol, st, it = engine.AStarAgent().getSolution(state, bal, prob._solver_power)
        iters[a] = it
        if st.checkWin():
            win = a
            break
    return iters + [win]


def pad(rows, width=None):
    L = max([1] + [len(r) for r in rows]) if width is None else width
    out = np.full((len(rows), L), -1, np.int8)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return out


def column_level(h, w, col, tcol):
    """A crate in every row of column `col`, a target in every row of column `tcol`, the player in the top left corner."""
    m = np.zeros((h, w), np.uint8)
    m[:, col] = 3
    m[:, tcol] = 4
    m[0, 0] = 2
    return m


def main():
    prob = PROBLEMS["sokoban"]()
    out = {}
    for size in SIZES:
        d = np.load(os.path.join(HERE, "stats_sokoban_%s.npz" % size))
        h, w = (int(v) for v in size.split("x"))
        prob._width, prob._height, prob._solver_power = w, h, int(d["solver_power"])
        t0 = time.time()
        rows = []
        for i, m in enumerate(d["maps"]):
            st, sol = solution_of(prob, m)
            assert len(sol) == d["stats"][i, 5] and int(st["dist-win"]) == d["stats"][i, 4], (size, i)
            rows.append(sol)
        out["moves_" + size] = pad(rows)
        print("  %s: %d levels, %d solved, longest %d, %.1fs" % (size, len(rows), sum(1 for r in rows if r), max(len(r) for r in rows), time.time() - t0), flush=True)
    hand = [(8, 6, 2, 3, 5000), (8, 6, 2, 3, 600), (9, 6, 2, 3, 5000), (8, 7, 2, 4, 5000)]
    stats, agents, moves = [], [], []
    for i, (h, w, col, tcol, power) in enumerate(hand):
        m = column_level(h, w, col, tcol)
        prob._width, prob._height, prob._solver_power = w, h, power
        t0 = time.time()
        st, sol = solution_of(prob, m)
        ag = agents_of(prob, m)
        assert (ag[4] >= 0) == (len(sol) > 0)
        out["hand_map_%d" % i] = m
        stats.append([int(st[k]) if k != "sol-length" else len(sol) for k in KEYS])
        agents.append(ag)
        moves.append(sol)
        print("  hand %d: %dx%d power %d: %d moves, agents %s, %.1fs" % (i, h, w, power, len(sol), ag, time.time() - t0), flush=True)
    out["hand_power"] = np.array([p for (_, _, _, _, p) in hand], np.int64)
    out["hand_stats"] = np.array(stats, np.int64)
    out["hand_agents"] = np.array(agents, np.int64)
    out["hand_moves"] = pad(moves)
    np.savez_compressed(os.path.join(HERE, "solutions_sokoban.npz"), **out)
    print("wrote solutions_sokoban.npz")


if __name__ == "__main__":
    main()
