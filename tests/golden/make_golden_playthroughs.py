#!/usr/bin/env python3
"""Generate tests/golden/playthroughs.npz by running the UNMODIFIED reference (where it is installed next to this
repository, like make_golden.py):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_playthroughs.py

MDungeonProblem._run_game (mdungeon_prob.py:100-138) and DDaveProblem._run_game (ddave_prob.py:92-127) ask AStarAgent with
balance 1, 0.5, 0 and then BFSAgent for a solution -- node.getActions() (mdungeon/engine.py:43-49) of the node the agent ends
on -- and keep only len(sol) and the game status of that node.  This file keeps the moves: those of the first agent whose
node wins, or, when no agent wins, those of the BFS agent (its best node: the state the statistics are taken from).  Data only:

  moves_<prob>_<file>   int8 [N, L]: for every level of stats_<prob>_<file>.npz, in its order, the index of each action in the
                        engine's `directions` (mdungeon 0..3 = left, right, up, down; ddave 0..3 = stay, left, right, jump),
                        -1 beyond the play and everywhere when the planner does not run (L = the longest of the file, at least 1)
  length_<prob>_<file>  int32 [N]: the number of moves (0 when the planner does not run)
  hand_<prob>_*         hand-made levels with more things on the floor / diamonds than the compact searches take (the generic
                        searches of csrc/mdungeon_solver.h, ddave_solver.h): hand_<prob>_map_<i> uint8 [h, w], hand_<prob>_power
                        [K], hand_<prob>_stats [K, 11] (the stats fixtures' keys), hand_<prob>_agents [K, 5] (pops of A*(1),
                        A*(0.5), A*(0), BFS; the winner, -1 = none), hand_<prob>_moves int8 [K, L], hand_<prob>_length [K]
"""
import importlib
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

FILES = {
    "mdungeon": ["1x6_p5000", "5x5_p5000", "6x9_p300", "7x11_p5000", "11x7_p1200", "11x7_p5000", "14x14_p5000"],
    "ddave": ["1x5_p5000", "2x6_p5000", "5x5_p5000", "6x9_p150", "7x11_p600", "7x11_p5000", "11x7_p5000", "14x14_p5000"],
}
CHARS = {"mdungeon": " #@H*$go", "ddave": " #@H$V*"}


def play(name, prob, m):
    """The agents in _run_game's order: (pops of each one that ran + the winner, -1 = none; the moves; the last agent's node)."""
    engine = importlib.import_module("gym_pcgrl.envs.probs.%s.engine" % name)
    chars = CHARS[name]
    rows = ["#" * (prob._width + 2)] + ["#" + "".join(chars[t] for t in r) + "#" for r in m] + ["#" * (prob._width + 2), ""]
    state = engine.State()
    state.stringInitialize(rows)
    iters, win = [0, 0, 0, 0], -1
    for a, bal in enumerate((1, 0.5, 0, None)):
        if bal is None:
            sol, node, it = engine.BFSAgent().getSolution(state, prob._solver_power)
        else:
            sol, node, it = engine.AStarAgent().getSolution(state, bal, prob._solver_power)
        iters[a] = it
        if node.checkWin():
            win = a
            break
    return iters + [win], [engine.directions.index(a) for a in sol], node


def stats_row(prob, m, keys):
    st = prob.get_stats(get_string_map(m, prob.get_tile_types()))
    return [int(st[k]) for k in keys]


def pad(rows):
    L = max([1] + [len(r) for r in rows])
    out = np.full((len(rows), L), -1, np.int8)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return out


def open_floor(h, w, thing, n, extra=()):
    """The player in the top left corner, the exit in the bottom right one, `n` things row by row from the second cell on,
    `extra` = ((row, column, tile), ...) on top."""
    m = np.zeros((h, w), np.uint8)
    cells = [(r, c) for r in range(h) for c in range(w)][1:-1]
    for r, c in cells[:n]:
        m[r, c] = thing
    m[0, 0], m[h - 1, w - 1] = 2, 3
    for r, c, t in extra:
        m[r, c] = t
    return m


# (problem, map, solver_power): 7 x 11 floors with more than 48 things; small powers keep the reference at seconds
HAND = {
    "mdungeon": [(open_floor(7, 11, 5, 50), 400), (open_floor(7, 11, 5, 50), 40), (open_floor(7, 11, 5, 52, ((6, 9, 7), (5, 10, 7), (5, 9, 7))), 300)],
    # (ddave: the player falls to the bottom row and jumps two cells high -- a key in the top row is out of reach: nobody wins)
    "ddave": [(open_floor(7, 11, 4, 50, ((6, 5, 5),)), 600), (open_floor(7, 11, 4, 50, ((6, 5, 5),)), 6), (open_floor(7, 11, 4, 60, ((0, 10, 5),)), 800)],
}


def main():
    out = {}
    for name in ("mdungeon", "ddave"):
        prob = PROBLEMS[name]()
        tally = {"win": [0, 0, 0, 0], "none": 0, "longest_win": 0, "longest_none": 0, "none_zero": 0}
        for f in FILES[name]:
            d = np.load(os.path.join(HERE, "stats_%s_%s.npz" % (name, f)))
            keys = [str(k) for k in d["keys"]]
            h, w = (int(v) for v in f.split("_")[0].split("x"))
            prob._width, prob._height, prob._solver_power = w, h, int(d["solver_power"])
            assert d["maps"].shape[1:] == (h, w) and f.endswith("_p%d" % prob._solver_power)
            t0 = time.time()
            rows = []
            for i, m in enumerate(d["maps"]):
                ag = d["agents"][i]
                if ag[4] == -2:
                    rows.append([])
                    continue
                got, sol, node = play(name, prob, m)
                assert got == ag.tolist(), (name, f, i, got, ag)
                st = dict(zip(keys, d["stats"][i].tolist()))
                if got[4] >= 0:
                    assert st["dist-win"] == 0 and st["sol-length"] == len(sol), (name, f, i)
                    tally["win"][got[4]] += 1
                    tally["longest_win"] = max(tally["longest_win"], len(sol))
                else:
                    assert st["dist-win"] == node.getHeuristic() and st["sol-length"] == 0, (name, f, i)
                    tally["none"] += 1
                    tally["longest_none"] = max(tally["longest_none"], len(sol))
                    tally["none_zero"] += len(sol) == 0
                rows.append(sol)
            out["moves_%s_%s" % (name, f)] = pad(rows)
            out["length_%s_%s" % (name, f)] = np.array([len(r) for r in rows], np.int32)
            print("  %s %s: %d levels, %.1fs" % (name, f, len(rows), time.time() - t0), flush=True)
        print("  %s: %s" % (name, tally), flush=True)
        stats, agents, moves = [], [], []
        for i, (m, power) in enumerate(HAND[name]):
            prob._width, prob._height, prob._solver_power = m.shape[1], m.shape[0], power
            t0 = time.time()
            keys = [str(k) for k in np.load(os.path.join(HERE, "stats_%s_%s.npz" % (name, FILES[name][0])))["keys"]]
            st = stats_row(prob, m, keys)
            ag, sol, node = play(name, prob, m)
            sd = dict(zip(keys, st))
            assert sd["sol-length"] == (len(sol) if ag[4] >= 0 else 0) and sd["dist-win"] == (0 if ag[4] >= 0 else node.getHeuristic())
            out["hand_%s_map_%d" % (name, i)] = m
            stats.append(st)
            agents.append(ag)
            moves.append(sol)
            print("  hand %s %d: power %d: %d moves, agents %s, stats %s, %.1fs" % (name, i, power, len(sol), ag, st, time.time() - t0), flush=True)
        out["hand_%s_power" % name] = np.array([p for (_, p) in HAND[name]], np.int64)
        out["hand_%s_stats" % name] = np.array(stats, np.int64)
        out["hand_%s_agents" % name] = np.array(agents, np.int64)
        out["hand_%s_moves" % name] = pad(moves)
        out["hand_%s_length" % name] = np.array([len(r) for r in moves], np.int32)
    np.savez_compressed(os.path.join(HERE, "playthroughs.npz"), **out)
    print("wrote playthroughs.npz")


if __name__ == "__main__":
    main()
