"""The moves behind sokoban's sol-length, without a GPU: the traced searches of gym_pcgrl_amd/csrc (SokTrace) instantiated on the CPU
(tests/hostsim/sim_solution.cpp) against the reference's get_stats(map)["solution"] (tests/golden/solutions_sokoban.npz), the host side
of pcgrl_get_solution_bytes / pcgrl_get_solution, and replay_sokoban()."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from host_kit import MOVES_PARAMS, config as _config, header, plain_header, prototype
from hostsim_build import build_so
from oracle_lib import _p

HERE = os.path.dirname(os.path.abspath(__file__))
G = os.path.join(HERE, "golden")
SIZES = ["4x6", "5x5", "5x6", "6x6", "7x7", "7x8", "8x8"]
NHAND = 4


@pytest.fixture(scope="module")
def sim():
    L = build_so("sim_solution.cpp")
    L.sim_sokoban_solution.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


@pytest.fixture(scope="module")
def sol():
    return np.load(os.path.join(G, "solutions_sokoban.npz"))


def _solve(L, m, power, fast, max_len):
    m = np.ascontiguousarray(m, np.uint8)
    moves = np.full(max_len + 2, 77, np.int8)            # two guard bytes behind the row
    length, winner = C.c_int(), C.c_int()
    it = np.zeros(4, np.int32)
    rc = L.sim_sokoban_solution(_p(m), m.shape[0], m.shape[1], power, fast, max_len, _p(moves), C.byref(length), C.byref(winner), _p(it))
    assert (moves[max_len:] == 77).all()
    return rc, moves[:max_len], length.value, winner.value, it


def _crates(m):
    return int((np.asarray(m) == 3).sum())


@pytest.mark.parametrize("fast", [1, 0], ids=["compact", "generic"])
@pytest.mark.parametrize("size", SIZES)
def test_traced_searches_vs_reference_solutions(sim, sol, size, fast):
    """Every level of the stats fixture: moves, length, winner and the pops of every agent are the reference's."""
    d = np.load(os.path.join(G, "stats_sokoban_%s.npz" % size))
    want = sol["moves_" + size]
    power = int(d["solver_power"])
    assert want.shape[0] == d["maps"].shape[0] and want.dtype == np.int8
    assert np.array_equal((want >= 0).sum(1), d["stats"][:, 5])          # the fixture itself: a row's moves are as many as sol-length
    width = want.shape[1]
    ran = solved = 0
    for i, m in enumerate(d["maps"]):
        ag = d["agents"][i]
        if ag[4] == -2:                                   # the planner does not run (sokoban_prob.py:143): no moves
            assert (want[i] == -1).all()
            continue
        rc, moves, length, winner, it = _solve(sim, m, power, fast, width)
        assert rc == 0, (size, i, rc)                    # (at most four crates in these files: the compact search takes them all)
        assert winner == ag[4] and length == d["stats"][i, 5], (size, i, winner, length, ag)
        assert np.array_equal(it, ag[:4]), (size, i, it, ag)
        assert np.array_equal(moves, want[i]), (size, i, moves, want[i])
        ran += 1
        solved += winner >= 0
    assert ran > 0 and solved == int((d["stats"][:, 5] > 0).sum()) and solved > 0
    # sok_search_fast<1> takes the levels of at most 64 bordered cells, <4> the rest: both are reached
    h, w = d["maps"].shape[1:]
    assert ((h + 2) * (w + 2) <= 64) == (size in ("4x6", "5x5", "5x6", "6x6"))


def test_fixture_covers_what_the_issue_lists(sol):
    solved = {s: int((sol["moves_" + s][:, 0] >= 0).sum()) for s in SIZES}
    assert solved == {"4x6": 9, "5x5": 43, "5x6": 30, "6x6": 10, "7x7": 3, "7x8": 9, "8x8": 11}
    assert max(int((sol["moves_" + s] >= 0).sum(1).max()) for s in SIZES) == 72
    winners = set()
    for s in SIZES:
        winners |= set(np.load(os.path.join(G, "stats_sokoban_%s.npz" % s))["agents"][:, 4].tolist())
    assert {0, 1, 2, 3} <= winners


def test_truncated_rows_are_prefixes(sim, sol):
    d = np.load(os.path.join(G, "stats_sokoban_7x8.npz"))
    want = sol["moves_7x8"]
    i = int(np.argmax((want >= 0).sum(1)))
    full = int((want[i] >= 0).sum())
    assert full == 72
    for max_len in (1, 4, full, full + 3):
        for fast in (1, 0):
            rc, moves, length, winner, _ = _solve(sim, d["maps"][i], int(d["solver_power"]), fast, max_len)
            assert rc == 0 and length == full
            assert np.array_equal(moves[:min(full, max_len)], want[i, :min(full, max_len)]) and (moves[full:] == -1).all()


def test_hand_made_levels_take_the_generic_search(sim, sol):
    """More than SOKF_MAXC crates: only the generic search takes them.  Moves, stats, winner and pops are the reference's."""
    maxc = sim.sim_sokf_maxc()
    lengths = []
    for i in range(NHAND):
        m, power = sol["hand_map_%d" % i], int(sol["hand_power"][i])
        assert _crates(m) > maxc
        st, ag, want = sol["hand_stats"][i], sol["hand_agents"][i], sol["hand_moves"][i]
        assert (st[0], st[1], st[2], st[3], st[4]) == (1, _crates(m), _crates(m), 1, 0)
        assert _solve(sim, m, power, 1, want.shape[0])[0] == -2           # the compact search refuses
        rc, moves, length, winner, it = _solve(sim, m, power, 0, want.shape[0])
        assert rc == 0 and winner == ag[4] and length == st[5] == int((want >= 0).sum())
        assert np.array_equal(it, ag[:4]) and np.array_equal(moves, want)
        lengths.append((m.shape, power, length, winner))
    assert lengths == [((8, 6), 5000, 23, 2), ((8, 6), 600, 30, 3), ((9, 6), 5000, 36, 3), ((8, 7), 5000, 52, 3)]


# ------------------------------------------------------------------ replay_sokoban: the check that needs no fixture of moves
def _all_solutions(sol):
    for s in SIZES:
        maps = np.load(os.path.join(G, "stats_sokoban_%s.npz" % s))["maps"]
        for i in np.nonzero(sol["moves_" + s][:, 0] >= 0)[0]:
            yield maps[i], sol["moves_" + s][i]
    for i in range(NHAND):
        yield sol["hand_map_%d" % i], sol["hand_moves"][i]


def test_replay_of_every_fixture_solution_wins(sol):
    from gym_pcgrl_amd import replay_sokoban
    n = 0
    for m, moves in _all_solutions(sol):
        k = int((moves >= 0).sum())
        r = replay_sokoban(m, moves)
        assert r.legal and r.won, (m, moves)
        assert r.player.shape == (k + 1, 2) and r.crates.shape == (k + 1, _crates(m), 2)
        assert np.abs(np.diff(r.player, axis=0)).sum(1).tolist() == [1] * k          # every frame is one step from the last
        short = replay_sokoban(m, moves[:k - 1])
        assert short.legal and not short.won, (m, moves)
        n += 1
    assert n == 115 + NHAND


def test_replay_rules():
    from gym_pcgrl_amd import replay_sokoban
    lv = np.array([[2, 3, 4, 0],
                   [1, 0, 0, 0]], np.uint8)
    r = replay_sokoban(lv, [1])
    assert r.legal and r.won and r.player.tolist() == [[0, 0], [0, 1]] and r.crates.tolist() == [[[0, 1]], [[0, 2]]]
    assert r.targets.tolist() == [[0, 2]]
    assert not replay_sokoban(lv, [3]).legal                        # into a wall
    assert not replay_sokoban(lv, [0]).legal and not replay_sokoban(lv, [2]).legal      # off the level: the border is solid
    assert replay_sokoban(lv, [3]).player.tolist() == [[0, 0], [0, 0]]
    r = replay_sokoban(lv, [1, 1, 1])                               # the crate ends against the border: the third move does nothing
    assert not r.legal and not r.won and r.player[-1].tolist() == [0, 2] and r.crates[-1].tolist() == [[0, 3]]
    two = np.array([[2, 3, 3, 0]], np.uint8)
    assert not replay_sokoban(two, [1]).legal                       # a crate behind the crate
    assert replay_sokoban(lv, [1, -1, 1]).player.shape[0] == 2      # a negative entry ends the list
    assert replay_sokoban(lv, []).legal and not replay_sokoban(lv, []).won
    with pytest.raises(ValueError):
        replay_sokoban(lv, [4])
    with pytest.raises(ValueError):
        replay_sokoban(np.zeros((3, 3), np.uint8), [0])


# ------------------------------------------------------------------ the ABI, without a device
def _bytes(cfg, count, max_len):
    from gym_pcgrl_amd import _lib
    return int(_lib.load().pcgrl_get_solution_bytes(C.byref(cfg), count, max_len))


def test_declared_exported_and_mirrored():
    from gym_pcgrl_amd import _lib
    hdr, plain = header(), plain_header()
    assert re.search(prototype("size_t", "pcgrl_get_solution_bytes", ["const pcgrl_config*", "int32_t", "int32_t"]), plain)
    assert re.search(prototype("int", "pcgrl_get_solution", MOVES_PARAMS), plain)
    for cited in ("sokoban_prob.py:133-145", "engine.py:38-44", "Still 15: + pcgrl_get_solution_bytes / pcgrl_get_solution"):
        assert cited in hdr, cited
    L = _lib.load()
    for name in ("pcgrl_get_solution_bytes", "pcgrl_get_solution"):
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert L.pcgrl_abi_version() == _lib.ABI_VERSION == 15
    assert L.pcgrl_get_solution_bytes.argtypes == [C.POINTER(_lib.Config), C.c_int32, C.c_int32] and L.pcgrl_get_solution_bytes.restype == C.c_size_t
    assert len(L.pcgrl_get_solution.argtypes) == 11
    # refused without a handle, not crashed
    assert L.pcgrl_get_solution(None, None, 1, 1, None, None, None, None, None, 0, None) == _lib.PCGRL_ESTATE


def test_workspace_sizes():
    sok = _config("sokoban", 5, 5)
    for prob in ("binary", "zelda", "mdungeon", "ddave", "smb"):
        assert _bytes(_config(prob, 5, 5), 64, 16) == 0, prob
    assert _bytes(_config("sokoban", 16, 24), 64, 16) == 0           # 18 x 26 bordered cells > 256
    assert _bytes(_config("sokoban", 5, 5, 5001), 64, 16) == 0       # beyond the searches that run in LDS
    assert _bytes(sok, 64, 0) == 0 and _bytes(sok, 64, -1) == 0 and _bytes(sok, 0, 16) == 0
    from gym_pcgrl_amd import _lib
    assert int(_lib.load().pcgrl_get_solution_bytes(None, 4, 4)) == 0
    last = 0
    for count in (1, 63, 64, 65, 129, 4096, 65536):
        sizes = [_bytes(sok, count, ml) for ml in (1, 4, 72, 255, 5000)]
        assert sizes[0] >= 256 and sizes == sorted(sizes), (count, sizes)
        assert sizes[0] >= last
        assert sizes[0] >= int(_lib.load().pcgrl_get_stats_bytes(C.byref(sok), count))
        last = sizes[0]
    assert _bytes(_config("sokoban", 14, 14), 10, 10) >= 256         # 16 x 16 = 256 bordered cells: the last size with the form
    # the exact values, recorded from the library as it was before solve() and playthrough() came to share one plan
    for cfg in (sok, _config("sokoban", 14, 14)):
        for count, want in zip((1, 63, 64, 65, 129, 4096, 65536), (801024, 802816, 802816, 1603584, 2406144, 51364096, 207225088)):
            assert _bytes(cfg, count, 1) == want and _bytes(cfg, count, 255) == want, (count, want)
