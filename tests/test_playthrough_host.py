"""The play behind the mdungeon / ddave statistics, without a GPU: the traced searches of gym_pcgrl_amd/csrc (PlayTrace) instantiated
on the CPU (tests/hostsim/sim_playthrough.cpp) against the reference's agents' moves (tests/golden/playthroughs.npz), the host replays
replay_mdungeon() / replay_ddave(), and the host side of pcgrl_get_playthrough_bytes / pcgrl_get_playthrough."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from host_kit import MOVES_PARAMS, config as _config, header, plain_header, prototype, run_sanitized
from hostsim_build import build_so
from oracle_lib import _p

HERE = os.path.dirname(os.path.abspath(__file__))
G = os.path.join(HERE, "golden")
FILES = {
    "mdungeon": ["1x6_p5000", "5x5_p5000", "6x9_p300", "7x11_p5000", "11x7_p1200", "11x7_p5000", "14x14_p5000"],
    "ddave": ["1x5_p5000", "2x6_p5000", "5x5_p5000", "6x9_p150", "7x11_p600", "7x11_p5000", "11x7_p5000", "14x14_p5000"],
}
CASES = [(p, f) for p in ("mdungeon", "ddave") for f in FILES[p]]
PROB_ID = {"mdungeon": 0, "ddave": 1}
NHAND = 3
# the planner's columns of a stats fixture row, in the order of the simulator's res[]
RES_COLS = {"mdungeon": [9, 10, 6, 7, 8], "ddave": [9, 10, 7, 8]}


@pytest.fixture(scope="module")
def sim():
    L = build_so("sim_playthrough.cpp")
    L.sim_playthrough.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.sim_play_things.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int]
    return L


@pytest.fixture(scope="module")
def play():
    return np.load(os.path.join(G, "playthroughs.npz"))


def _run(L, prob, m, power, fast, max_len):
    m = np.ascontiguousarray(m, np.uint8)
    moves = np.full(max_len + 2, 77, np.int8)            # two guard bytes behind the row
    length, winner = C.c_int(), C.c_int()
    it, res = np.zeros(4, np.int32), np.zeros(5, np.int32)
    rc = L.sim_playthrough(PROB_ID[prob], _p(m), m.shape[0], m.shape[1], power, fast, max_len, _p(moves), C.byref(length), C.byref(winner), _p(it), _p(res))
    assert (moves[max_len:] == 77).all()
    return rc, moves[:max_len], length.value, winner.value, it, res


@pytest.mark.parametrize("fast", [1, 0], ids=["compact", "generic"])
@pytest.mark.parametrize("prob,name", CASES, ids=["%s_%s" % c for c in CASES])
def test_traced_searches_vs_reference_plays(sim, play, prob, name, fast):
    """Every level of the stats fixture: moves, length, winner, the planner's columns and the pops of every agent are the
    reference's -- with the compact and with the generic search."""
    d = np.load(os.path.join(G, "stats_%s_%s.npz" % (prob, name)))
    want, wlen = play["moves_%s_%s" % (prob, name)], play["length_%s_%s" % (prob, name)]
    power = int(d["solver_power"])
    assert want.shape[0] == d["maps"].shape[0] and want.dtype == np.int8 and wlen.dtype == np.int32
    assert np.array_equal((want >= 0).sum(1), wlen)
    width = want.shape[1]
    cols = RES_COLS[prob]
    ran = 0
    for i, m in enumerate(d["maps"]):
        ag = d["agents"][i]
        if ag[4] == -2:                                   # the planner does not run: no moves
            assert (want[i] == -1).all() and wlen[i] == 0
            continue
        rc, moves, length, winner, it, res = _run(sim, prob, m, power, fast, width)
        assert rc == 0, (name, i, rc)                    # (no level of these files has more than 48 things: the compact search takes them all)
        assert winner == ag[4] and length == wlen[i], (name, i, winner, length, ag)
        assert np.array_equal(it, ag[:4]), (name, i, it, ag)
        assert np.array_equal(moves, want[i]), (name, i, moves, want[i])
        assert res[:len(cols)].tolist() == d["stats"][i, cols].tolist(), (name, i, res)
        if winner >= 0:
            assert length == d["stats"][i, 10]
        ran += 1
    assert ran > 0


def test_fixture_covers_what_the_issue_lists(sim, play):
    for prob, winners, nobody, longest_win, longest_none, none_zero in (("mdungeon", [425, 1, 2, 6], 35, 56, 16, 7),
                                                                        ("ddave", [157, 2, 3, 0], 340, 36, 30, 23)):
        ag = np.concatenate([np.load(os.path.join(G, "stats_%s_%s.npz" % (prob, f)))["agents"][:, 4] for f in FILES[prob]])
        ln = np.concatenate([play["length_%s_%s" % (prob, f)] for f in FILES[prob]])
        assert [int((ag == a).sum()) for a in range(4)] == winners
        assert int((ag == -1).sum()) == nobody
        assert int(ln[ag >= 0].max()) == longest_win and int(ln[ag == -1].max()) == longest_none
        assert int((ln[ag == -1] == 0).sum()) == none_zero
        assert (ln[ag == -2] == 0).all()
    # (no ddave level of these files is won by BFS -- the 0 above; its no-win rows walk the BFS agent's pool all the same)
    assert int(play["length_mdungeon_11x7_p5000"].max()) == 56 and int(play["length_ddave_7x11_p5000"].max()) == 36
    # the hand-made levels are beyond the compact searches, and each problem has one with a winner and one without
    for prob, limit in (("mdungeon", sim.sim_mdf_maxi()), ("ddave", sim.sim_ddf_maxd())):
        assert limit == 48
        won = []
        for i in range(NHAND):
            m = np.ascontiguousarray(play["hand_%s_map_%d" % (prob, i)])
            assert sim.sim_play_things(PROB_ID[prob], _p(m), m.shape[0], m.shape[1]) > limit
            won.append(int(play["hand_%s_agents" % prob][i, 4]))
        assert max(won) >= 0 and min(won) == -1, won


@pytest.mark.parametrize("prob", ["mdungeon", "ddave"])
def test_hand_made_levels_take_the_generic_search(sim, play, prob):
    """More than MDF_MAXI things / DDF_MAXD diamonds: only the generic search takes them.  Moves, stats, winner and pops are the reference's."""
    cols = RES_COLS[prob]
    for i in range(NHAND):
        m, power = play["hand_%s_map_%d" % (prob, i)], int(play["hand_%s_power" % prob][i])
        st, ag, want = play["hand_%s_stats" % prob][i], play["hand_%s_agents" % prob][i], play["hand_%s_moves" % prob][i]
        assert _run(sim, prob, m, power, 1, want.shape[0])[0] == -2           # the compact search refuses
        rc, moves, length, winner, it, res = _run(sim, prob, m, power, 0, want.shape[0])
        assert rc == 0 and winner == ag[4] and length == play["hand_%s_length" % prob][i] == int((want >= 0).sum())
        assert np.array_equal(it, ag[:4]) and np.array_equal(moves, want)
        assert res[:len(cols)].tolist() == st[cols].tolist()


def test_truncated_rows_are_prefixes(sim, play):
    d = np.load(os.path.join(G, "stats_mdungeon_11x7_p5000.npz"))
    want = play["moves_mdungeon_11x7_p5000"]
    i = int(np.argmax(play["length_mdungeon_11x7_p5000"]))
    full = int((want[i] >= 0).sum())
    assert full == 56
    for max_len in (1, 4, full, full + 3):
        for fast in (1, 0):
            rc, moves, length, winner, _, _ = _run(sim, "mdungeon", d["maps"][i], int(d["solver_power"]), fast, max_len)
            assert rc == 0 and length == full
            assert np.array_equal(moves[:min(full, max_len)], want[i, :min(full, max_len)]) and (moves[full:] == -1).all()
    # a play that nobody won (BFS's best node), truncated the same way
    d = np.load(os.path.join(G, "stats_ddave_7x11_p5000.npz"))
    want, ln = play["moves_ddave_7x11_p5000"], play["length_ddave_7x11_p5000"]
    i = int(np.argmax(np.where(d["agents"][:, 4] == -1, ln, -1)))
    full = int(ln[i])
    assert full == 30
    for max_len in (1, 4, full, full + 3):
        for fast in (1, 0):
            rc, moves, length, winner, _, _ = _run(sim, "ddave", d["maps"][i], int(d["solver_power"]), fast, max_len)
            assert rc == 0 and length == full and winner == -1
            assert np.array_equal(moves[:min(full, max_len)], want[i, :min(full, max_len)]) and (moves[full:] == -1).all()


def test_sanitized_stand_alone_program():
    """sim_playthrough.cpp with its own main(), built with the address and undefined-behaviour sanitizers and run as a program: a
    handful of built-in levels through every traced search and walk-back."""
    run_sanitized("sim_playthrough.cpp", "SIM_PLAYTHROUGH_MAIN", 120)


# ------------------------------------------------------------------ the host replays: the check that owes nothing to a fixture of moves
def _all_plays(play, prob):
    for f in FILES[prob]:
        d = np.load(os.path.join(G, "stats_%s_%s.npz" % (prob, f)))
        for i in np.nonzero(d["agents"][:, 4] > -2)[0]:
            yield d["maps"][i], play["moves_%s_%s" % (prob, f)][i], int(d["agents"][i, 4]), d["stats"][i]
    for i in range(NHAND):
        yield play["hand_%s_map_%d" % (prob, i)], play["hand_%s_moves" % prob][i], int(play["hand_%s_agents" % prob][i, 4]), play["hand_%s_stats" % prob][i]


def test_replay_mdungeon_of_every_fixture_play(play):
    from gym_pcgrl_amd import replay_mdungeon
    n = 0
    for m, moves, winner, st in _all_plays(play, "mdungeon"):
        k = int((moves >= 0).sum())
        r = replay_mdungeon(m, moves)
        assert r.player.shape == (k + 1, 2) and r.health.shape == (k + 1,)
        assert r.won == (winner >= 0) and not r.dead, (m, moves)
        assert (r.potions[-1], r.treasures[-1], r.enemies[-1]) == (st[6], st[7], st[8]), (m, moves)
        if winner >= 0:
            assert k == st[10] and k > 0 and not replay_mdungeon(m, moves[:k - 1]).won          # not before the last move
        else:
            assert r.heuristic == st[9] and st[10] == 0
        n += 1
    assert n == 469 + NHAND


def test_replay_ddave_of_every_fixture_play(play):
    from gym_pcgrl_amd import replay_ddave
    n = 0
    for m, moves, winner, st in _all_plays(play, "ddave"):
        k = int((moves >= 0).sum())
        r = replay_ddave(m, moves)
        assert r.player.shape == (k + 1, 2) and r.air.shape == (k + 1,)
        assert r.won == (winner >= 0) and not r.dead, (m, moves)
        assert (r.jumps[-1], r.diamonds[-1]) == (st[7], st[8]), (m, moves)
        if winner >= 0:
            assert k == st[10] and k > 0 and r.has_key[-1] == 1 and not replay_ddave(m, moves[:k - 1]).won
        else:
            assert r.heuristic == st[9] and st[10] == 0
        n += 1
    assert n == 502 + NHAND


def test_replay_rules():
    from gym_pcgrl_amd import replay_ddave, replay_mdungeon
    lv = np.array([[2, 4, 6, 7, 5, 3],
                   [1, 0, 0, 0, 0, 0]], np.uint8)
    r = replay_mdungeon(lv, [1, 1, 1, 1, 1])
    assert r.won and not r.dead and r.health.tolist() == [5, 5, 4, 2, 2, 2] and r.potions[-1] == 1 and r.enemies[-1] == 2 and r.treasures[-1] == 1
    assert r.player[-1].tolist() == [0, 5] and r.heuristic == 0 + 4 * 3 - 4
    assert replay_mdungeon(lv, [0]).player.tolist() == [[0, 0], [0, 0]]              # off the level: the border is solid
    assert replay_mdungeon(lv, [3]).player.tolist() == [[0, 0], [0, 0]]              # into a wall
    assert replay_mdungeon(lv, [1, -1, 1]).player.shape[0] == 2                      # a negative entry ends the list
    assert replay_mdungeon(lv, [1, 1, 1, 1, 1, 0]).player[-1].tolist() == [0, 5]     # nothing moves once the game is over
    dead = np.array([[2, 7, 7, 7, 0, 3]], np.uint8)
    r = replay_mdungeon(dead, [1, 1, 1, 1])
    assert r.dead and not r.won and r.health.tolist() == [5, 3, 1, 0, 0] and r.player[-1].tolist() == [0, 3]
    with pytest.raises(ValueError):
        replay_mdungeon(lv, [4])
    with pytest.raises(ValueError):
        replay_mdungeon(np.zeros((3, 3), np.uint8), [0])
    dd = np.array([[0, 0, 4, 0, 0],
                   [2, 0, 1, 5, 3]], np.uint8)
    r = replay_ddave(dd, [3, 2, 2, 2, 0, 2])
    # a jump from the bottom row: up, (blocked by the level's top: air time 1) hover over the block, pick the diamond, fall onto the key
    assert r.jumps[-1] == 1 and r.diamonds[-1] == 1 and r.has_key[-1] == 1 and r.won and not r.dead, (r.player, r.air)
    assert replay_ddave(dd, [1]).player.tolist() == [[1, 0], [1, 0]]
    spikes = np.array([[2, 6, 5, 3]], np.uint8)
    r = replay_ddave(spikes, [2, 2])
    assert r.dead and not r.won and r.player[-1].tolist() == [0, 1]
    with pytest.raises(ValueError):
        replay_ddave(dd, [7])
    with pytest.raises(ValueError):
        replay_ddave(np.array([[2, 3]], np.uint8), [0])            # no key


# ------------------------------------------------------------------ the ABI, without a device
def _bytes(cfg, count, max_len):
    from gym_pcgrl_amd import _lib
    return int(_lib.load().pcgrl_get_playthrough_bytes(C.byref(cfg), count, max_len))


def test_declared_exported_and_mirrored():
    from gym_pcgrl_amd import _lib
    hdr, plain = header(), plain_header()
    assert re.search(prototype("size_t", "pcgrl_get_playthrough_bytes", ["const pcgrl_config*", "int32_t", "int32_t"]), plain)
    assert re.search(prototype("int", "pcgrl_get_playthrough", MOVES_PARAMS), plain)
    for cited in ("mdungeon_prob.py:100-138", "ddave_prob.py:92-127", "engine.py:43-49", "Still 15: + pcgrl_get_solution_bytes / pcgrl_get_solution",
                  "Still 15: + pcgrl_get_playthrough_bytes / pcgrl_get_playthrough"):
        assert cited in hdr, cited
    L = _lib.load()
    for name in ("pcgrl_get_playthrough_bytes", "pcgrl_get_playthrough"):
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert L.pcgrl_abi_version() == _lib.ABI_VERSION == 15
    assert L.pcgrl_get_playthrough_bytes.argtypes == [C.POINTER(_lib.Config), C.c_int32, C.c_int32] and L.pcgrl_get_playthrough_bytes.restype == C.c_size_t
    assert len(L.pcgrl_get_playthrough.argtypes) == 11
    # refused without a handle, not crashed
    assert L.pcgrl_get_playthrough(None, None, 1, 1, None, None, None, None, None, 0, None) == _lib.PCGRL_ESTATE


@pytest.mark.parametrize("prob", ["mdungeon", "ddave"])
def test_workspace_sizes(prob):
    from gym_pcgrl_amd import _lib
    L = _lib.load()
    for other in ("binary", "zelda", "sokoban", "smb"):
        assert _bytes(_config(other, 5, 5), 64, 16) == 0, other
    assert _bytes(_config(prob, 16, 24), 64, 16) == 0                # 18 x 26 bordered cells > 256
    assert _bytes(_config(prob, 5, 5, 5001), 64, 16) == 0            # beyond the searches that run in LDS
    cfg = _config(prob, 5, 5)
    assert _bytes(cfg, 64, 0) == 0 and _bytes(cfg, 64, -1) == 0 and _bytes(cfg, 0, 16) == 0
    assert int(L.pcgrl_get_playthrough_bytes(None, 4, 4)) == 0
    last = 0
    for count in (1, 63, 64, 65, 129, 4096, 65536):
        sizes = [_bytes(cfg, count, ml) for ml in (1, 4, 72, 255, 5000)]
        assert sizes[0] >= 256 and sizes == sorted(sizes), (count, sizes)
        assert sizes[0] >= last
        assert sizes[0] >= int(L.pcgrl_get_stats_bytes(C.byref(cfg), count))
        last = sizes[0]
    assert _bytes(_config(prob, 14, 14), 10, 10) >= 256              # 16 x 16 = 256 bordered cells: the last size with the form
    # the exact values (the same for both problems), recorded from the library as it was before solve() and playthrough() came to
    # share one plan
    for c in (cfg, _config(prob, 14, 14)):
        for count, want in zip((1, 63, 64, 65, 129, 4096, 65536), (881152, 882944, 882944, 1763840, 2646528, 56492288, 227737856)):
            assert _bytes(c, count, 1) == want and _bytes(c, count, 255) == want, (count, want)
