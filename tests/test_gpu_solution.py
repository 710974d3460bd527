"""BatchedPcgrlEnv.solve() / pcgrl_get_solution on the GPU: the moves of sokoban's planner, bit for bit against the reference's
get_stats(map)["solution"] (tests/golden/solutions_sokoban.npz), replayed by the game's rules (replay_sokoban), and without a trace on
the handle that computed them.  Every case uses a handle of THREE environments and solves another number of levels."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import readout_harness as rh
from readout_harness import N_ENVS, make_env, padded as _padded, torch as _torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
G = os.path.join(HERE, "golden")
SIZES = ["4x6", "5x5", "5x6", "6x6", "7x7", "7x8", "8x8"]
CSRC = os.path.join(os.path.dirname(HERE), "gym_pcgrl_amd", "csrc")
# what a small-region try may pop per agent
SMALL_POPS = int(re.search(r"#define SS_SMALL_POPS (\d+)", open(os.path.join(CSRC, "kernels_step_solver.h")).read()).group(1))


_CACHE = {}


def _fixture(size):
    """(maps, stats, agents, power, moves) of one size: loaded once; the tests copy what they change."""
    if size not in _CACHE:
        d = np.load(os.path.join(G, "stats_sokoban_%s.npz" % size))
        s = np.load(os.path.join(G, "solutions_sokoban.npz"))
        _CACHE[size] = (d["maps"], d["stats"], d["agents"], int(d["solver_power"]), s["moves_" + size])
    return _CACHE[size]


def _check(env, maps, stats, agents, want, max_len=None, sol=None):
    """solve(maps) against the fixture rows of the same levels; returns the Solutions."""
    torch = _torch()
    sol = env.solve(maps, max_len=max_len) if sol is None else sol
    M = maps.shape[0]
    ml = sol.moves.shape[1]
    assert sol.moves.dtype == torch.int8 and sol.length.dtype == torch.int32 and sol.agent.dtype == torch.int8
    assert tuple(sol.moves.shape) == (M, ml) and tuple(sol.length.shape) == (M,) and tuple(sol.agent.shape) == (M,) and tuple(sol.rows.shape) == (M, 8)
    moves, length, agent = sol.moves.cpu().numpy(), sol.length.cpu().numpy(), sol.agent.cpu().numpy()
    assert env.check_status() == 0
    assert np.array_equal(length, stats[:, 5]), np.nonzero(length != stats[:, 5])[0][:5]
    assert np.array_equal(agent, agents[:, 4]), np.nonzero(agent != agents[:, 4])[0][:5]
    exp = _padded(want, ml)
    bad = np.nonzero((moves != exp).any(1))[0]
    assert bad.size == 0, (bad[:5], moves[bad[:1]], exp[bad[:1]])
    assert np.array_equal(sol.truncated.cpu().numpy(), stats[:, 5] > ml)
    assert np.array_equal(sol.stats.cpu().numpy().astype(np.int64), stats)
    return sol


def _replay_all(maps, moves, length):
    """Every solved level's moves, by the game's rules: legal, and a win in exactly `length` moves."""
    from gym_pcgrl_amd import replay_sokoban
    n = 0
    for i in np.nonzero(length > 0)[0]:
        assert length[i] <= moves.shape[1]
        assert int((moves[i] >= 0).sum()) == length[i] and (moves[i, :length[i]] >= 0).all()
        r = replay_sokoban(maps[i], moves[i])
        assert r.legal and r.won and r.player.shape[0] == length[i] + 1, i
        assert not replay_sokoban(maps[i], moves[i, :length[i] - 1]).won, i
        n += 1
    return n


# ------------------------------------------------------------------ every fixture level
@pytest.mark.parametrize("tuning", [None, {"sok_generic": 1}], ids=["default", "generic"])
@pytest.mark.parametrize("size", SIZES)
def test_fixture_solutions(size, tuning):
    torch = _torch()
    maps, stats, agents, power, want = _fixture(size)
    assert maps.shape[0] != N_ENVS and maps.shape[0] <= 412
    env = make_env("sokoban", maps.shape[1], maps.shape[2], power, tuning=tuning)
    sol = _check(env, maps, stats, agents, want, max_len=want.shape[1])
    assert torch.equal(sol.rows, env.evaluate(maps).rows)
    assert _replay_all(maps, sol.moves.cpu().numpy(), sol.length.cpu().numpy()) == int((stats[:, 5] > 0).sum()) > 0
    env.close()


def test_hand_made_levels_reach_the_generic_search():
    _torch()
    src = open(os.path.join(CSRC, "sokoban_fast.h")).read()
    maxc = int(re.search(r"#define SOKF_MAXC (\d+)", src).group(1))
    s = np.load(os.path.join(G, "solutions_sokoban.npz"))
    for i in range(4):
        m, power = s["hand_map_%d" % i], int(s["hand_power"][i])
        assert int((m == 3).sum()) > maxc                           # more crates than the compact search takes
        st, ag, want = s["hand_stats"][i:i + 1], s["hand_agents"][i:i + 1], s["hand_moves"][i:i + 1]
        assert st[0, 5] > 0 and ag[0, 4] >= 2                        # solved, by a later agent
        env = make_env("sokoban", m.shape[0], m.shape[1], power)
        sol = _check(env, m[None], st, ag, want, max_len=want.shape[1])
        assert _replay_all(m[None], sol.moves.cpu().numpy(), sol.length.cpu().numpy()) == 1
        env.close()


def test_full_region_redo():
    """Levels on which an agent needed more than SS_SMALL_POPS pops before the game ended: the small-region try is "not final" and
    contributes nothing; wavefront 0 redoes them with the full solver_power, and the moves are that run's."""
    _torch()
    total = solved = 0
    for size in SIZES:
        maps, stats, agents, power, want = _fixture(size)
        pick = np.nonzero((agents[:, :4].max(1) > SMALL_POPS) & (agents[:, 4] > -2))[0]
        if pick.size == 0:
            continue
        env = make_env("sokoban", maps.shape[1], maps.shape[2], power)
        sol = _check(env, maps[pick], stats[pick], agents[pick], want[pick], max_len=want.shape[1])
        solved += _replay_all(maps[pick], sol.moves.cpu().numpy(), sol.length.cpu().numpy())
        total += pick.size
        env.close()
    assert total > 0 and solved > 0, (total, solved)


@pytest.mark.parametrize("count", [1, 63, 64, 65, 129])
def test_chunk_and_ticket_edges(count):
    """EVAL_CHUNK = 64 jobs a ticket: counts around it, with solved, unsolved and planner-not-run levels mixed."""
    _torch()
    maps, stats, agents, power, want = _fixture("5x5")
    order = np.random.RandomState(5).permutation(maps.shape[0])
    first = int(np.nonzero(stats[order, 5] > 0)[0][0])
    order = np.concatenate([order[first:first + 1], np.delete(order, first)])           # (a solved level first: count = 1 has moves)
    pick = order[:count]
    if count > 1:
        assert (agents[pick, 4] == -2).any() and (agents[pick, 4] == -1).any() and (agents[pick, 4] >= 0).any()
    env = make_env("sokoban", 5, 5, power)
    sol = _check(env, maps[pick], stats[pick], agents[pick], want[pick])
    assert sol.moves.shape[1] == 255                                                    # the default: min(solver_power, 255)
    assert (stats[pick, 5] > 0).any()
    env.close()


@pytest.mark.parametrize("max_len", [1, 4, 72])
def test_max_len_and_row_bounds(max_len):
    """Rows shorter than the solutions: the full length, the prefix, `truncated`; and through the C entry point nothing is written
    outside [count, max_len] -- guard rows of a known byte on both sides of the outputs stay intact."""
    torch = _torch()
    maps, stats, agents, power, want = _fixture("7x8")
    assert int(stats[:, 5].max()) == 72
    env = make_env("sokoban", 7, 8, power)
    sol = _check(env, maps, stats, agents, want, max_len=max_len)
    assert sol.truncated.any().item() == (max_len < 72)
    M, dev, lib = maps.shape[0], env.device, env._lib
    mv, ln, ag = rh.Guarded(torch.int8, M * max_len, dev), rh.Guarded(torch.int32, M, dev), rh.Guarded(torch.int8, M, dev)
    m = torch.as_tensor(np.ascontiguousarray(maps)).to(dev)
    cfg = env._config()
    need = int(lib.pcgrl_get_solution_bytes(C.byref(cfg), M, max_len))
    assert need >= 256
    work = torch.empty((need,), dtype=torch.uint8, device=dev)
    rh.guarded_call((mv, ln, ag), lambda a, b, c: lib.pcgrl_get_solution(env._handle, rh.ptr(m), M, max_len, a, b, c, None, rh.ptr(work), need, env._stream()))      # (no rows wanted)
    assert torch.equal(mv.inner.view(M, max_len), sol.moves) and torch.equal(ln.inner, sol.length) and torch.equal(ag.inner, sol.agent)
    # refusals: a workspace one byte short, max_len 0
    assert lib.pcgrl_get_solution(env._handle, rh.ptr(m), M, max_len, mv.ptr, ln.ptr, None, None, rh.ptr(work), need - 1, env._stream()) == -1
    assert lib.pcgrl_get_solution(env._handle, rh.ptr(m), M, 0, mv.ptr, ln.ptr, None, None, rh.ptr(work), need, env._stream()) == -1
    env.close()


# ------------------------------------------------------------------ the handle is left alone
def test_handle_in_the_middle_of_its_episodes():
    from gym_pcgrl_amd.envs import BatchedPcgrlEnv
    maps, stats, agents, power, want = _fixture("5x5")

    def after_own(env, own):
        assert own.moves.shape == (N_ENVS, 255)

    rh.check_handle_left_alone(lambda: BatchedPcgrlEnv(prob="sokoban", rep="narrow", num_envs=N_ENVS, seed=77),
                               lambda env: np.random.RandomState(3).randint(0, 6, size=(40, N_ENVS)).astype(np.int32),
                               lambda env, *m: env.solve(*m), ("moves", "length", "agent", "rows"),
                               lambda env: ("map", "stats", "start_stats", "counters", "heatmap", "pos"), after_own,
                               lambda env: _check(env, maps[:9], stats[:9], agents[:9], want[:9]))


def test_solve_leaves_pending_searches_alone():
    torch = _torch()
    import oracle_lib as ol
    from gym_pcgrl_amd.envs import BatchedPcgrlEnv
    maps, stats, agents, power, want = _fixture("5x5")
    picks = []
    for m in maps:                                                # a wall cell turned into floor leaves the solver dozens of pops
        for y, x in zip(*np.nonzero(m == 1)):
            b = m.copy()
            b[y, x] = 0
            if int(ol.get_stats("sokoban", b, with_iters=True)[1].max()) >= 40:
                picks.append((m, (int(x), int(y), 0)))
                break
        if len(picks) == N_ENVS:
            break
    assert len(picks) == N_ENVS
    env = BatchedPcgrlEnv(prob="sokoban", rep="wide", num_envs=N_ENVS, seed=11)
    assert env.enable_async(nslots=8)
    env.reset()
    env.set_maps(np.stack([m for m, _ in picks]))
    *_, pending = env.tick(np.array([a for _, a in picks], np.int32), pop_budget=1)       # one pop: every search is suspended
    before_p, before_c = pending.clone(), env._async["counters"].clone()
    sol = env.solve(maps[:7])                                                          # ... with the tick's searches in flight
    torch.cuda.synchronize()
    assert before_p.any() and env.async_counters()["suspended"] > 0
    assert np.array_equal(sol.moves.cpu().numpy(), _padded(want[:7], 255)) and np.array_equal(sol.length.cpu().numpy(), stats[:7, 5])
    assert torch.equal(env._async["pending"], before_p) and torch.equal(env._async["counters"], before_c)
    for _ in range(200):                                                               # the suspended steps still complete
        *_, pending = env.tick(np.array([a for _, a in picks], np.int32), pop_budget=4096)
        if not pending.any():
            break
    assert not pending.any()
    assert env.check_status() == 0
    env.close()


def test_bad_tile_is_clamped_and_reported():
    maps, stats, agents, power, want = _fixture("5x5")
    env = make_env("sokoban", 5, 5, power)
    rh.check_bad_tile(env, env.solve, ("moves", "length", "agent", "rows"), maps[:40], [(i, i % 5, (2 * i) % 5) for i in range(5)])
    env.close()


def test_configurations_without_the_form():
    _torch()
    import gym_pcgrl_amd
    for kw in (dict(prob="mdungeon", h=5, w=5), dict(prob="sokoban", h=16, w=24, power=2500), dict(prob="sokoban", h=5, w=5, power=5001)):
        env = make_env(**kw)
        with pytest.raises(NotImplementedError):
            env.solve(np.zeros((2, kw["h"], kw["w"]), np.uint8))
        env.close()
    env = make_env("sokoban", 5, 5)
    with pytest.raises(ValueError):
        env.solve(np.zeros((2, 5, 6), np.uint8))
    with pytest.raises(ValueError):
        env.solve(np.zeros((5, 5), np.uint8))
    with pytest.raises(ValueError):
        env.solve(np.zeros((2, 5, 5), np.uint8), max_len=0)
    env.close()
    maps, stats, agents, power, want = _fixture("4x6")               # the one-call form, with adjust_param's keys
    sol = gym_pcgrl_amd.solve_levels("sokoban", maps, solver_power=power, max_len=want.shape[1])
    assert np.array_equal(sol.moves.cpu().numpy(), want) and np.array_equal(sol.length.cpu().numpy(), stats[:, 5])
    assert np.array_equal(sol.agent.cpu().numpy(), agents[:, 4])
