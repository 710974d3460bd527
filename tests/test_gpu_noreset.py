"""Stepping past done (auto_reset=False), against the CPU oracle stepped without reset().

The reference's PcgrlEnv goes on stepping after `done` (pcgrl_env.py:130-150): the map keeps changing, the counters keep
counting and the float64 heat map keeps growing.  The facade PcgrlEnv and every batched handle made with auto_reset=False do
the same; these tests run that on every problem and on the kernels a configuration takes (fused-size maps, 64-bit rows, tall
maps, maps beyond 64 x 64, the search problems' compact and general searches), with small change budgets so that most
environments spend most steps past done, next to ones that are not done yet in the same blocks.  Nothing here reads the
reference."""
import os

import numpy as np
import pytest

import oracle_lib as ol
import parity_harness as ph

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


SOKOBAN_OPEN = {"empty": 0.93, "solid": 0.04, "player": 0.003, "crate": 0.003, "target": 0.003}
NORESET_CASES = [
    ("binary", "narrow", (dict(change_percentage=0.05),), 64, 120),
    ("binary", "wide", (dict(change_percentage=0.05),), 64, 120),
    ("binary", "turtle", (dict(change_percentage=0.05),), 64, 120),
    ("binary", "narrow", (dict(width=33, height=14), dict(change_percentage=0.03)), 64, 100),      # 64-bit rows
    ("binary", "wide", (dict(width=20, height=30), dict(change_percentage=0.01)), 64, 100),        # tall: k_stats_wide
    ("zelda", "wide", (dict(width=11, height=16), dict(change_percentage=0.03)), 64, 100),
    ("zelda", "narrow", (dict(change_percentage=0.03),), 64, 100),
    ("sokoban", "narrow", (dict(change_percentage=0.1),), 64, 80),
    ("mdungeon", "narrow", (dict(change_percentage=0.05),), 64, 80),
    ("ddave", "narrow", (dict(change_percentage=0.05),), 64, 80),
    ("smb", "narrow", (dict(change_percentage=0.01),), 64, 40),
    ("binary", "narrow", (dict(width=90, height=70), dict(change_percentage=0.002)), 64, 60),      # beyond 64 x 64: k_big
    ("sokoban", "narrow", (dict(width=20, height=20), dict(change_percentage=0.02, solver_power=300, probs=SOKOBAN_OPEN)), 64, 60),  # search_big.h
]
_ids = lambda v: str(v) if isinstance(v, (str, int)) else "cfg"


@pytest.mark.parametrize("how", ["step", "rollout"])
@pytest.mark.parametrize("prob,rep,calls,E,T", NORESET_CASES, ids=_ids)
def test_past_done_vs_oracle(prob, rep, calls, E, T, how):
    """Every step (step()) or the whole tape (rollout()) of a batch without auto-reset against the oracle without reset(): reward,
    done, every info key, iterations and changes at every step; with step() also the map, the cursor and the heat map as exact
    counts at every step; with rollout() the map, cursor and heat map the tape ends in."""
    _torch()
    err = ph.run_config(prob, rep, list(calls), E, T, 9001, np.random.RandomState(21), use_rollout=how == "rollout",
                        auto_reset=False, map_every=1)
    assert err is None, err


@pytest.mark.parametrize("prob,calls", [("sokoban", ()), ("mdungeon", ()), ("ddave", ())], ids=_ids)
def test_past_done_async_ticks_vs_oracle(prob, calls):
    """Asynchronous ticks (pcgrl_step_async) with a pop budget of 4 on a batch without auto-reset: per environment the sequence of
    taken actions -> completed steps must be the oracle's, stepped past done without reset()."""
    _torch()
    cnt = ph.async_case(prob, "narrow", [dict(change_percentage=0.1)] + list(calls), 64, 60, 3131, np.random.RandomState(4), 4, 64,
                        auto_reset=False)
    assert cnt["consumed"] == cnt["steps"], cnt


def _random_actions(env, T, rs):
    sp = env.single_action_space
    if hasattr(sp, "n"):
        return rs.randint(0, sp.n, size=(T, env.num_envs)).astype(np.int32)
    return np.stack([rs.randint(0, int(k), size=(T, env.num_envs)) for k in sp.nvec], -1).astype(np.int32)


@pytest.mark.parametrize("prob,rep,calls", [("binary", "narrow", (dict(change_percentage=0.05),)),
                                            ("sokoban", "narrow", (dict(change_percentage=0.1),))], ids=_ids)
def test_state_round_trip_past_done(prob, rep, calls):
    """state_dict() in the middle of a run past done, load_state_dict() into a fresh batch: the resumed run must be the
    uninterrupted one, step for step (heat maps beyond the episodes' change budgets included)."""
    torch = _torch()
    from gym_pcgrl_amd.envs import BatchedPcgrlEnv

    def make():
        env = BatchedPcgrlEnv(prob=prob, rep=rep, num_envs=64, seed=555, auto_reset=False)
        for kw in calls:
            env.adjust_param(**kw)
        env.reset()
        return env
    T, cut = 80, 37
    a, b = make(), make()
    acts = _random_actions(a, T, np.random.RandomState(8))
    keys = list(a._prob.info_keys) + ["iterations", "changes"]

    def rows(env, obs, rew, done, info):
        return [obs[k].cpu().numpy().copy() for k in obs] + [rew.cpu().numpy().copy(), done.cpu().numpy().copy()] + \
               [info[k].cpu().numpy().copy() for k in keys]
    ref = [rows(a, *a.step(acts[t])) for t in range(T)]
    assert bool(a._bufs["done"].any().item()) and int(a._bufs["counters"][:, 1].max().item()) > a._max_changes
    for t in range(cut):
        b.step(acts[t])
    sd = b.state_dict()
    b.close()
    c = make()
    c.load_state_dict(sd)
    for t in range(cut, T):
        got = rows(c, *c.step(acts[t]))
        for k, (x, y) in enumerate(zip(got, ref[t])):
            assert np.array_equal(x, y), (prob, "step", t, "field", k)
    a.close(); c.close()


# ------------------------------------------------------------------ heat counts beyond 16 bits
def _alternating(m0, T):
    """Tiles that rewrite a cell holding m0 at every step: 1 - m0, m0, 1 - m0, ... (every write is a change)."""
    return np.where(np.arange(T) % 2 == 0, 1 - int(m0), int(m0)).astype(np.int32)


def test_facade_heat_map_counts_past_16_bits():
    """binary-wide 14 x 14 (max_changes 39) through the facade (no auto-reset), one cell rewritten 70 000 times: the reference's
    float64 heat map reads 70000.0 there and 0 everywhere else.  The first 300 steps against the oracle as well."""
    _torch()
    import gym_pcgrl_amd
    env = gym_pcgrl_amd.make("binary-wide-v0")
    env.seed(71)
    obs = env.reset()
    o = ol.OracleEnv("binary", "wide")
    o.seed(71)
    eo = o.reset()
    assert np.array_equal(obs["map"], eo["map"])
    x, y, T = 5, 9, 70000
    tiles = _alternating(obs["map"][y, x], T)
    for t in range(T):
        obs, rew, done, info = env.step(np.array([x, y, tiles[t]]))
        if t < 300:
            eo, er, ed, ei = o.step(np.array([x, y, tiles[t]]))
            assert rew == er and done == ed and np.array_equal(obs["map"], eo["map"]), ("facade vs oracle", t)
            assert obs["heatmap"].dtype == np.float64 and np.array_equal(obs["heatmap"], eo["heatmap"]), ("heatmap", t)
            assert all(info[k] == ei[k] for k in ei), ("info", t, info, ei)
    assert done and info["changes"] == T and info["iterations"] == T
    want = np.zeros((14, 14), np.float64)
    want[y, x] = 70000.0
    assert np.array_equal(obs["heatmap"], want), (obs["heatmap"][y, x], np.argwhere(obs["heatmap"] != want))


def test_batched_heat_map_counts_past_16_bits():
    """A batched rollout() without auto-reset past 65 536 changes of one cell per environment, 13 x 13 maps (169 cells: odd, so
    neighbouring environments share 32-bit words of a 16-bit heat map): environment 0 rewrites its LAST cell (the word it shares
    with environment 1's first cell), environment 1 a cell in the low half of a word, environment 2 one in the high half,
    environment 3 a cell in the middle.  Every count must be exact -- T at the rewritten cell, 0 at its neighbours and in the
    neighbouring environment -- and the observation must show it in a dtype that holds it."""
    torch = _torch()
    from gym_pcgrl_amd.envs import BatchedPcgrlEnv
    W = H = 13
    N, T = 4, 70000
    env = BatchedPcgrlEnv(prob="binary", rep="wide", num_envs=N, seed=321, auto_reset=False)
    env.adjust_param(width=W, height=H)
    obs = env.reset()
    m0 = obs["map"].cpu().numpy()
    cells = [(W - 1, H - 1), (1, 0), (1, 0), (6, 6)]            # (x, y)
    flat = [e * W * H + y * W + x for e, (x, y) in enumerate(cells)]
    assert flat[0] % 2 == 0 and flat[1] % 2 == 0 and flat[2] % 2 == 1    # low half / low half / high half of a 16-bit pair
    acts = np.zeros((T, N, 3), np.int32)
    for e, (x, y) in enumerate(cells):
        acts[:, e, 0], acts[:, e, 1], acts[:, e, 2] = x, y, _alternating(m0[e, y, x], T)
    rew, done, info = env.rollout(torch.as_tensor(acts, device="cuda"))
    # the first 300 steps against the oracle, stepped without reset()
    keys = list(env._prob.info_keys) + ["iterations", "changes"]
    got = np.stack([info[k].view(T, N)[:300].cpu().numpy() for k in keys], 2).astype(np.int64)
    for e in range(N):
        o = ol.OracleEnv("binary", "wide")
        o.adjust_param(width=W, height=H)
        o.seed(321 + e)
        assert np.array_equal(o.reset()["map"], m0[e])
        x = ph.oracle_noreset(o, acts[:300, e])
        assert np.array_equal(rew[:300, e].cpu().numpy(), x["reward"]) and np.array_equal(done[:300, e].cpu().numpy(), x["done"]), e
        assert np.array_equal(got[:, e], x["info"]), e
    assert bool(done[-1].all().item())
    assert np.array_equal(info["changes"].view(T, N)[-1].cpu().numpy(), [T] * N)
    heat = env._obs()["heatmap"]
    want = np.zeros((N, H, W), np.int64)
    for e, (x, y) in enumerate(cells):
        want[e, y, x] = T
    h = heat.cpu().numpy().astype(np.int64)
    assert np.array_equal(h, want), [(tuple(ix), int(h[tuple(ix)])) for ix in np.argwhere(h != want)[:8]]
    assert heat.dtype == torch.int32, heat.dtype
    env.close()


# ------------------------------------------------------------------ the reference's own runs past done (tests/golden/noreset.npz)
@pytest.mark.parametrize("prob,rep", [("binary", "wide"), ("zelda", "narrow")])
def test_reference_fixture_past_done(prob, rep):
    """make_golden.py gen_noreset: the unmodified reference stepped 300 times with no reset at change_percentage 0.05 (most steps past
    done).  A batch without auto-reset must give every step's reward / done / info, the final map and the final heat map."""
    _torch()
    from gym_pcgrl_amd.envs import BatchedPcgrlEnv
    d = np.load(os.path.join(G, "noreset.npz"))
    p = prob + "_"
    W, H, max_changes, max_iter, seed = [int(v) for v in d[p + "cfg"]]
    env = BatchedPcgrlEnv(prob=prob, rep=rep, num_envs=1, seed=seed, auto_reset=False)
    env.adjust_param(change_percentage=0.05)
    env.reset()
    assert (env._prob._width, env._prob._height, env._max_changes, env._max_iterations) == (W, H, max_changes, max_iter)
    keys = list(env._prob.info_keys) + ["iterations", "changes"]
    for t, a in enumerate(d[p + "actions"]):
        obs, rew, done, info = env.step(a[None] if rep == "wide" else a[:1])
        assert float(rew[0]) == d[p + "reward"][t] and bool(done[0]) == d[p + "done"][t], ("reward/done", t)
        assert [int(info[k][0]) for k in keys] == list(d[p + "info"][t]), ("info", t)
    assert np.array_equal(obs["map"][0].cpu().numpy(), d[p + "map"])
    heat = obs["heatmap"][0].cpu().numpy().astype(np.int64)
    cells = np.argwhere(heat != 0)
    assert np.array_equal(cells, d[p + "heat_cells"]) and np.array_equal(heat[cells[:, 0], cells[:, 1]], d[p + "heat_counts"])
    env.close()


def test_reference_fixture_heat_past_16_bits():
    """make_golden.py gen_noreset: one cell of binary-wide 14 x 14 rewritten 66 000 times by the reference, no reset -- as one
    rollout() tape without auto-reset: the kept steps' reward / done / info and the final heat map (the cell at 66 000, no other)."""
    torch = _torch()
    from gym_pcgrl_amd.envs import BatchedPcgrlEnv
    d = np.load(os.path.join(G, "noreset.npz"))
    W, H, seed, T, x, y, m0 = [int(v) for v in d["long_cfg"]]
    env = BatchedPcgrlEnv(prob="binary", rep="wide", num_envs=1, seed=seed, auto_reset=False)
    obs = env.reset()
    assert int(obs["map"][0, y, x].item()) == m0
    acts = np.zeros((T, 1, 3), np.int32)
    acts[:, 0, 0], acts[:, 0, 1], acts[:, 0, 2] = x, y, _alternating(m0, T)
    rew, done, info = env.rollout(torch.as_tensor(acts, device="cuda"))
    steps = d["long_steps"]
    keys = list(env._prob.info_keys) + ["iterations", "changes"]
    got = np.stack([info[k].view(T, 1)[:, 0].cpu().numpy() for k in keys], 1).astype(np.int64)
    assert np.array_equal(rew[:, 0].cpu().numpy()[steps], d["long_reward"]) and np.array_equal(done[:, 0].cpu().numpy()[steps], d["long_done"])
    assert np.array_equal(got[steps], d["long_info"])
    heat = env._obs()["heatmap"][0].cpu().numpy().astype(np.int64)
    cells = np.argwhere(heat != 0)
    assert np.array_equal(cells, d["long_heat_cells"]) and np.array_equal(heat[cells[:, 0], cells[:, 1]], d["long_heat_counts"])
    env.close()
