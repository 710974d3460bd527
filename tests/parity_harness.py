"""Step-by-step GPU-vs-oracle comparisons shared by the `-m gpu` tests and the command-line tools (tools/fuzz_parity.py,
tools/fullsize_parity.py).  Test infrastructure: the oracle is the checker here, never the thing measured.

fuzz_case(rs, ...)      one random (problem, representation, map size, parameters, seed) configuration; every step of the
                        HIP path -- stepping, or the whole tape as one pcgrl_rollout call -- against the CPU oracle
fullsize_case(...)      a benchmark configuration at its real batch size (the paths only large batches take: paired certain
                        resets, every bucket in use, 512 environments per persistent block); a sample of environments
                        compared with the oracle at every step
search_game_case(...)   chosen levels of a search problem through one stepping route (steps, one rollout, asynchronous ticks): four
                        scripted writes per environment that compute the level, its neighbour and both again
live_case(...)          a script of steps, rollouts and events -- adjust_param, seed, set_maps ... in the middle of running episodes --
                        on one handle; every step and the state after every phase against the oracle put through the same script
"""
import numpy as np

import oracle_lib as ol

REPS = ["narrow", "wide", "turtle", "narrowcast", "narrowmulti", "turtlecast"]
PROB_MIX = ["binary", "binary", "zelda", "zelda", "sokoban", "mdungeon", "mdungeon", "ddave", "ddave", "smb"]


def draw_config_extra(rs, mode, only=None):
    """The fuzz modes of round 4 (tools/fuzz_parity.py ... big|goal; their own draw stream, so that the seeded slice of draw_config
    that test_fuzz_slice runs stays what it was):
      big   sizes beyond the tuned kernels: maps with a side of 65..130 (csrc/bigmap.h), search levels of 257..1 200 bordered cells
            and now and then a solver_power beyond 16 383 (csrc/search_big.h);
      goal  binary / zelda on the fused step kernel with goals that are met all the time (target_path 1..3, a near enemy allowed):
            episodes end where nobody saw it coming, which is what the draw-cache hand-over between the update wavefronts and the
            in-kernel reset is for (StepLocal::pend)."""
    if mode == "goal":
        prob = only or ("binary", "zelda")[rs.randint(2)]
        rep = ("narrow", "narrow", "turtle", "wide")[rs.randint(4)]
        w, h = int(rs.randint(3, 33)), int(rs.randint(3, 17))
        calls = [dict(width=w, height=h), dict(change_percentage=float(rs.choice([0.2, 0.5, 1.0])), target_path=int(rs.randint(1, 4)))]
        if prob == "zelda":
            calls.append(dict(target_enemy_dist=int(rs.randint(1, 3)), probs={"empty": 0.8, "solid": 0.1, "player": 0.02, "key": 0.02, "door": 0.02,
                                                                              "bat": 0.01, "scorpion": 0.01, "spider": 0.01}))
        return prob, rep, (w, h), calls, int(rs.choice([96, 300, 1000])), 150, int(rs.randint(1, 10 ** 6))
    prob = only or ("binary", "zelda", "sokoban", "mdungeon", "ddave")[rs.randint(5)]
    rep = REPS[rs.randint(6)]
    if prob in ("binary", "zelda"):
        w, h = int(rs.randint(65, 131)), int(rs.randint(1, 131))
        if rs.rand() < 0.5:
            w, h = h, w
        calls = [dict(width=w, height=h), dict(change_percentage=float(rs.choice([0.001, 0.003, 0.01])))]
        E, T = int(rs.choice([5, 16, 40])), 60
    else:
        while True:
            w, h = int(rs.randint(3, 41)), int(rs.randint(3, 41))
            if 256 < (w + 2) * (h + 2) <= 1200:
                break
        power = int(rs.choice([60, 300, 1000])) if rs.rand() < 0.85 else 17000
        calls = [dict(width=w, height=h), dict(change_percentage=float(rs.choice([0.01, 0.03, 0.1])), solver_power=power)]
        if rs.rand() < 0.7:     # open maps with few of the things a level must have exactly one of: the planner runs
            few = float(rs.choice([0.002, 0.004]))
            if prob == "sokoban":
                calls.append(dict(probs={"empty": 0.93, "solid": 0.04, "player": few, "crate": few, "target": few}))
            elif prob == "mdungeon":
                calls.append(dict(probs={"empty": 0.9, "solid": 0.05, "player": few, "exit": few, "potion": 0.01, "treasure": 0.01, "goblin": 0.01, "ogre": 0.01}))
            else:
                calls.append(dict(probs={"empty": 0.8, "solid": 0.17, "player": few, "exit": few, "diamond": 0.004, "key": few, "spike": 0.004}))
        E, T = int(rs.choice([16, 48])), 80
    if rep in ("turtle", "turtlecast") and rs.rand() < 0.5:
        calls.append(dict(warp=True))
    return prob, rep, (w, h), calls, E, T, int(rs.randint(1, 10 ** 6))


def draw_config(rs, only=None):
    """-> (prob, rep, (w, h), calls, E, T, seed0, use_rollout): everything random about one fuzz configuration."""
    prob = only or PROB_MIX[rs.randint(len(PROB_MIX))]
    rep = REPS[rs.randint(6)]
    if prob == "sokoban":
        w, h = int(rs.randint(2, 8)), int(rs.randint(2, 8))
    elif prob in ("mdungeon", "ddave"):
        w, h = int(rs.randint(1, 13)), int(rs.randint(1, 13))
    elif prob == "smb":
        w, h = int(rs.randint(1, 61)), int(rs.randint(3, 17))
    else:
        w, h = int(rs.randint(1, 41)), int(rs.randint(1, 41))
        if rs.rand() < 0.4:
            h = int(rs.randint(1, 17)); w = int(rs.randint(1, 33))
    calls = [dict(width=w, height=h), dict(change_percentage=float(rs.choice([0.05, 0.2, 0.5, 1.0])))]
    if prob == "sokoban":
        calls.append(dict(solver_power=int(rs.choice([50, 300, 1000]))))
    if prob == "mdungeon":
        calls.append(dict(solver_power=int(rs.choice([50, 300, 1000, 5000]))))
        if rs.rand() < 0.7:     # open maps with few players / exits: the planner runs in a good share of the steps
            mon = float(rs.choice([0.0, 0.03, 0.15]))
            calls.append(dict(probs={"empty": 0.75, "solid": float(rs.choice([0.02, 0.1])), "player": 0.03, "exit": 0.03,
                                     "goblin": mon, "ogre": mon}))
        if rs.rand() < 0.5:
            calls.append(dict(target_solution=int(rs.randint(1, 8)), target_col_enemies=float(rs.choice([0.0, 0.3, 0.5])),
                              max_enemies=int(rs.randint(1, 5)), max_potions=int(rs.randint(0, 3)), max_treasures=int(rs.randint(0, 3)),
                              rewards={"dist-win": float(rs.choice([0.1, 0.3, 1.0])), "sol-length": float(rs.choice([1, 0.7]))}))
    if prob == "ddave":
        calls.append(dict(solver_power=int(rs.choice([50, 300, 1000, 5000]))))
        if rs.rand() < 0.7:     # open maps with few players / exits / keys: the planner runs in a good share of the steps
            calls.append(dict(probs={"empty": 0.7, "solid": float(rs.choice([0.05, 0.15])), "player": 0.04, "exit": 0.04, "key": 0.04,
                                     "spike": float(rs.choice([0.0, 0.03]))}))
        if rs.rand() < 0.5:
            calls.append(dict(target_solution=int(rs.randint(1, 8)), target_jumps=int(rs.randint(0, 3)), max_diamonds=int(rs.randint(0, 4)),
                              min_spikes=int(rs.randint(0, 6)), rewards={"dist-win": float(rs.choice([0.1, 0.3, 1.0])), "dist-floor": float(rs.choice([2, 0.5]))}))
    if prob == "smb" and rs.rand() < 0.7:      # mostly blocked levels: episodes do not end at once (smb_prob.py:191-192)
        calls.append(dict(probs={"empty": 0.5, "solid": float(rs.choice([0.3, 0.45])), "tube": float(rs.choice([0.02, 0.1]))}))
    if rep in ("narrow", "narrowcast", "narrowmulti") and rs.rand() < 0.3:
        calls.append(dict(random_tile=False))
    if rep in ("turtle", "turtlecast") and rs.rand() < 0.5:
        calls.append(dict(warp=True))
    if rs.rand() < 0.2:
        calls.append(dict(random_start=False))
    E = int(rs.choice([8, 33, 96])) if w * h > 400 else int(rs.choice([33, 96, 200]))
    T = 120 if w * h > 400 else 200
    seed0 = int(rs.randint(1, 10 ** 6))
    return prob, rep, (w, h), calls, E, T, seed0


MAP_EVERY = 5      # stepping: the cursor and the heat map are compared at every step, the whole map every MAP_EVERY steps and at the end


def _obs_mismatch(obs, exp, t, has_pos, sel=None, map_every=MAP_EVERY):
    """Observation of step t (device tensors, optionally the rows `sel`) against the oracle's: cursor and heat map always,
    the map every `map_every` steps.  -> None or the name of what differs."""
    pick = (lambda x: x) if sel is None else (lambda x: x[sel])
    if has_pos and not np.array_equal(pick(obs["pos"]).cpu().numpy().astype(np.int64), np.stack([x["pos"][t] for x in exp])):
        return "pos"
    if not np.array_equal(pick(obs["heatmap"]).cpu().numpy().astype(np.int64), np.stack([x["heatmap"][t] for x in exp]).astype(np.int64)):
        return "heatmap"
    if t % map_every == 0 and not np.array_equal(pick(obs["map"]).cpu().numpy(), np.stack([x["maps"][t] for x in exp])):
        return "map"
    return None


def oracle_noreset(o, actions):
    """The oracle stepped through `actions` [T, k] with PcgrlEnv.step and no reset at done (pcgrl_env.py:130-150: an episode goes
    on past done, the heat map keeps counting) -> the dict of OracleEnv.rollout, the heat map as the oracle's float64 counts."""
    keys = ol.INFO_KEYS[o.prob] + ["iterations", "changes"]
    steps = [o.step(a) for a in np.asarray(actions, dtype=np.int32).reshape(len(actions), -1)]
    return dict(maps=np.stack([s[0]["map"] for s in steps]), heatmap=np.stack([s[0]["heatmap"] for s in steps]),
                pos=np.stack([s[0].get("pos", np.zeros(2, np.uint8)) for s in steps]).astype(np.int32),
                reward=np.array([s[1] for s in steps], np.float64), done=np.array([s[2] for s in steps], bool),
                info=np.array([[s[3][k] for k in keys] for s in steps], np.int64).reshape(len(steps), len(keys)))


def _oracle_rollouts(prob, rep, calls, seeds, acts_by_env, auto_reset=True, keep_start=False):
    out = []
    for seed, a in zip(seeds, acts_by_env):
        o = ol.OracleEnv(prob, rep)
        for kw in calls:
            o.adjust_param(**kw)
        o.seed(int(seed))
        map0 = o.reset()["map"]
        out.append(o.rollout(a) if auto_reset else oracle_noreset(o, a))
        if keep_start:
            out[-1]["map0"] = map0
    return out


def action_dims(prob, rep, w, h):
    """The sizes of a representation's action space, as the representations define them (narrow_rep.py:37-38, turtle_rep.py:50-51,
    wide_rep.py:22-23, narrow_cast_rep.py:24-25, narrow_multi_rep.py:25-26, turtle_cast_rep.py:26-27) -- for drawing a tape of actions
    where there is no device to ask."""
    nt = len(ol.TILES[prob])
    return {"narrow": [nt + 1], "turtle": [nt + 4], "wide": [w, h, nt], "narrowcast": [3, nt], "narrowmulti": [nt + 1] * 9, "turtlecast": [6, nt]}[rep]


def draw_actions(dims, rs, T, E):
    """[T, E, len(dims)] int32, drawn from `rs` the way run_config always has."""
    if len(dims) == 1:
        return rs.randint(0, int(dims[0]), size=(T, E, 1)).astype(np.int32)
    return np.stack([rs.randint(0, int(k), size=(T, E)) for k in dims], -1).astype(np.int32)


def oracle_tape(prob, rep, calls, E, T, seed0, rs, sample=None):
    """The host half of run_config on its own: a tape of random actions for E environments and the oracle's rollouts of the
    environments `sample` (default: all), each with the map it started from as x["map0"].  -> (acts, exp), for run_config(tape=)."""
    o = ol.OracleEnv(prob, rep)
    for kw in calls:
        o.adjust_param(**kw)
    w, h = o.width, o.height
    acts = draw_actions(action_dims(prob, rep, w, h), rs, T, E)
    idx = np.arange(E) if sample is None else np.asarray(sample)
    return acts, _oracle_rollouts(prob, rep, calls, [seed0 + int(i) for i in idx], [acts[:, i] for i in idx], keep_start=True)


def run_config(prob, rep, calls, E, T, seed0, rs, use_rollout, mixed=False, steps_scale=1.0, auto_reset=True, map_every=MAP_EVERY,
               tuning=None, sample=None, tape=None, setup=None):
    """One configuration on the GPU against the oracle.  `mixed`: the first part of the tape as one rollout of ODD length,
    the rest as single steps on the same handle (switching between the fused and the work-list pipelines).  auto_reset=False:
    the environments step on past done, the oracle without reset().  tuning: the library's developer switches for this handle.
    sample: indices of the environments compared with the oracle (default: all).  tape: (acts, exp) of oracle_tape -- the actions
    and the oracle's side made beforehand (`rs` is then not drawn from).  setup: called with the batch after `calls`, before reset() -- for what
    adjust_param does not take (smb's solver_power); the tape's oracle side has to be made the same way.  Returns None or a string describing
    the first mismatch."""
    import torch
    from gym_pcgrl_amd.envs import BatchedPcgrlEnv
    T = max(4, int(T * steps_scale))
    env = BatchedPcgrlEnv(prob=prob, rep=rep, num_envs=E, seed=seed0, auto_reset=auto_reset, tuning=tuning)
    try:
        for kw in calls:
            env.adjust_param(**kw)
        if setup is not None:
            assert tape is not None, "setup= needs the oracle's side made the same way: pass tape="
            setup(env)
        env.reset()
        sp = env.single_action_space
        dims = [sp.n] if hasattr(sp, "n") else [int(k) for k in sp.nvec]
        idx = np.arange(E) if sample is None else np.asarray(sample)
        if tape is None:
            acts = draw_actions(dims, rs, T, E)
            exp = _oracle_rollouts(prob, rep, calls, [seed0 + int(i) for i in idx], [acts[:, i] for i in idx], auto_reset)
        else:
            acts, exp = tape
            assert acts.shape == (T, E, len(dims)) and len(exp) == len(idx) and dims == action_dims(prob, rep, env._prob._width, env._prob._height), \
                "the tape was made for another configuration"
        sel = None if sample is None else torch.as_tensor(idx, device="cuda")
        keys = list(env._prob.info_keys) + ["iterations", "changes"]
        t_roll = 0
        obs = env._obs()
        if use_rollout or mixed:
            t_roll = T if not mixed else (T // 3) | 1
            tape_d = torch.as_tensor(acts[:t_roll] if acts.shape[2] > 1 else acts[:t_roll, :, 0], device="cuda")
            rew_t, done_t, info_t = env.rollout(tape_d)
            col = (lambda x: x) if sel is None else (lambda x: x[:, sel])
            got_info = np.stack([col(info_t[k].view(t_roll, E)).cpu().numpy() for k in keys], 2).astype(np.int64)
            ok = np.array_equal(col(done_t).cpu().numpy(), np.stack([x["done"][:t_roll] for x in exp], 1)) and \
                np.array_equal(col(rew_t).cpu().numpy(), np.stack([x["reward"][:t_roll] for x in exp], 1)) and \
                np.array_equal(got_info, np.stack([x["info"][:t_roll] for x in exp], 1))
            if not ok:
                return "ROLLOUT MISMATCH %s %s %s E %d seed %d" % (prob, rep, calls, E, seed0)
        row = (lambda x: x) if sel is None else (lambda x: x[sel])
        for t in range(t_roll, T):
            obs, rew, done, info = env.step(acts[t] if acts.shape[2] > 1 else acts[t, :, 0])
            ok = np.array_equal(row(done).cpu().numpy(), np.array([x["done"][t] for x in exp])) and \
                np.array_equal(row(rew).cpu().numpy(), np.array([x["reward"][t] for x in exp])) and \
                np.array_equal(np.stack([row(info[k]).cpu().numpy() for k in keys], 1).astype(np.int64), np.stack([x["info"][t] for x in exp]))
            if not ok:
                return "MISMATCH %s %s %s E %d seed %d step %d" % (prob, rep, calls, E, seed0, t)
            bad = _obs_mismatch(obs, exp, t, env._rep.has_pos, sel, map_every=map_every)
            if bad:
                return "OBS MISMATCH (%s) %s %s %s E %d seed %d step %d" % (bad, prob, rep, calls, E, seed0, t)
        # the state the tape / the steps end in: map, cursor, heat map
        if not np.array_equal(row(obs["map"]).cpu().numpy(), np.stack([x["maps"][-1] for x in exp])):
            return "MAP MISMATCH %s %s %s E %d seed %d" % (prob, rep, calls, E, seed0)
        if env._rep.has_pos and not np.array_equal(row(obs["pos"]).cpu().numpy().astype(np.int64), np.stack([x["pos"][-1] for x in exp])):
            return "POS MISMATCH %s %s %s E %d seed %d" % (prob, rep, calls, E, seed0)
        if not np.array_equal(row(obs["heatmap"]).cpu().numpy().astype(np.int64), np.stack([x["heatmap"][-1] for x in exp]).astype(np.int64)):
            return "HEATMAP MISMATCH %s %s %s E %d seed %d" % (prob, rep, calls, E, seed0)
        env.check_status()
    finally:
        env.close()
    return None


def fuzz_case(rs, only=None, rollout_share=0.4, mixed_share=0.0, steps_scale=1.0, mode=None):
    """Draw one configuration from `rs` and run it.  -> (description, error or None)."""
    prob, rep, wh, calls, E, T, seed0 = draw_config(rs, only) if mode is None else draw_config_extra(rs, mode, only)
    u = rs.rand()
    use_rollout = u < rollout_share
    mixed = (not use_rollout) and u < rollout_share + mixed_share
    err = run_config(prob, rep, calls, E, T, seed0, rs, use_rollout, mixed, steps_scale)
    how = "rollout" if use_rollout else ("rollout+steps" if mixed else "steps")
    return "%s %s %s %s %s E %d" % (how, prob, rep, wh, [list(c.items())[0] for c in calls[1:]], E), err


FULLSIZE_CASES = {
    "C2": ("binary", "narrow", (), 65536, 160),
    "C3": ("zelda", "wide", (dict(width=11, height=16),), 65536, 80),
    "C5": ("binary", "turtle", (dict(width=64, height=64),), 8192, 100),
    "C4": ("sokoban", "narrow", (), 131072, 40),
    "M1": ("mdungeon", "narrow", (), 65536, 40),
    "D1": ("ddave", "narrow", (), 65536, 40),
    "S1": ("smb", "narrow", (), 16384, 30),
}


def fullsize_case(name, use_rollout, max_steps=None):
    """A benchmark configuration at its real batch size; 294 sampled environments (the first 64, the last 32, 200 spread
    over the batch) compared with the oracle at every step.  Raises AssertionError on a mismatch; returns the number of
    sampled environments."""
    import torch
    from gym_pcgrl_amd.envs import BatchedPcgrlEnv
    prob, rep, calls, N, T = FULLSIZE_CASES[name]
    if max_steps:
        T = min(T, max_steps)
    env = BatchedPcgrlEnv(prob=prob, rep=rep, num_envs=N, seed=0)
    try:
        for kw in calls:
            env.adjust_param(**kw)
        env.reset()
        sp = env.single_action_space
        g = torch.Generator(device="cuda"); g.manual_seed(5)
        if hasattr(sp, "n"):
            acts = torch.randint(0, sp.n, (T, N, 1), device="cuda", dtype=torch.int32, generator=g)
        else:
            acts = torch.stack([torch.randint(0, int(k), (T, N), device="cuda", dtype=torch.int32, generator=g) for k in sp.nvec], -1).contiguous()
        idx = np.unique(np.concatenate([np.arange(0, 64), np.linspace(0, N - 1, 200).astype(int), np.arange(N - 32, N)]))
        a_host = acts[:, torch.as_tensor(idx, device="cuda")].cpu().numpy()
        exp = _oracle_rollouts(prob, rep, calls, idx, [a_host[:, j] for j in range(len(idx))])
        keys = list(env._prob.info_keys) + ["iterations", "changes"]
        ti = torch.as_tensor(idx, device="cuda")
        obs = env._obs()
        if use_rollout:
            rew_t, done_t, info_t = env.rollout(acts if acts.shape[2] > 1 else acts[:, :, 0])
            got = np.stack([info_t[k].view(T, N)[:, ti].cpu().numpy() for k in keys], 2).astype(np.int64)
            assert np.array_equal(done_t[:, ti].cpu().numpy(), np.stack([x["done"] for x in exp], 1)), ("rollout done", name)
            assert np.array_equal(rew_t[:, ti].cpu().numpy(), np.stack([x["reward"] for x in exp], 1)), ("rollout reward", name)
            assert np.array_equal(got, np.stack([x["info"] for x in exp], 1)), ("rollout info", name)
        else:
            for t in range(T):
                obs, rew, done, info = env.step(acts[t] if acts.shape[2] > 1 else acts[t, :, 0])
                assert np.array_equal(done[ti].cpu().numpy(), np.array([x["done"][t] for x in exp])), ("done", name, t)
                assert np.array_equal(rew[ti].cpu().numpy(), np.array([x["reward"][t] for x in exp])), ("reward", name, t)
                assert np.array_equal(np.stack([info[k][ti].cpu().numpy() for k in keys], 1).astype(np.int64),
                                      np.stack([x["info"][t] for x in exp])), ("info", name, t)
                bad = _obs_mismatch(obs, exp, t, env._rep.has_pos, ti)
                assert bad is None, (bad, name, t)
        assert np.array_equal(obs["map"][ti].cpu().numpy(), np.stack([x["maps"][-1] for x in exp])), ("map", name)
        if env._rep.has_pos:
            assert np.array_equal(obs["pos"][ti].cpu().numpy().astype(np.int64), np.stack([x["pos"][-1] for x in exp])), ("pos", name)
        assert np.array_equal(obs["heatmap"][ti].cpu().numpy().astype(np.int64), np.stack([x["heatmap"][-1] for x in exp]).astype(np.int64)), ("heatmap", name)
        env.check_status()
    finally:
        env.close()
    return len(idx)


def async_case(prob, rep, calls, E, ticks, seed0, rs, pop_budget, nslots, sample=None, flush_every=0, tuning=None, auto_reset=True):
    """Asynchronous stepping (BatchedPcgrlEnv.tick, pcgrl_step_async) against the oracle: `ticks` ticks of random actions; per
    environment the actions it *took* (the ticks it was not pending at) and the outputs of every step it completed are recorded,
    and afterwards the oracle is stepped through exactly the taken actions -- reward, done, info, cursor, heat map and map of
    every completed step must be equal, bit for bit.  `sample`: indices of the environments compared (default: all).
    flush_every > 0: every that many ticks the pending steps are finished by flush() and a lockstep step() is taken in between
    (the two kinds of stepping on one handle).  auto_reset=False: past done, against the oracle without reset().  Returns a dict
    of counters; raises AssertionError on a mismatch."""
    import torch
    from gym_pcgrl_amd.envs import BatchedPcgrlEnv
    env = BatchedPcgrlEnv(prob=prob, rep=rep, num_envs=E, seed=seed0, tuning=tuning, auto_reset=auto_reset)
    try:
        for kw in calls:
            env.adjust_param(**kw)
        env.reset()
        assert env.enable_async(nslots), "no asynchronous form for this configuration"
        sp = env.single_action_space
        if hasattr(sp, "n"):
            acts = rs.randint(0, sp.n, size=(ticks, E, 1)).astype(np.int32)
        else:
            acts = np.stack([rs.randint(0, int(k), size=(ticks, E)) for k in sp.nvec], -1).astype(np.int32)
        idx = np.arange(E) if sample is None else np.asarray(sample)
        ti = torch.as_tensor(idx, device="cuda")
        keys = list(env._prob.info_keys) + ["iterations", "changes"]
        taken = [[] for _ in idx]
        got = [[] for _ in idx]
        pending = np.zeros(len(idx), bool)
        in_flight = [None] * len(idx)
        n_pending_ticks = 0
        for t in range(ticks):
            lock = flush_every and t % flush_every == flush_every - 1
            a = acts[t] if acts.shape[2] > 1 else acts[t, :, 0]
            if lock:
                # lockstep step on the same handle: finishes what is pending first (those steps complete with their own actions),
                # then every environment takes a[t]
                env.flush()
                assert not env._async["pending"][ti].any()
                rows_f = _async_rows(env, ti, keys)
                for j in np.nonzero(pending)[0]:
                    got[j].append(tuple(x[j] for x in rows_f))
                pending[:] = False
                obs, rew, done, info = env.step(a)
                after = np.zeros(len(idx), bool)
            else:
                obs, rew, done, info, pend = env.tick(a, pop_budget=pop_budget)
                after = pend[ti].cpu().numpy() != 0
            rows = None
            for j in range(len(idx)):
                if not pending[j]:
                    taken[j].append(acts[t, idx[j]])
                if not after[j]:
                    if rows is None:
                        rows = _async_rows(env, ti, keys)
                    got[j].append(tuple(x[j] for x in rows))
            pending = after
            n_pending_ticks += int(after.sum())
        env.flush()
        rows = _async_rows(env, ti, keys)
        for j in np.nonzero(pending)[0]:
            got[j].append(tuple(x[j] for x in rows))
        cnt = env.async_counters()
        exp = _oracle_rollouts(prob, rep, calls, [seed0 + int(i) for i in idx], [np.asarray(tk) for tk in taken], auto_reset)
        for j, x in enumerate(exp):
            assert len(got[j]) == len(taken[j]), ("steps completed vs actions taken", prob, idx[j], len(got[j]), len(taken[j]))
            for k, (rew_k, done_k, info_k, pos_k, heat_k, map_k) in enumerate(got[j]):
                where = (prob, rep, "env", int(idx[j]), "its step", k)
                assert rew_k == x["reward"][k] and bool(done_k) == bool(x["done"][k]), ("reward/done",) + where + (rew_k, x["reward"][k], done_k, x["done"][k])
                assert np.array_equal(info_k, x["info"][k]), ("info",) + where + (info_k, x["info"][k])
                if env._rep.has_pos:
                    assert np.array_equal(pos_k, x["pos"][k]), ("pos",) + where
                assert np.array_equal(heat_k, x["heatmap"][k].astype(np.int64)), ("heatmap",) + where
                assert np.array_equal(map_k, x["maps"][k]), ("map",) + where
        env.check_status()
        cnt["pending_env_ticks"] = n_pending_ticks
        cnt["steps"] = sum(len(tk) for tk in taken)
        return cnt
    finally:
        env.close()


def _async_rows(env, ti, keys):
    b = env._bufs
    info = env._prob.decode_rows(b["info"]) if env._prob.packed_rows else None
    tab = b["info"][ti].cpu().numpy().astype(np.int64)
    if info is not None:
        from gym_pcgrl_amd.envs.batched_env import InfoBatch
        ib = InfoBatch(env._prob.info_keys, b["info"], env._max_iterations, env._max_changes, env._prob.decode_rows)
        inf = np.stack([ib[k][ti].cpu().numpy() for k in keys], 1).astype(np.int64)
    else:
        nk = len(env._prob.info_keys)
        inf = np.concatenate([tab[:, :nk], tab[:, 8:10]], 1)
    return (b["reward"][ti].cpu().numpy(), b["done"][ti].cpu().numpy(), inf, b["pos"][ti].cpu().numpy().astype(np.int64),
            b["heatmap"][ti].cpu().numpy().astype(np.int64), b["map"][ti].cpu().numpy())


def flip_tape(maps, cells):
    """For levels `maps` [N, H, W] and one cell (x, y) per level that is empty or solid in it: the neighbours M' (that cell flipped
    between empty and solid) and the wide actions [4, N, 3] that write the cell back to its value in M, to M' again, and both once
    more -- the level itself is what steps 1 and 3 compute, its neighbour steps 2 and 4."""
    maps = np.ascontiguousarray(maps, dtype=np.uint8)
    n = len(maps)
    x, y = np.asarray(cells)[:, 0], np.asarray(cells)[:, 1]
    v = maps[np.arange(n), y, x]
    assert (v <= 1).all()
    start = maps.copy()
    start[np.arange(n), y, x] = 1 - v
    acts = np.stack([np.stack([x, y, v if t % 2 == 0 else 1 - v], 1) for t in range(4)]).astype(np.int32)
    return start, acts


def write_tape(maps, cells, tiles):
    """flip_tape for any write: for levels `maps` [N, H, W], one cell (x, y) and one other tile per level, the neighbours M' (that cell
    holding the tile) and the wide actions [4, N, 3] that write the cell back to its value in M, to the tile again, and both once more
    -- steps 1 and 3 compute M, steps 2 and 4 M'."""
    maps = np.ascontiguousarray(maps, dtype=np.uint8)
    n = len(maps)
    x, y = np.asarray(cells)[:, 0], np.asarray(cells)[:, 1]
    v = maps[np.arange(n), y, x]
    tiles = np.asarray(tiles).astype(np.uint8)
    assert tiles.shape == (n,) and (tiles != v).all()
    start = maps.copy()
    start[np.arange(n), y, x] = tiles
    acts = np.stack([np.stack([x, y, v if t % 2 == 0 else tiles], 1) for t in range(4)]).astype(np.int32)
    return start, acts


def smb_game_expected(w, h, power, maps, cells, tiles, seed0=7000, auto_reset=True):
    """What the oracle says of smb_game_case's four steps -> dict(start, acts, reward [4, N], done, info [4, N, keys], maps [4, N, H, W]).
    The oracle's solver_power is set the way smb's is (OracleEnv.set_solver_power), before the reset."""
    start, acts = write_tape(maps, cells, tiles)
    exp = []
    for i in range(len(maps)):
        o = ol.OracleEnv("smb", "wide")
        o.adjust_param(width=w, height=h)
        o.adjust_param(change_percentage=1.0)
        o.set_solver_power(power)
        o.seed(seed0 + i)
        o.reset()
        o.set_map(start[i])
        exp.append(o.rollout(acts[:, i], want_heat=False) if auto_reset else oracle_noreset(o, acts[:, i]))
    return dict(start=start, acts=acts, reward=np.stack([x["reward"] for x in exp], 1), done=np.stack([x["done"] for x in exp], 1),
                info=np.stack([x["info"] for x in exp], 1), maps=np.stack([x["maps"] for x in exp], 1))


def smb_game_case(w, h, power, maps, cells, tiles, route, tuning=None, auto_reset=True, seed0=7000, labels=None, expected=None):
    """search_game_case for smb (tests/test_gpu_smb_games.py): chosen levels through a stepping route against the oracle.  One handle of
    N wide environments, change_percentage 1.0, solver_power set as smb's is (prob._solver_power, then adjust_param()); set_maps() puts
    every environment one write away from its level (write_tape: the cell holds `tiles[i]`), four actions write the level's tile, the
    other one, and both again.  route: "step" -- step() four times; "rollout" -- the four actions as one rollout() (smb has no
    asynchronous form).  Reward, done, every info column (iterations and changes too) of every step and the map must equal the
    oracle's (smb_game_expected: seeded seed0 + i, reset(), set_map(), the four steps, with auto-reset or -- auto_reset=False -- on past
    done); check_status() must be 0.  expected: smb_game_expected of the same arguments, computed before."""
    import torch
    from gym_pcgrl_amd.envs import BatchedPcgrlEnv
    n = len(maps)
    E = expected if expected is not None else smb_game_expected(w, h, power, maps, cells, tiles, seed0, auto_reset)
    start, acts = E["start"], E["acts"]

    def check(what, got, want, t):
        got, want = np.asarray(got), np.asarray(want)
        bad = np.nonzero((got != want).reshape(n, -1).any(1))[0]
        if bad.size:
            i = int(bad[0])
            raise AssertionError("%s differs at step %d (route %s, smb %dx%d power %d, tuning %s) for %d levels: %s; level %d, cell %s, tiles %d <-> %d: got %s, the oracle %s"
                                 % (what, t, route, w, h, power, tuning, bad.size, [(int(j), labels[j] if labels else "") for j in bad[:8]],
                                    i, tuple(int(v) for v in acts[0, i, :2]), acts[0, i, 2], acts[1, i, 2], got[i].tolist(), want[i].tolist()))

    env = BatchedPcgrlEnv(prob="smb", rep="wide", num_envs=n, seed=seed0, tuning=tuning, auto_reset=auto_reset)
    try:
        env.adjust_param(width=w, height=h)
        env.adjust_param(change_percentage=1.0)
        env._prob._solver_power = int(power)
        env.adjust_param()
        env.reset()
        keys = list(env._prob.info_keys) + ["iterations", "changes"]
        env.set_maps(start)
        if route == "step":
            for t in range(4):
                obs, rew, done, info = env.step(acts[t])
                check("done", done.cpu().numpy(), E["done"][t], t)
                check("info", np.stack([info[k].cpu().numpy() for k in keys], 1).astype(np.int64), E["info"][t], t)
                check("reward", rew.cpu().numpy(), E["reward"][t], t)
                check("map", obs["map"].cpu().numpy(), E["maps"][t], t)
        elif route == "rollout":
            rew, done, info = env.rollout(torch.as_tensor(acts, device=env.device))
            got_info = np.stack([info[k].view(4, n).cpu().numpy() for k in keys], 2).astype(np.int64)
            for t in range(4):
                check("done", done[t].cpu().numpy(), E["done"][t], t)
                check("info", got_info[t], E["info"][t], t)
                check("reward", rew[t].cpu().numpy(), E["reward"][t], t)
            check("map", env._bufs["map"].cpu().numpy(), E["maps"][3], 3)
        else:
            raise ValueError(route)
        assert env.check_status() == 0
    finally:
        env.close()


def search_game_case(prob, w, h, power, maps, cells, route, seed0=7000, tuning=None, pop_budget=4, nslots=8, labels=None):
    """Chosen levels through one stepping route of a search problem against the oracle (tests/test_gpu_search_games.py).  One handle
    of N wide environments with change_percentage 1.0; set_maps() puts every environment one write away from its level (flip_tape)
    and four actions compute the level, its neighbour, and both again.  route: "step" -- step() four times; "rollout" -- the four
    actions as one rollout(); "async" -- enable_async(nslots) and tick(pop_budget) until every environment has completed the four
    steps and nothing is pending.  Reward, done and every info column of every step, and the map, must equal the oracle's
    (OracleEnv seeded seed0 + i, reset(), set_map(), the four steps with auto-reset); check_status() must be 0.  labels: a name per
    level for the message of a mismatch.  Returns the asynchronous counters (route "async") or None."""
    import torch
    from gym_pcgrl_amd.envs import BatchedPcgrlEnv
    n = len(maps)
    calls = [dict(width=w, height=h), dict(change_percentage=1.0, solver_power=power)]
    start, acts = flip_tape(maps, cells)
    exp = []
    for i in range(n):
        o = ol.OracleEnv(prob, "wide")
        for kw in calls:
            o.adjust_param(**kw)
        o.seed(seed0 + i)
        o.reset()
        o.set_map(start[i])
        exp.append(o.rollout(acts[:, i]))
    e_rew = np.stack([x["reward"] for x in exp], 1)           # [4, N]
    e_done = np.stack([x["done"] for x in exp], 1)
    e_info = np.stack([x["info"] for x in exp], 1)            # [4, N, keys]
    e_maps = np.stack([x["maps"] for x in exp], 1)            # [4, N, H, W]

    def check(what, got, want, t):
        got, want = np.asarray(got), np.asarray(want)
        bad = np.nonzero((got != want).reshape(n, -1).any(1))[0]
        if bad.size:
            i = int(bad[0])
            raise AssertionError("%s differs at step %d (route %s, %s %dx%d power %d) for %d levels: %s; level %d: got %s, the oracle %s"
                                 % (what, t, route, prob, w, h, power, bad.size, [(int(j), labels[j] if labels else "") for j in bad[:8]],
                                    i, got[i].tolist(), want[i].tolist()))

    env = BatchedPcgrlEnv(prob=prob, rep="wide", num_envs=n, seed=seed0, tuning=tuning)
    try:
        for kw in calls:
            env.adjust_param(**kw)
        env.reset()
        keys = list(env._prob.info_keys) + ["iterations", "changes"]
        cnt = None
        if route == "async":
            assert env.enable_async(nslots), "no asynchronous form for this configuration"
        env.set_maps(start)
        if route == "step":
            for t in range(4):
                obs, rew, done, info = env.step(acts[t])
                check("done", done.cpu().numpy(), e_done[t], t)
                check("reward", rew.cpu().numpy(), e_rew[t], t)
                check("info", np.stack([info[k].cpu().numpy() for k in keys], 1).astype(np.int64), e_info[t], t)
                check("map", obs["map"].cpu().numpy(), e_maps[t], t)
        elif route == "rollout":
            rew, done, info = env.rollout(torch.as_tensor(acts, device=env.device))
            got_info = np.stack([info[k].view(4, n).cpu().numpy() for k in keys], 2).astype(np.int64)
            for t in range(4):
                check("done", done[t].cpu().numpy(), e_done[t], t)
                check("reward", rew[t].cpu().numpy(), e_rew[t], t)
                check("info", got_info[t], e_info[t], t)
            check("map", env._bufs["map"].cpu().numpy(), e_maps[3], 3)
        elif route == "async":
            ti = torch.arange(n, device=env.device)
            ar = np.arange(n)
            ntaken, ngot = np.zeros(n, np.int64), np.zeros(n, np.int64)
            pending = np.zeros(n, bool)
            got = [[np.zeros_like(e[t]) for t in range(4)] for e in (e_rew, e_done, e_info, e_maps)]
            # every search ends within 4 * power pops; a tick gives a suspended one pop_budget of them (and the end of an episode takes one more)
            max_ticks = 4 * (4 * power // pop_budget + 4) + 64
            for tick in range(max_ticks):
                a = acts[np.minimum(ntaken, 3), ar]              # past its four steps an environment repeats the last write
                _obs, _rew, _done, _info, pend = env.tick(a, pop_budget=pop_budget)
                after = pend.cpu().numpy() != 0
                ntaken += ~pending
                fresh = ~after & (ngot < 4)
                if fresh.any():
                    rew_k, done_k, info_k, _pos, _heat, map_k = _async_rows(env, ti, keys)
                    for j in np.nonzero(fresh)[0]:
                        for dst, src in zip(got, (rew_k, done_k, info_k, map_k)):
                            dst[ngot[j]][j] = src[j]
                ngot += ~after
                pending = after
                if not after.any() and (ngot >= 4).all():
                    break
            else:
                raise AssertionError("still pending after %d ticks: %s" % (max_ticks, np.nonzero(pending | (ngot < 4))[0][:8]))
            assert (ntaken >= ngot).all()
            for t in range(4):
                check("done", got[1][t] != 0, e_done[t], t)
                check("reward", got[0][t], e_rew[t], t)
                check("info", got[2][t], e_info[t], t)
                check("map", got[3][t], e_maps[t], t)
            cnt = env.async_counters()
            cnt["ticks"] = tick + 1
        else:
            raise ValueError(route)
        assert env.check_status() == 0
        return cnt
    finally:
        env.close()


def live_steps(script):
    """Number of steps in a live_case script."""
    return sum(int(arg) for kind, arg in script if kind in ("step", "rollout"))


def live_oracle(prob, rep, calls, E, script, seed0, acts):
    """The oracle's side of live_case, without a device: E OracleEnvs (environment i seeded seed0 + i, `calls`, reset()) put through
    `script` with the actions acts [T, E, k], auto-reset at done.  -> dict: reward [T, E], done [T, E], info [T, E, keys + iterations +
    changes], limits [T, 2] (max_changes, max_iterations in force at the step), phase [T] (the script entry a step belongs to),
    start / states[p] (map, pos, heatmap after reset() / after script entry p), first[p] (the first step after entry p)."""
    orc = []
    for i in range(E):
        o = ol.OracleEnv(prob, rep)
        for kw in calls:
            o.adjust_param(**kw)
        o.seed(seed0 + i)
        o.reset()
        orc.append(o)

    def state():
        obs = [o.obs() for o in orc]
        return dict(map=np.stack([x["map"] for x in obs]), heatmap=np.stack([x["heatmap"] for x in obs]).astype(np.int64),
                    pos=np.stack([x.get("pos", np.zeros(2, np.uint8)) for x in obs]).astype(np.int64))

    rec = dict(reward=[], done=[], info=[], limits=[], phase=[], start=state(), states=[], first=[])
    t = 0
    for p, (kind, arg) in enumerate(script):
        rec["first"].append(t)
        if kind == "event":
            for i, o in enumerate(orc):
                arg(o, i)
        elif kind in ("step", "rollout"):
            for _ in range(int(arg)):
                rows = [o.rollout(acts[t, i][None], want_maps=False, want_heat=False) for i, o in enumerate(orc)]
                rec["reward"].append(np.array([x["reward"][0] for x in rows]))
                rec["done"].append(np.array([x["done"][0] for x in rows]))
                rec["info"].append(np.stack([x["info"][0] for x in rows]))
                lim = {(o.max_changes, o.max_iterations) for o in orc}
                assert len(lim) == 1, lim
                rec["limits"].append(lim.pop())
                rec["phase"].append(p)
                t += 1
        else:
            raise ValueError(kind)
        rec["states"].append(state())
    assert t == len(acts), (t, len(acts))
    for k in ("reward", "done", "info", "limits", "phase"):
        rec[k] = np.array(rec[k])
    return rec


def live_case(prob, rep, calls, E, script, seed0, acts, tuning=None, setup=None, rec=None):
    """Reconfiguring a handle that is being stepped (tests/test_gpu_live_handle.py).  One handle of E environments (seed0, `calls`,
    setup(env) if given, reset()) goes through `script`, a list of
      ("step", n)      n calls of step()
      ("rollout", n)   n steps as one rollout()
      ("event", fn)    fn(env, None) on the batch and fn(oracle i, i) on every OracleEnv -- adjust_param, seed, set_maps / set_map ...
    with the actions acts [T, E, k] (draw_actions).  Every environment is compared with the oracle (live_oracle; `rec`: its result,
    when the caller made it already): reward, done, every info column, iterations, changes, max_changes and max_iterations of every
    step, map, cursor and heat map after reset() and after every script entry, and check_status() == 0 there.  All exact.  Returns
    the oracle's record, for what a test has to ask of its own case; raises AssertionError on the first difference."""
    import torch
    from gym_pcgrl_amd.envs import BatchedPcgrlEnv
    if rec is None:
        rec = live_oracle(prob, rep, calls, E, script, seed0, acts)
    what = "%s %s %s E %d seed %d" % (prob, rep, calls, E, seed0)

    def same(name, got, want, where):
        got, want = np.asarray(got), np.asarray(want)
        assert got.shape == want.shape, (name, where, got.shape, want.shape)
        bad = np.nonzero((got != want).reshape(E, -1).any(1))[0]
        if bad.size:
            i = int(bad[0])
            raise AssertionError("%s differs %s (%s) in %d environments %s; environment %d: got %s, the oracle %s"
                                 % (name, where, what, bad.size, bad[:8].tolist(), i, got[i].tolist(), want[i].tolist()))

    env = BatchedPcgrlEnv(prob=prob, rep=rep, num_envs=E, seed=seed0, tuning=tuning)
    try:
        for kw in calls:
            env.adjust_param(**kw)
        if setup is not None:
            setup(env)
        env.reset()
        keys = list(env._prob.info_keys) + ["iterations", "changes"]
        wide_act = acts.shape[2] > 1

        def same_state(want, where):
            obs = env._obs()
            same("map", obs["map"].cpu().numpy(), want["map"], where)
            if env._rep.has_pos:
                same("pos", obs["pos"].cpu().numpy().astype(np.int64), want["pos"], where)
            same("heatmap", obs["heatmap"].cpu().numpy().astype(np.int64), want["heatmap"], where)
            assert env.check_status() == 0, where

        def same_step(t, rew, done, info_cols, limits):
            where = "at step %d (script entry %d)" % (t, rec["phase"][t])
            same("done", done, rec["done"][t], where)
            same("reward", rew, rec["reward"][t], where)
            same("info", info_cols, rec["info"][t], where)
            assert tuple(int(v) for v in limits) == tuple(int(v) for v in rec["limits"][t]), ("max_changes / max_iterations", where, limits, rec["limits"][t])

        same_state(rec["start"], "after reset()")
        t = 0
        for p, (kind, arg) in enumerate(script):
            if kind == "event":
                arg(env, None)
            elif kind == "step":
                for _ in range(int(arg)):
                    obs, rew, done, info = env.step(acts[t] if wide_act else acts[t, :, 0])
                    same_step(t, rew.cpu().numpy(), done.cpu().numpy(), np.stack([info[k].cpu().numpy() for k in keys], 1).astype(np.int64),
                              (info["max_changes"], info["max_iterations"]))
                    t += 1
            else:
                n = int(arg)
                tape = torch.as_tensor(acts[t:t + n] if wide_act else acts[t:t + n, :, 0], device=env.device)
                rew, done, info = env.rollout(tape)
                cols = np.stack([info[k].view(n, E).cpu().numpy() for k in keys], 2).astype(np.int64)
                rew, done = rew.cpu().numpy(), done.cpu().numpy()
                for j in range(n):
                    same_step(t + j, rew[j], done[j], cols[j], (info["max_changes"], info["max_iterations"]))
                t += n
            same_state(rec["states"][p], "after script entry %d (%s)" % (p, kind))
    finally:
        env.close()
    return rec


def expected_image(m, pos, oh, ow, centered, pad, depth):
    """wrappers.py restated with numpy: Cropped.transform :197-206 (np.pad with the border tile, window at the cursor),
    OneHotEncoding.transform :101-104 (np.eye(dim)[map]), ToImage.transform :53-60.  m [N,H,W], pos [N,2] = (x, y)."""
    n, H, W = m.shape
    out = np.full((n, oh, ow), pad, dtype=np.int64)
    for i in range(n):
        if centered:
            ph_, pw_ = oh // 2 + oh, ow // 2 + ow
            padded = np.pad(m[i].astype(np.int64), ((ph_, ph_), (pw_, pw_)), constant_values=pad)
            x, y = int(pos[i, 0]), int(pos[i, 1])
            out[i] = padded[y + ph_ - oh // 2: y + ph_ - oh // 2 + oh, x + pw_ - ow // 2: x + pw_ - ow // 2 + ow]
        else:
            hh, ww = min(oh, H), min(ow, W)
            out[i, :hh, :ww] = m[i, :hh, :ww]
    if depth == 1:
        return out[..., None].astype(np.uint8)
    return np.eye(depth, dtype=np.uint8)[out]


def fullsize_wrapped_case(name, max_steps=40):
    """The trainer-shaped configurations of bench.py at their real batch size against the ORACLE (not against another call of the
    library): C2w = binary-narrow behind CroppedImagePCGRLWrapper(28) -- the fused step writes the [N, 28, 28, 1] image --, C3w =
    zelda-wide 11 x 16 behind ActionMapImagePCGRLWrapper -- flat ActionMap indices decoded inside the step (pcgrl_step_flat), one-hot
    [N, 16, 11, 8] image.  294 sampled environments: the oracle is stepped with the decoded actions (wrappers.py:139-154: index into
    (H, W, tiles)); reward, done, info and the IMAGE (the wrappers' transform of the oracle's map and cursor) of every step."""
    import torch
    from gym_pcgrl_amd import wrappers
    from gym_pcgrl_amd.envs import BatchedPcgrlEnv
    N = 65536
    if name == "C2w":
        prob, rep, calls = "binary", "narrow", []
    else:
        prob, rep, calls = "zelda", "wide", [dict(width=11, height=16)]
    env = BatchedPcgrlEnv(prob=prob, rep=rep, num_envs=N, seed=0)
    for kw in calls:
        env.adjust_param(**kw)
    w = wrappers.CroppedImagePCGRLWrapper(env, 28) if name == "C2w" else wrappers.ActionMapImagePCGRLWrapper(env)
    try:
        img = w.reset()
        W, H, nt = env._prob._width, env._prob._height, env.get_num_tiles()
        T = max_steps
        g = torch.Generator(device="cuda"); g.manual_seed(6)
        if name == "C2w":
            acts = torch.randint(0, nt + 1, (T, N), device="cuda", dtype=torch.int32, generator=g)
        else:
            acts = torch.randint(0, W * H * nt, (T, N), device="cuda", dtype=torch.int32, generator=g)
        idx = np.unique(np.concatenate([np.arange(0, 64), np.linspace(0, N - 1, 200).astype(int), np.arange(N - 32, N)]))
        ti = torch.as_tensor(idx, device="cuda")
        a_host = acts[:, ti].cpu().numpy()
        if name == "C2w":
            dec = a_host[:, :, None]
        else:       # ActionMap: flat -> (x, y, tile)
            dec = np.stack([(a_host // nt) % W, a_host // (nt * W), a_host % nt], -1)
        exp = _oracle_rollouts(prob, rep, calls, idx, [dec[:, j] for j in range(len(idx))])
        keys = list(env._prob.info_keys) + ["iterations", "changes"]
        oh, ow, centered, pad = w._window()
        depth = nt if w.one_hot else 1
        for t in range(T):
            img, rew, done, info = w.step(acts[t])
            assert np.array_equal(done[ti].cpu().numpy(), np.array([x["done"][t] for x in exp])), ("done", name, t)
            assert np.array_equal(rew[ti].cpu().numpy(), np.array([x["reward"][t] for x in exp])), ("reward", name, t)
            assert np.array_equal(np.stack([info[k][ti].cpu().numpy() for k in keys], 1).astype(np.int64), np.stack([x["info"][t] for x in exp])), ("info", name, t)
            e_img = expected_image(np.stack([x["maps"][t] for x in exp]), np.stack([x["pos"][t] for x in exp]), oh, ow, centered, pad, depth)
            got = img[ti].cpu().numpy()
            bad = np.nonzero((got != e_img).reshape(len(idx), -1).any(1))[0]
            assert bad.size == 0, ("image", name, t, idx[bad[:5]])
        env.check_status()
    finally:
        env.close()
    return len(idx)
