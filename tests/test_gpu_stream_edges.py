"""The MT19937 draw paths at their rejection, wrap and staging edges, on the device, against the oracle and the numpy stream model.

Every test runs a case of tests/stream_model.py -- a shape, a problem, seeds and a tape chosen so that the rarely taken branches of
the draw code are taken (tests/test_stream_census_host.py counts them without a GPU: the draw cache's fallback, k_update's, lane 0's
in wave_draw_xy with and without the rest of the ring to re-stage, certain resets that draw the step's cursor move themselves, episode
ends nobody foresaw whose cache words are patched into the staged ring, stretches that cross slot 623 -> 0, axes of one cell).  After
every step: map, cursor position, heat map, reward, done and every info column against the oracle, bit for bit, and rng_cursor[:, 0]
against the model's ring cursor.  At the end the ring itself, two ways: rng_rep against the lazy-ring image built from numpy's state
arrays (slots below the cursor: the block of 624 being consumed; the others: the block before), and again after reset() calls that
make every environment consume at least 624 more words -- a write-back that missed a word does not survive that lap.
check_status() is 0 throughout.

Routes (stream_model.Case.route; the classes each covers are tabulated in README.md):
  reset() called repeatedly (k_reset, k_big)            every case, behind its tape run as one rollout()
  step() on k_step, step_pair 0 and 1                    the "fused" cases
  no_fused = 1, pair_min = 1 (k_update + k_stats)        the same cases
  step() on k_stats_wide / k_big / k_step_solver / k_smb the "block", "big", "solver", "smb" cases
  tick() with a small pop budget                         the "solver" cases
  seed() / load_state_dict() in the middle of a tape     the draw cache dropped under running episodes (TAG)
"""
import numpy as np
import pytest

import stream_model as sm

pytestmark = pytest.mark.gpu

FUSED = [c.name for c in sm.CASES if c.route == "fused"]
OTHER = [c.name for c in sm.CASES if c.route in ("block", "big", "solver", "smb")]
SOLVER = [c.name for c in sm.CASES if c.route == "solver"]


def _tune(monkeypatch, field, value):
    """A developer switch of the library (include/pcgrl_hip.h pcgrl_tuning) for the environments made in this test."""
    from gym_pcgrl_amd import _lib
    monkeypatch.setitem(_lib.TUNING_OVERRIDES, field, int(value))


def _make(case, seeds):
    import torch
    from gym_pcgrl_amd.envs import BatchedPcgrlEnv
    assert torch.cuda.is_available(), "these tests need the MI355X"
    env = BatchedPcgrlEnv(prob=case.prob, rep=case.rep, num_envs=len(seeds), seed=0)
    for kw in case.calls:
        env.adjust_param(**kw)
    env.seed([int(s) for s in seeds])
    return env


def _stacked(tr):
    """The oracle's side of a trace as [T, E, ...] arrays (made once per trace)."""
    if "stacked" not in tr:
        exp = tr["exp"]
        tr["stacked"] = dict(reward=np.stack([x["reward"] for x in exp], 1), done=np.stack([x["done"] for x in exp], 1),
                             info=np.stack([x["info"] for x in exp], 1), maps=np.stack([x["maps"] for x in exp], 1),
                             pos=np.stack([x["pos"] for x in exp], 1).astype(np.int64), heat=np.stack([x["heatmap"] for x in exp], 1).astype(np.int64),
                             map0=np.stack([x["map0"] for x in exp]))
    return tr["stacked"]


def _same(what, got, want, where, seeds):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, where, got.shape, want.shape)
    bad = np.nonzero((got != want).reshape(len(want), -1).any(1))[0]
    if bad.size:
        i = int(bad[0])
        raise AssertionError("%s differs %s in %d environments %s (seeds %s); environment %d: got %s, expected %s"
                             % (what, where, bad.size, bad[:8].tolist(), [seeds[j] for j in bad[:8]], i, got[i].tolist(), want[i].tolist()))


def _info_cols(info, keys):
    return np.stack([info[k].cpu().numpy() for k in keys], 1).astype(np.int64)


def _check_state(env, S, t, cursor, where, seeds, has_pos):
    b = env._bufs
    _same("map", b["map"].cpu().numpy(), S["maps"][t], where, seeds)
    if has_pos:
        _same("cursor position", b["pos"].cpu().numpy().astype(np.int64), S["pos"][t], where, seeds)
    _same("heat map", env._obs()["heatmap"].cpu().numpy().astype(np.int64), S["heat"][t], where, seeds)
    _same("ring cursor", b["rng_cursor"][:, 0].cpu().numpy(), cursor, where, seeds)


def _check_ring(env, models, where, seeds):
    """rng_cursor and rng_rep against the model: the ring is the lazy-ring image of numpy's state arrays."""
    b = env._bufs
    _same("ring cursor", b["rng_cursor"][:, 0].cpu().numpy(), np.array([m.cursor for m in models]), where, seeds)
    ring = b["rng_rep"].cpu().numpy().view(np.uint32)
    img = np.stack([m.ring_image() for m in models])
    bad = np.nonzero((ring != img).any(1))[0]
    if bad.size:
        i = int(bad[0])
        raise AssertionError("ring differs %s in %d environments %s (seeds %s); environment %d: cursor %d, slots %s"
                             % (where, bad.size, bad[:8].tolist(), [seeds[j] for j in bad[:8]], i, models[i].cursor, np.nonzero(ring[i] != img[i])[0].tolist()))
    assert env.check_status() == 0, where


def _run_on(env, models, seeds, has_pos):
    """reset() until every environment has consumed at least 624 more words (two calls for most shapes), the models alongside; then
    the cursor position and the ring again."""
    start = [m.words for m in models]
    calls = 0
    pos = np.zeros((len(models), 2), np.int64)
    while min(m.words - s for m, s in zip(models, start)) < sm.MT_N:
        env.reset()
        for i, m in enumerate(models):
            d = m.reset()[2]
            if d is not None:
                pos[i] = d[3:]
        calls += 1
        assert calls <= 400
    if has_pos:
        _same("cursor position", env._bufs["pos"].cpu().numpy().astype(np.int64), pos, "after %d more reset() calls" % calls, seeds)
    _check_ring(env, models, "a lap of the ring later (%d reset() calls)" % calls, seeds)


def _steps(case, tr, env, t0=0, t1=None):
    """step() through the tape of trace `tr` from t0 to t1, everything compared after every step."""
    S, seeds = _stacked(tr), tr["seeds"]
    acts = tr["acts"]
    keys = list(env._prob.info_keys) + ["iterations", "changes"]
    for t in range(t0, len(acts) if t1 is None else t1):
        where = "at step %d (%s)" % (t, case.name)
        obs, rew, done, info = env.step(acts[t] if acts.shape[2] > 1 else acts[t, :, 0])
        _same("done", done.cpu().numpy() != 0, S["done"][t], where, seeds)
        _same("info", _info_cols(info, keys), S["info"][t], where, seeds)
        _same("reward", rew.cpu().numpy(), S["reward"][t], where, seeds)
        _check_state(env, S, t, tr["cursor"][t], where, seeds, env._rep.has_pos)
        assert env.check_status() == 0, where


def _start(case, tr):
    env = _make(case, tr["seeds"])
    for _ in range(1 + case.pre):
        env.reset()
    _same("map", env._bufs["map"].cpu().numpy(), _stacked(tr)["map0"], "after reset()", tr["seeds"])
    _same("ring cursor", env._bufs["rng_cursor"][:, 0].cpu().numpy(), tr["cursor0"], "after reset()", tr["seeds"])
    return env


def _step_case(name):
    case = sm.CASE[name]
    tr = sm.case_trace(name)
    env = _start(case, tr)
    try:
        _steps(case, tr, env)
        models = [m.clone() for m in tr["models"]]
        _check_ring(env, models, "at the end of the tape", tr["seeds"])
        _run_on(env, models, tr["seeds"], env._rep.has_pos)
    finally:
        env.close()


# ------------------------------------------------------------------ reset() called repeatedly, behind the tape as one rollout()
@pytest.mark.parametrize("name", [c.name for c in sm.CASES])
def test_rollout_then_reset_calls(name):
    """The tape as one rollout() (the rows of reward, done and info, then map, cursor position, heat map and ring at its end), then
    reset() RESET_CALLS times -- at the end of a tape the ring cursors of the environments have drifted apart and a dozen calls take
    them through the wrap classes --: map, cursor position and ring cursor after every call; the ring at the end and a lap later."""
    import torch
    case = sm.CASE[name]
    tr, rs = sm.case_trace(name), sm.case_resets(name)
    S, seeds = _stacked(tr), tr["seeds"]
    env = _start(case, tr)
    try:
        acts = tr["acts"]
        T, E = acts.shape[:2]
        keys = list(env._prob.info_keys) + ["iterations", "changes"]
        rew, done, info = env.rollout(torch.as_tensor(acts if acts.shape[2] > 1 else acts[:, :, 0], device=env.device))
        got_info = np.stack([info[k].view(T, E).cpu().numpy() for k in keys], 2).astype(np.int64)
        rew, done = rew.cpu().numpy(), done.cpu().numpy() != 0
        for t in range(T):
            where = "in row %d of the rollout (%s)" % (t, name)
            _same("done", done[t], S["done"][t], where, seeds)
            _same("info", got_info[t], S["info"][t], where, seeds)
            _same("reward", rew[t], S["reward"][t], where, seeds)
        _check_state(env, S, T - 1, tr["cursor"][T - 1], "at the end of the rollout (%s)" % name, seeds, env._rep.has_pos)
        _check_ring(env, tr["models"], "at the end of the rollout", seeds)
        for k in range(len(rs["rst"])):
            where = "after reset() call %d behind the tape (%s)" % (k, name)
            env.reset()
            _same("map", env._bufs["map"].cpu().numpy(), rs["maps"][k], where, seeds)
            if env._rep.has_pos:
                _same("cursor position", env._bufs["pos"].cpu().numpy().astype(np.int64), rs["pos"][k], where, seeds)
            _same("ring cursor", env._bufs["rng_cursor"][:, 0].cpu().numpy(), rs["cursor"][k], where, seeds)
            assert int(env._bufs["heatmap"].abs().sum()) == 0 and int(env._bufs["counters"].abs().sum()) == 0, where
        models = [m.clone() for m in rs["models"]]
        _check_ring(env, models, "after the reset() calls", seeds)
        _run_on(env, models, seeds, env._rep.has_pos)
    finally:
        env.close()


# ------------------------------------------------------------------ step() on the fused kernel
@pytest.mark.parametrize("pair", [0, 1])
@pytest.mark.parametrize("name", FUSED)
def test_fused_step(name, pair, monkeypatch):
    """k_step: the draw cache and its fallback, certain resets that draw the step's cursor move themselves (step_draws), episode ends
    nobody foresaw (pend), all in one launch.  step_pair = 1: two certain resets a wavefront from one staging area (zelda)."""
    _tune(monkeypatch, "step_pair", pair)
    _step_case(name)


# ------------------------------------------------------------------ k_update + k_stats
@pytest.mark.parametrize("name", FUSED)
def test_two_launch_step(name, monkeypatch):
    """no_fused = 1, pair_min = 1: k_update's six speculative draws and its fallback; k_stats' resets, certain (paired) and unforeseen,
    with partial staging where the shape allows it."""
    _tune(monkeypatch, "no_fused", 1)
    _tune(monkeypatch, "pair_min", 1)
    _step_case(name)


# ------------------------------------------------------------------ the other step kernels
@pytest.mark.parametrize("name", OTHER)
def test_step_other_kernels(name):
    """Tall binary maps (k_stats_wide: block_reset_env, narrow and wide), maps beyond 64 columns (k_big), the search problems
    (k_step_solver) and smb (k_smb), narrow: k_update's draws in front of each."""
    _step_case(name)


@pytest.mark.parametrize("name", SOLVER)
def test_search_ticks(name):
    """tick() with a small pop budget: an environment takes its next action only when its search is through, so every environment ends
    up with a tape of its own -- the actions it took.  The oracle and the model are put through those afterwards: every completed
    step's outputs, then ring cursor and ring."""
    import parity_harness as ph
    import torch
    case = sm.CASE[name]
    seeds = sm.seeds_of(case)[:128]
    E, ticks = len(seeds), 30
    acts = sm.case_actions(case, seeds, T=ticks)
    env = _make(case, seeds)
    try:
        env.reset()
        assert env.enable_async(8), "no asynchronous form for this configuration"
        keys = list(env._prob.info_keys) + ["iterations", "changes"]
        ti = torch.arange(E, device=env.device)
        taken, got = [[] for _ in range(E)], [[] for _ in range(E)]
        pending = np.zeros(E, bool)
        for t in range(ticks):
            _obs, _rew, _done, _info, pend = env.tick(acts[t, :, 0], pop_budget=4)
            after = pend.cpu().numpy() != 0
            rows = ph._async_rows(env, ti, keys) if not after.all() else None
            for j in range(E):
                if not pending[j]:
                    taken[j].append(acts[t, j])
                if not after[j]:
                    got[j].append(tuple(x[j] for x in rows))
            pending = after
        env.flush()
        rows = ph._async_rows(env, ti, keys)
        for j in np.nonzero(pending)[0]:
            got[j].append(tuple(x[j] for x in rows))
        models = []
        for j in range(E):
            tr = sm.trace_steps(case, seeds=[seeds[j]], acts=np.asarray(taken[j])[:, None, :])
            x = tr["exp"][0]
            assert len(got[j]) == len(taken[j])
            for k, (rew_k, done_k, info_k, pos_k, heat_k, map_k) in enumerate(got[j]):
                where = (name, "seed", seeds[j], "its step", k)
                assert rew_k == x["reward"][k] and bool(done_k) == bool(x["done"][k]), ("reward / done",) + where
                assert np.array_equal(info_k, x["info"][k]), ("info",) + where
                assert np.array_equal(pos_k, x["pos"][k]) and np.array_equal(map_k, x["maps"][k]), ("cursor position / map",) + where
                assert np.array_equal(heat_k, x["heatmap"][k].astype(np.int64)), ("heat map",) + where
            models.append(tr["models"][0])
        _check_ring(env, models, "after %d ticks and flush()" % ticks, seeds)
        _run_on(env, models, seeds, True)
    finally:
        env.close()


# ------------------------------------------------------------------ the draw cache dropped in the middle of a tape
TAG_CASES = ["binary-narrow-9x9", "zelda-narrow-5x5", "binary-narrow-33x2"]


@pytest.mark.parametrize("name", TAG_CASES)
def test_seed_in_the_middle_of_a_tape(name):
    """seed() with new seeds twice under running episodes: the next cache draw of every environment finds fifo_tag != cursor and makes
    its eight words from the new ring (cursor 0: the words 397 on are old ones of the same ring)."""
    case = sm.CASE[name]
    seeds = sm.seeds_of(case)[:128]
    T = 24
    reseed = {7: [s + 10 ** 6 for s in seeds], 16: [s + 2 * 10 ** 6 for s in seeds]}
    tr = sm.trace_steps(case, seeds=seeds, acts=sm.case_actions(case, seeds, T=T), reseed=reseed)
    tags = sm.census(case, "fused", tr=tr).get("TAG", [])
    assert len(set(tags)) >= len(seeds) // 2, "the first draw after seed() comes out of the cache in most environments"
    env = _start(case, tr)
    try:
        t0 = 0
        for t1 in sorted(reseed) + [T]:
            _steps(case, tr, env, t0, t1)
            if t1 in reseed:
                env.seed(reseed[t1])
            t0 = t1
        models = [m.clone() for m in tr["models"]]
        _check_ring(env, models, "at the end of the tape", seeds)
        _run_on(env, models, seeds, True)
    finally:
        env.close()


@pytest.mark.parametrize("name", TAG_CASES)
def test_load_state_dict_in_the_middle_of_a_tape(name):
    """state_dict() after 9 steps, 5 steps of other actions, load_state_dict(): rings and cursors are those of step 9 again while the
    draw caches were made for the steps in between (load_state_dict drops them).  The tape goes on from step 9 as if nothing happened."""
    case = sm.CASE[name]
    seeds = sm.seeds_of(case)[:128]
    T = 24
    acts = sm.case_actions(case, seeds, T=T)
    tr = sm.trace_steps(case, seeds=seeds, acts=acts)
    env = _start(case, tr)
    try:
        _steps(case, tr, env, 0, 9)
        sd = env.state_dict()
        cur9 = env._bufs["rng_cursor"].clone()
        junk = sm.case_actions(case, [s + 77 for s in seeds], T=5)
        for t in range(5):
            env.step(junk[t, :, 0])
        assert not bool((env._bufs["rng_cursor"] == cur9).all())
        env.load_state_dict(sd)
        _steps(case, tr, env, 9, T)
        models = [m.clone() for m in tr["models"]]
        _check_ring(env, models, "at the end of the tape", seeds)
        _run_on(env, models, seeds, True)
    finally:
        env.close()
