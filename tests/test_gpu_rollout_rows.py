"""The step kernels write the rollout row (pcgrl_bind_row; RolloutCollector(kernel_rows=True)): held against the collector's loop of
small copies (kernel_rows=False) on a twin batch -- same seeds, a policy that is a pure function of the observation, two consecutive
rollouts -- bit for bit: every tensor of the buffer, the Monitor columns (float columns as int64: NaN patterns count) and the
environments' own state afterwards.  One case per pipeline that writes rows: the fused k_step (its row-writing instantiations, all
block sizes, the flat-index path), k_update + k_stats, k_stats_wide, k_big, the lockstep searches, k_smb, k_update_block (action widths 2
and 9), and the asynchronous ticks behind k_update and behind k_update_block."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _policy_for(torch, space):
    nvec = None if hasattr(space, "n") else torch.as_tensor(np.asarray(space.nvec), dtype=torch.int64, device="cuda:0")

    def policy(obs):
        flat = obs.reshape(obs.shape[0], -1).to(torch.int64)
        w = torch.arange(1, flat.shape[1] + 1, device=obs.device, dtype=torch.int64) % 97 + 1
        h = (flat * w).sum(1)
        if nvec is None:
            return h % int(space.n)
        return (h[:, None] * (torch.arange(nvec.numel(), device=obs.device, dtype=torch.int64) * 2 + 3)) % nvec[None, :]
    return policy


def _policy_by_digits(torch, space):
    """For the (type, value) action spaces: _policy_for's multipliers 3 and 5 leave a type below 3 or 6 at 0 (or 3) and a value below 5
    at 0 -- no block is ever written.  Here every column is its own digit of the hash, so every type and value occurs."""
    nvec = torch.as_tensor(np.asarray(space.nvec), dtype=torch.int64, device="cuda:0")
    div = torch.as_tensor([7 ** i for i in range(nvec.numel())], dtype=torch.int64, device="cuda:0")

    def policy(obs):
        flat = obs.reshape(obs.shape[0], -1).to(torch.int64)
        w = torch.arange(1, flat.shape[1] + 1, device=obs.device, dtype=torch.int64) % 97 + 1
        return ((flat * w).sum(1)[:, None] // div[None, :]) % nvec[None, :]
    return policy


def _collect_twins(env_id, rep, N, T, monitor, pop_budget=None, nslots=None, kw=None, policy_for=None):
    """-> per kernel_rows in (True, False): the snapshots of two consecutive rollouts and of the environments' state afterwards."""
    import torch
    from gym_pcgrl_amd.rollout import RolloutCollector
    from gym_pcgrl_amd.utils import make_vec_envs
    out = []
    for rows in (True, False):
        venv = make_vec_envs(env_id, rep, n_cpu=N, seed=11, device="cuda:0", monitor=monitor, **(kw or {}))
        e = venv.env.pcgrl_env
        if nslots is not None:
            assert e.enable_async(nslots)
        col = RolloutCollector(venv, T, kernel_rows=rows)
        assert col.kernel_rows is rows
        policy = (policy_for or _policy_for)(torch, venv.action_space)
        snap = {"direct": col.direct}
        for r in range(2):
            b = col.collect(policy, pop_budget=pop_budget)
            torch.cuda.synchronize()
            for k, v in b.as_dict().items():
                snap["%d/%s" % (r, k)] = v.clone()
            if monitor:
                assert len(col.episode_returns) == len(col.episode_lengths) == T
                snap["%d/episode_returns" % r] = torch.stack(col.episode_returns).view(torch.int64).clone()
                snap["%d/episode_lengths" % r] = torch.stack(col.episode_lengths).clone()
        for k in ("map", "counters", "reward", "done", "info"):
            snap["env/" + k] = e._bufs[k].clone()
        if monitor:
            for k, v in e.episode_stats().items():
                snap["env/" + k] = v.view(torch.int64).clone() if v.dtype == torch.float64 else v.clone()
        out.append(snap)
        venv.close()
    return out


def _assert_same(rows, copies):
    import torch
    assert rows.keys() == copies.keys()
    for k in rows:
        if k == "direct":
            assert rows[k] == copies[k]
            continue
        a, b = rows[k], copies[k]
        if a.dtype == torch.float64:
            a, b = a.view(torch.int64), b.view(torch.int64)
        assert a.dtype == b.dtype and torch.equal(a, b), k


# ---- the fused k_step: no extra launch, the row from the block's LDS copy
@pytest.mark.parametrize("epb", [64, 128, 256])
@pytest.mark.parametrize("monitor", [True, False])
@pytest.mark.parametrize("N", [192, 100])
@pytest.mark.parametrize("env_id,rep,kw", [("binary-narrow-v0", "narrow", {}), ("zelda-wide-v0", "wide", dict(width=11, height=16))])
def test_fused_step_writes_the_row(monkeypatch, env_id, rep, kw, N, monitor, epb):
    from gym_pcgrl_amd import _lib
    monkeypatch.setitem(_lib.TUNING_OVERRIDES, "step_epb", epb)
    rows, copies = _collect_twins(env_id, rep, N, 12, monitor, kw=kw)
    _assert_same(rows, copies)


# ---- every other lockstep pipeline: one small kernel behind the step
@pytest.mark.parametrize("env_id,rep,N,T,kw,tune", [
    ("zelda-narrow-v0", "narrow", 192, 10, {}, {"no_fused": 1}),                      # k_update + k_stats
    ("binary-turtle-v0", "turtle", 96, 8, dict(width=64, height=64), {}),             # k_stats_wide
    ("binary-narrow-v0", "narrow", 8, 6, dict(width=80, height=72), {}),              # k_big
    ("sokoban-narrow-v0", "narrow", 64, 10, dict(change_percentage=0.6), {}),         # the lockstep searches
    ("smb-narrow-v0", "narrow", 8, 6, {}, {}),                                        # k_smb
    ("binary-narrowcast-v0", "narrowcast", 100, 8, {}, {}),                           # action width 2: the int64 stride
    ("zelda-narrowmulti-v0", "narrowmulti", 100, 8, {}, {}),                          # action width 9
    ("zelda-wide-v0", "wide", 100, 8, {}, {"no_fused": 1}),                           # flat int64 indices: k_action_map, then k_row takes them as the column
    ("binary-narrow-v0", "narrow", 100, 10, dict(width=40, height=14), {}),           # 64-bit row masks: k_step's row-writing instantiation for them
    ("binary-wide-v0", "wide", 100, 10, dict(width=40, height=14), {}),               # ... and its flat-index path
])
def test_row_kernel_behind_the_other_pipelines(monkeypatch, env_id, rep, N, T, kw, tune):
    from gym_pcgrl_amd import _lib
    for k, v in tune.items():
        monkeypatch.setitem(_lib.TUNING_OVERRIDES, k, v)
    # (type, value) actions: every type and value, so that blocks are written (_policy_by_digits)
    rows, copies = _collect_twins(env_id, rep, N, T, True, kw=kw, policy_for=_policy_by_digits if rep == "narrowcast" else None)
    _assert_same(rows, copies)
    if rep == "narrowcast":
        a = rows["0/actions"].reshape(-1, 2).cpu().numpy()
        assert set(a[:, 0].tolist()) == {0, 1, 2} and set(a[:, 1].tolist()) == {0, 1}


# ---- asynchronous ticks: took / fresh, zeroed rewards, carried episode starts
def _async_masks(rows):
    cat = lambda k: np.concatenate([rows["0/" + k].cpu().numpy(), rows["1/" + k].cpu().numpy()])
    fresh, took, dones, rewards = cat("fresh"), cat("took"), cat("dones"), cat("rewards")
    assert (~fresh).sum() > 0 and (~took).sum() > 0          # an environment really sat a tick out
    assert dones.any()                                        # an episode really ended
    assert (rewards[~fresh] == 0).all() and not dones[~fresh].any()


@pytest.mark.parametrize("budget,nslots", [(4, 1024), (40, 8)])
@pytest.mark.parametrize("env_id,kw", [("sokoban-narrow-v0", dict(change_percentage=0.6)), ("mdungeon-narrow-v0", {})])
def test_asynchronous_ticks_write_the_row(env_id, kw, budget, nslots):
    """Twin batches, as above.  Only where no search overflows the slots: which of the searches that are cut short in one tick get the
    free slots is decided by a race between blocks, so with overflows two runs of the SAME loop differ in which environment sits
    which tick out (measured: kernel_rows=False against itself, sokoban, 8 slots, budget 4: every column differs; 71 / 68 overflows)
    -- the figures are in profiles/rollout_rows/NOTES.md; that case is held row by row inside one run, below."""
    N, T = 384, 40           # (the sizes of tests/test_gpu_async.py's collector case: searches are suspended, episodes end)
    rows, copies = _collect_twins(env_id, "narrow", N, T, True, pop_budget=budget, nslots=nslots, kw=kw)
    _assert_same(rows, copies)
    _async_masks(rows)


@pytest.mark.parametrize("env_id,rep,kw", [("sokoban-narrowmulti-v0", "narrowmulti", dict(change_percentage=0.6)), ("sokoban-turtlecast-v0", "turtlecast", dict(change_percentage=0.6))])
def test_asynchronous_ticks_write_the_row_block_representations(env_id, rep, kw):
    """The same for the representations of k_update_block (its own copy of the tick's preamble writes `took`): int64 actions of
    width 9 and 2 under ticks.  Slots for every environment, so that no search overflows (see above)."""
    N, T = 384, 40
    rows, copies = _collect_twins(env_id, rep, N, T, True, pop_budget=4, nslots=1024, kw=kw, policy_for=_policy_by_digits if rep == "turtlecast" else None)
    _assert_same(rows, copies)
    _async_masks(rows)
    if rep == "turtlecast":         # the policy really moves and writes: all six types, every tile
        a = rows["0/actions"].reshape(-1, 2).cpu().numpy()
        assert set(a[:, 0].tolist()) == set(range(6)) and set(a[:, 1].tolist()) == set(range(5))


@pytest.mark.parametrize("budget", [4, 40])
@pytest.mark.parametrize("env_id,kw", [("sokoban-narrow-v0", dict(change_percentage=0.6)), ("mdungeon-narrow-v0", {})])
def test_asynchronous_ticks_with_few_slots_row_by_row(env_id, kw, budget):
    """Eight slots (budget 4: the overflow path).  Every row the tick wrote is held, bit for bit, against what the copying loop
    (rollout.py, kernel_rows=False) computes for that same tick from the environment's live tensors."""
    import torch
    from gym_pcgrl_amd.rollout import RolloutCollector
    from gym_pcgrl_amd.utils import make_vec_envs
    N, T = 384, 40
    venv = make_vec_envs(env_id, "narrow", n_cpu=N, seed=11, device="cuda:0", monitor=True, **kw)
    e = venv.env.pcgrl_env
    assert e.enable_async(8)
    col = RolloutCollector(venv, T, kernel_rows=True)
    b = col.buffer
    inner = _policy_for(torch, venv.action_space)
    seen = {}

    def policy(obs):
        seen["took"] = e.async_idle()                 # the pending state right before the tick, as the copying loop reads it
        seen["actions"] = inner(obs)
        return seen["actions"]

    i64 = lambda x: x.view(torch.int64)
    sat_out = ended = 0
    for r in range(2):
        col.begin(budget)
        start = col._start.clone()
        for t in range(T):
            col.step(t, policy, budget)
            fresh = e._async["pending"] == 0
            rew, done, st = e._bufs["reward"], e._bufs["done"].view(torch.bool), e.episode_stats()
            done_ref = done & fresh
            assert torch.equal(b.episode_starts[t], start), (r, t)
            start = torch.where(fresh, done, start)
            assert torch.equal(b.actions[t], seen["actions"]) and torch.equal(b.took[t], seen["took"]) and torch.equal(b.fresh[t], fresh), (r, t)
            assert torch.equal(i64(b.rewards[t]), i64(torch.where(fresh, rew, torch.zeros_like(rew)))) and torch.equal(b.dones[t], done_ref), (r, t)
            assert torch.equal(i64(col.episode_returns[-1]), i64(torch.where(done_ref, st["last_return"], torch.full_like(st["last_return"], float("nan"))))), (r, t)
            assert torch.equal(col.episode_lengths[-1], torch.where(done_ref, st["last_length"], torch.zeros_like(st["last_length"]))), (r, t)
            sat_out += int((~fresh).sum())
            ended += int(done_ref.sum())
        assert torch.equal(col._start, start)         # the last row's episode starts: the carry into the next rollout
    cnt = e.async_counters()
    assert sat_out > 0 and ended > 0 and cnt["suspended"] > 0, cnt
    if budget == 4 and "sokoban" in env_id:          # (MiniDungeons' searches are short: eight slots are enough for them)
        assert cnt["overflow"] > 0, cnt
    venv.close()


def test_rows_that_are_not_16_byte_aligned():
    """Three 5 x 5 binary crops: a row of the observation storage is 75 bytes, so the image is copied -- the small columns are bound all the same."""
    rows, copies = _collect_twins("binary-narrow-v0", "narrow", 3, 10, True, kw=dict(cropped_size=5))
    assert rows["direct"] is False
    _assert_same(rows, copies)


# ---- environment level, no collector
def _status(env):
    st = C.c_int32()
    assert env._lib.pcgrl_status(env._handle, env._stream(), C.byref(st)) == 0
    return st.value


@pytest.mark.parametrize("prob,rep,kw,tune", [("binary", "narrow", {}, {}), ("zelda", "narrow", {}, {"no_fused": 1}),
                                               ("binary", "wide", {}, {}), ("zelda", "narrowmulti", {}, {})])
def test_int64_actions_are_their_low_words(monkeypatch, prob, rep, kw, tune):
    """int64 actions, out-of-range values among them, give the maps and the status word of `actions.to(torch.int32)`."""
    import torch
    from gym_pcgrl_amd import _lib
    from gym_pcgrl_amd.envs import BatchedPcgrlEnv
    for k, v in tune.items():
        monkeypatch.setitem(_lib.TUNING_OVERRIDES, k, v)
    N = 100
    a64 = BatchedPcgrlEnv(prob=prob, rep=rep, num_envs=N, seed=5, device="cuda:0")
    a32 = BatchedPcgrlEnv(prob=prob, rep=rep, num_envs=N, seed=5, device="cuda:0")
    a64.reset(), a32.reset()
    aw = a64._rep.action_width()
    g = torch.Generator().manual_seed(3)
    for t in range(12):
        act = torch.randint(0, 2, (N, aw) if aw > 1 else (N,), generator=g, dtype=torch.int64)
        if t == 5:
            assert _status(a64) == _status(a32) == 0
        if t >= 5:       # out of range: negative, too large, and large values whose low word is a valid action
            act.view(-1)[0::7] = -3
            act.view(-1)[1::7] = 1000
            act.view(-1)[2::7] += 1 << 32
            act.view(-1)[3::7] -= 1 << 40
        act = act.to("cuda:0")
        o64 = a64.step(act)
        o32 = a32.step(act.to(torch.int32))
        assert torch.equal(o64[0]["map"], o32[0]["map"]) and torch.equal(o64[1].view(torch.int64), o32[1].view(torch.int64)) and torch.equal(o64[2], o32[2]), t
    assert _status(a64) == _status(a32) == 2
    for k in ("map", "heatmap", "counters", "info"):
        assert torch.equal(a64._bufs[k], a32._bufs[k]), k
    a64.close(), a32.close()


@pytest.mark.parametrize("prob,tune", [("binary", {}), ("zelda", {"no_fused": 1})])
def test_unbound_row_is_left_alone(monkeypatch, prob, tune):
    import torch
    from gym_pcgrl_amd import _lib
    from gym_pcgrl_amd.envs import BatchedPcgrlEnv
    for k, v in tune.items():
        monkeypatch.setitem(_lib.TUNING_OVERRIDES, k, v)
    N = 100
    env = BatchedPcgrlEnv(prob=prob, rep="narrow", num_envs=N, seed=5, device="cuda:0")
    env.enable_episode_stats()
    env.reset()
    dev = env.device
    cols = dict(actions_out=torch.full((N,), -7, dtype=torch.int64, device=dev), reward=torch.full((N,), -7.0, dtype=torch.float64, device=dev),
                done=torch.full((N,), 7, dtype=torch.uint8, device=dev), start_out=torch.full((N,), 7, dtype=torch.uint8, device=dev),
                ep_return=torch.full((N,), -7.0, dtype=torch.float64, device=dev), ep_length=torch.full((N,), -7, dtype=torch.int32, device=dev),
                took=torch.full((N,), 7, dtype=torch.uint8, device=dev), fresh=torch.full((N,), 7, dtype=torch.uint8, device=dev))
    act = torch.ones(N, dtype=torch.int64, device=dev)
    env.bind_rollout_row(**cols)
    _, rew, done, _ = env.step(act)
    torch.cuda.synchronize()
    assert torch.equal(cols["actions_out"], act) and torch.equal(cols["reward"], rew) and torch.equal(cols["done"], done.view(torch.uint8))
    assert torch.equal(cols["start_out"], cols["done"]) and bool((cols["took"] == 1).all()) and bool((cols["fresh"] == 1).all())
    assert bool((cols["ep_length"] == 0).all()) and bool(torch.isnan(cols["ep_return"]).all())         # no episode ends in its first step
    sentinels = {k: v.clone().fill_(-7 if v.dtype != torch.uint8 else 7) for k, v in cols.items()}
    for k, v in cols.items():
        v.copy_(sentinels[k])
    env.unbind_rollout_row()
    env.step(act)
    env.step(act.to(torch.int32))
    torch.cuda.synchronize()
    for k, v in cols.items():
        assert torch.equal(v, sentinels[k]), k
    env.close()


@pytest.mark.parametrize("prob,kw,tune", [("zelda", {}, {}), ("zelda", {}, {"no_fused": 1}), ("binary", dict(width=40, height=14), {})])
def test_int64_flat_indices_are_their_low_words(monkeypatch, prob, kw, tune):
    """step_flat() with int64 indices, out-of-range values among them (the fused kernel's decode, k_action_map): the maps and the
    status word of the same indices converted to int32."""
    import torch
    from gym_pcgrl_amd import _lib
    from gym_pcgrl_amd.envs import BatchedPcgrlEnv
    for k, v in tune.items():
        monkeypatch.setitem(_lib.TUNING_OVERRIDES, k, v)
    N = 100
    envs = [BatchedPcgrlEnv(prob=prob, rep="wide", num_envs=N, seed=5, device="cuda:0") for _ in range(2)]
    for e in envs:
        e.adjust_param(**kw)
        e.reset()
    a64, a32 = envs
    total = a64._prob._width * a64._prob._height * a64.get_num_tiles()
    xyv = [torch.empty((N, 3), dtype=torch.int32, device="cuda:0") for _ in range(2)]
    g = torch.Generator().manual_seed(4)
    for t in range(10):
        act = torch.randint(0, total, (N,), generator=g, dtype=torch.int64)
        if t == 5:
            assert _status(a64) == _status(a32) == 0
        if t >= 5:
            act[0::7] = -3
            act[1::7] = total + 5
            act[2::7] += 1 << 32
            act[3::7] -= 1 << 40
        act = act.to("cuda:0")
        o64 = a64.step_flat(act, xyv[0])
        o32 = a32.step_flat(act.to(torch.int32), xyv[1])
        assert torch.equal(o64[0]["map"], o32[0]["map"]) and torch.equal(o64[1].view(torch.int64), o32[1].view(torch.int64)) and torch.equal(o64[2], o32[2]), t
    assert _status(a64) == _status(a32) == 2
    for k in ("map", "heatmap", "counters", "info"):
        assert torch.equal(a64._bufs[k], a32._bufs[k]), k
    a64.close(), a32.close()


def test_bind_rollout_row_checks_device_tensors():
    """The argument checks with tensors that ARE on the environment's device -- each bad one refused for its own reason -- and a
    binding that is accepted, whole and in part."""
    import torch
    from gym_pcgrl_amd.envs import BatchedPcgrlEnv
    n = 6
    env = BatchedPcgrlEnv(prob="zelda", rep="narrowcast", num_envs=n, seed=1, device="cuda:0")
    env.reset()
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda:0")
    bad = [("wrong dtype", dict(reward=z((n,), torch.float32))), ("wrong dtype", dict(actions_out=z((n, 2), torch.int32))),
           ("wrong dtype", dict(start_in=z((n,), torch.int8))), ("wrong dtype", dict(ep_return=z((n,), torch.float32))),
           ("wrong shape", dict(actions_out=z((n,), torch.int64))), ("wrong shape", dict(done=z((n + 1,), torch.bool))),
           ("wrong shape", dict(ep_length=z((1, n), torch.int32))),
           ("not contiguous", dict(actions_out=z((n, 4), torch.int64)[:, :2])), ("not contiguous", dict(start_out=z((n, 2), torch.uint8)[:, 1])),
           ("wrong device", dict(fresh=torch.zeros(n, dtype=torch.bool)))]
    for why, cols in bad:
        with pytest.raises(ValueError, match=why):
            env.bind_rollout_row(**cols)
        assert env._row is None
    with pytest.raises(RuntimeError, match="enable_episode_stats"):
        env.bind_rollout_row(ep_length=z((n,), torch.int32))
    env.enable_episode_stats()
    good = dict(actions_out=z((n, 2), torch.int64), reward=z((n,), torch.float64), done=z((n,), torch.bool), start_in=z((n,), torch.uint8),
                start_out=z((n,), torch.bool), ep_return=z((n,), torch.float64), ep_length=z((n,), torch.int32), took=z((n,), torch.uint8), fresh=z((n,), torch.bool))
    env.bind_rollout_row(**good)
    act = torch.ones((n, 2), dtype=torch.int64, device="cuda:0")
    _, rew, done, _ = env.step(act)
    torch.cuda.synchronize()
    assert torch.equal(good["actions_out"], act) and torch.equal(good["reward"], rew) and torch.equal(good["done"], done) and bool(good["fresh"].all())
    env.bind_rollout_row(reward=good["reward"], done=None)            # a part of the columns
    good["done"].fill_(True)
    _, rew, done, _ = env.step(act)
    torch.cuda.synchronize()
    assert torch.equal(good["reward"], rew) and bool(good["done"].all())
    env.close()


def test_int64_reading_does_not_outlive_the_call():
    """A shard of MultiGpuPcgrlEnv stepped once with an int64 tensor, then the node through its one-call step (pcgrl_step_multi:
    raw int32 pointers): the int64 reading of `actions` must be gone from the handle.  Likewise a row bound on a shard: the node
    takes the per-shard path while it is, and the one-call path again afterwards.  Against a twin batch stepped with the same actions."""
    import torch
    from gym_pcgrl_amd.envs import BatchedPcgrlEnv
    from gym_pcgrl_amd.node import MultiGpuPcgrlEnv
    n, G = 400, 4
    one = BatchedPcgrlEnv(prob="binary", rep="narrow", num_envs=n, seed=5, device="cuda:0")
    node = MultiGpuPcgrlEnv(prob="binary", rep="narrow", num_envs=n, devices=["cuda:0"] * G, seed=5)
    one.reset(); node.reset()
    rs = np.random.RandomState(2)
    per = n // G
    col = torch.full((per,), -7.0, dtype=torch.float64, device="cuda:0")

    def same(t):
        torch.cuda.synchronize()
        m = torch.cat([sh._bufs["map"] for sh in node.shards])
        r = torch.cat([sh._bufs["reward"] for sh in node.shards])
        assert torch.equal(m, one._bufs["map"]) and torch.equal(r.view(torch.int64), one._bufs["reward"].view(torch.int64)), t

    for t in range(12):
        a = torch.as_tensor(rs.randint(0, 3, size=n), dtype=torch.int64, device="cuda:0")
        one.step(a.to(torch.int32))
        if t in (2, 6):                    # the shards directly, with contiguous int64 slices
            for g, sh in enumerate(node.shards):
                sh.step(a[g * per:(g + 1) * per])
                assert sh._row_plain()
        else:
            if t == 8:
                node.shards[1].bind_rollout_row(reward=col)
            if t == 10:
                node.shards[1].unbind_rollout_row()
            node.step(a.to(torch.int32) if t % 2 else a)
            assert (node._multi is not None) == (t not in (8, 9)), t
        same(t)
        if t in (8, 9):
            assert torch.equal(col.view(torch.int64), node.shards[1]._bufs["reward"].view(torch.int64))
    one.close(); node.close()
