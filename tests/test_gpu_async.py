"""pcgrl_step_async (include/pcgrl_hip.h; csrc/kernels_search_async.h) against the CPU oracle: asynchronous ticks with pop
budgets small enough that most searches are suspended -- several times -- before they finish, slots running out, ticks mixed
with lockstep steps on one handle.  Per environment the taken actions and the outputs of the completed steps must be the
oracle's, bit for bit (tests/parity_harness.py async_case).  GPU only."""
import numpy as np
import pytest

import parity_harness as ph

pytestmark = pytest.mark.gpu

FEW_SOK = dict(probs={"empty": 0.75, "solid": 0.1, "player": 0.02, "crate": 0.07, "target": 0.06})


@pytest.mark.parametrize("prob,rep,calls,E,ticks,budget,nslots", [
    ("sokoban", "narrow", (), 512, 120, 24, 256),                                        # the BASELINE shape (C4), tiny budget
    ("sokoban", "narrow", (dict(width=7, height=6), FEW_SOK), 256, 120, 16, 256),         # levels of 72 bordered cells (four-word sets), open maps: long searches
    ("sokoban", "wide", (dict(width=6, height=6), dict(solver_power=700), FEW_SOK), 200, 100, 40, 64),
    ("sokoban", "turtle", (), 300, 150, 7, 256),
    ("mdungeon", "narrow", (), 256, 100, 24, 256),
    ("mdungeon", "wide", (dict(solver_power=900),), 128, 100, 4, 64),
    ("ddave", "narrow", (), 256, 100, 5, 256),
    ("ddave", "turtle", (dict(solver_power=1200),), 128, 100, 3, 64),
])
def test_async_ticks_vs_oracle(prob, rep, calls, E, ticks, budget, nslots):
    import zlib
    rs = np.random.RandomState(zlib.crc32(("%s %s %d" % (prob, rep, E)).encode()))
    cnt = ph.async_case(prob, rep, list(calls), E, ticks, 4242, rs, budget, nslots)
    few = prob != "sokoban"       # (planners that usually win within a few pops: little to cut even with a budget of 3)
    assert cnt["suspended"] > (3 if few else 10), cnt     # searches really were cut
    assert cnt["late"] >= (1 if few else 3) and cnt["pending_env_ticks"] > (3 if few else 10), cnt
    assert cnt["consumed"] == cnt["steps"], cnt       # the library's count of taken actions is the harness's


def test_async_slot_overflow_and_lockstep_mix():
    """Two slots for hundreds of environments: most suspensions find no slot and run to their end inside the tick (still exact);
    every seventh tick is a flush + lockstep step on the same handle."""
    rs = np.random.RandomState(11)
    cnt = ph.async_case("sokoban", "narrow", [dict(width=6, height=6), FEW_SOK], 384, 90, 77, rs, 12, 2, flush_every=7)
    assert cnt["overflow"] > 3 and cnt["suspended"] > 3, cnt


def test_async_budget_invariance():
    """The same actions, taken by every environment in the same order, whatever the budget: a huge budget is lockstep."""
    rs = np.random.RandomState(5)
    cnt = ph.async_case("sokoban", "narrow", [], 256, 60, 99, rs, 10 ** 6, 16, tuning={"async_split": 0})
    assert cnt["suspended"] == 0 and cnt["overflow"] == 0, cnt
    # (the only environments that ever sit a tick out are those whose search ended their episode: they are reset by the next tick)
    assert cnt["steps"] + cnt["pending_env_ticks"] == 256 * 60, cnt


def test_async_no_form_falls_back_to_step():
    import torch
    from gym_pcgrl_amd.envs import BatchedPcgrlEnv
    env = BatchedPcgrlEnv(prob="binary", rep="narrow", num_envs=64, seed=1)
    env.reset()
    assert env.enable_async() is False
    o, r, d, i, pend = env.tick(torch.zeros(64, dtype=torch.int32, device="cuda"))
    assert not pend.any()
    env.close()


@pytest.mark.parametrize("prob,budget,split", [("sokoban", 20, 0), ("mdungeon", 6, 1), ("ddave", 6, 1)])
def test_async_other_launch_form(prob, budget, split):
    """pcgrl_tuning async_split: every job of a tick -- fresh and suspended -- in ONE launch with the full search region (0: the default
    of mdungeon / ddave), or the fresh jobs in a launch of their own with small regions, what it suspends re-hashed into the full
    table by the launch that continues it (1: sokoban's default).  Here: the form that is NOT the problem's default."""
    rs = np.random.RandomState(21)
    cnt = ph.async_case(prob, "narrow", [], 256, 80, 909, rs, budget, 128, tuning={"async_split": split})
    assert cnt["suspended"] > 3, cnt


def test_async_small_launch_budget_beyond_its_region():
    """A pop budget beyond what the small launch's regions hold (ASYNC_SMALL_POPS = 128): fresh jobs are cut at 128 there and go on
    with the full budget from the next tick."""
    rs = np.random.RandomState(22)
    cnt = ph.async_case("sokoban", "narrow", [dict(width=6, height=6), FEW_SOK], 256, 60, 313, rs, 700, 256)
    assert cnt["suspended"] > 10, cnt


@pytest.mark.parametrize("env_id,rep", [("sokoban-narrow-v0", "narrow"), ("sokoban-wide-v0", "wide"), ("mdungeon-narrow-v0", "narrow")])
def test_async_collector_holds_the_lockstep_transitions(env_id, rep):
    """RolloutCollector.collect(policy, pop_budget=...) -- the trainer-shaped loop (utils.make_vec_envs + the image wrappers) on
    asynchronous ticks, with a policy that is a deterministic function of the image: per environment, the rows flagged `took` /
    `fresh` must be, in order, exactly the (action, reward, done) transitions of the lockstep collector on a twin batch."""
    import torch
    from gym_pcgrl_amd.rollout import RolloutCollector
    from gym_pcgrl_amd.utils import make_vec_envs
    N, T_lock, T_tick = 384, 24, 40
    kw = dict(change_percentage=0.6) if "sokoban" in env_id else {}
    n_act = None

    def policy(obs):
        flat = obs.reshape(obs.shape[0], -1).to(torch.int64)
        w = torch.arange(1, flat.shape[1] + 1, device=obs.device, dtype=torch.int64) % 97 + 1
        return (flat * w).sum(1) % n_act

    out = []
    for budget in (None, 6):
        venv = make_vec_envs(env_id, rep, n_cpu=N, seed=11, device="cuda:0", **kw)
        a = venv.action_space
        n_act = int(a.n) if hasattr(a, "n") else None
        assert n_act is not None
        col = RolloutCollector(venv, T_lock if budget is None else T_tick)
        b = col.collect(policy, pop_budget=budget)
        torch.cuda.synchronize()
        out.append({k: v.cpu().numpy() for k, v in b.as_dict().items() if k in ("actions", "rewards", "dones", "took", "fresh")})
        venv.close()
    lock, asy = out
    assert lock["took"].all() and lock["fresh"].all()
    assert (~asy["fresh"]).sum() > 10               # environments really sat ticks out
    # rows in which no step completed carry reward 0 / done False: summing the reward rows of an environment gives the
    # sum over its completed steps, with or without looking at `fresh`
    assert (asy["rewards"][~asy["fresh"]] == 0).all() and not asy["dones"][~asy["fresh"]].any()
    short = 0
    for e in range(N):
        acts = asy["actions"][asy["took"][:, e], e]
        rew = asy["rewards"][asy["fresh"][:, e], e]
        done = asy["dones"][asy["fresh"][:, e], e]
        k = min(len(rew), T_lock)
        short += int(len(rew) < T_tick)
        assert np.array_equal(acts[:k], lock["actions"][:k, e]), ("actions", e)
        assert np.array_equal(rew[:k], lock["rewards"][:k, e]) and np.array_equal(done[:k], lock["dones"][:k, e]), ("reward/done", e)
    assert short > 0          # (an environment with a long search completes fewer steps than there were ticks)


def test_async_ticks_through_the_node_driver_and_a_checkpoint():
    """MultiGpuPcgrlEnv.tick (a handle and a stream per shard: here four on this box's one GPU) gives every environment what one
    batch's tick gives it; state_dict() finishes the steps in flight first, and a batch restored from it goes on like the original."""
    import torch
    from gym_pcgrl_amd.envs import BatchedPcgrlEnv
    from gym_pcgrl_amd.node import MultiGpuPcgrlEnv
    n = 400
    one = BatchedPcgrlEnv(prob="sokoban", rep="narrow", num_envs=n, seed=5)
    node = MultiGpuPcgrlEnv(prob="sokoban", rep="narrow", num_envs=n, devices=["cuda:0"] * 4, seed=5)
    one.reset(); node.reset()
    assert one.enable_async(64) and node.enable_async(64)
    rs = np.random.RandomState(2)
    for t in range(50):
        a = torch.as_tensor(rs.randint(0, 6, size=n).astype(np.int32), device="cuda")
        o1, r1, d1, i1, p1 = one.tick(a, pop_budget=9)
        o2, r2, d2, i2, p2 = node.tick(a, pop_budget=9)
        p2 = p2.to("cuda:0")
        assert torch.equal(p1, p2), t
        ok = p1 == 0
        assert torch.equal(r1[ok], r2.to("cuda:0")[ok]) and torch.equal(d1[ok], d2.to("cuda:0")[ok]) and torch.equal(o1["map"][ok], o2["map"].to("cuda:0")[ok]), t
    assert int((one._async["pending"] != 0).sum()) > 0
    sd = one.state_dict()                              # flushes
    assert int((one._async["pending"] != 0).sum()) == 0
    twin = BatchedPcgrlEnv(prob="sokoban", rep="narrow", num_envs=n, seed=5)
    twin.reset()
    twin.load_state_dict(sd)
    for t in range(20):
        a = rs.randint(0, 6, size=n).astype(np.int32)
        _, ra, da, _ = one.step(a)
        _, rb, db, _ = twin.step(a)
        assert torch.equal(ra, rb) and torch.equal(da, db) and torch.equal(one._bufs["map"], twin._bufs["map"]), t
    one.close(); node.close(); twin.close()


def test_make_vec_envs_async_ticks_gives_the_lockstep_transitions_per_environment():
    """the asynchronous form behind the reference-shaped surface -- make_vec_envs(..., async_ticks=budget).step()
    returns the usual four values, `infos.took` / `infos.fresh` say who acted and who completed a step; per environment the
    (took action -> fresh outcome) pairs are bitwise the transitions of the lockstep environment, and reward / done are zero in the
    calls an environment sat out."""
    import torch
    from gym_pcgrl_amd.utils import make_vec_envs
    N, T_lock, T_tick = 320, 20, 36
    n_act = None

    def policy(obs):
        flat = obs.reshape(obs.shape[0], -1).to(torch.int64)
        w = torch.arange(1, flat.shape[1] + 1, device=obs.device, dtype=torch.int64) % 89 + 1
        return (flat * w).sum(1) % n_act

    rec = []
    for budget in (None, 5):
        venv = make_vec_envs("sokoban-narrow-v0", "narrow", n_cpu=N, seed=23, device="cuda:0", monitor=True, async_ticks=budget, change_percentage=0.6)
        n_act = int(venv.action_space.n)
        obs = venv.reset()
        rows = dict(a=[], r=[], d=[], took=[], fresh=[], ep=[])
        for t in range(T_lock if budget is None else T_tick):
            a = policy(obs)
            obs, rew, done, infos = venv.step(a)
            rows["a"].append(a.cpu().numpy()); rows["r"].append(rew.cpu().numpy()); rows["d"].append(done.cpu().numpy())
            if budget is None:
                assert not hasattr(infos, "took")
                rows["took"].append(np.ones(N, bool)); rows["fresh"].append(np.ones(N, bool))
            else:
                rows["took"].append(infos.took.cpu().numpy()); rows["fresh"].append(infos.fresh.cpu().numpy())
            rows["ep"].append(dict(getattr(infos, "episodes", {})))
        rec.append({k: (np.stack(v) if k != "ep" else v) for k, v in rows.items()})
        venv.close()
    lock, asy = rec
    assert (~asy["fresh"]).sum() > 10 and (asy["r"][~asy["fresh"]] == 0).all() and not asy["d"][~asy["fresh"]].any()
    n_eps = 0
    for e in range(N):
        acts = asy["a"][asy["took"][:, e], e]
        rew, done = asy["r"][asy["fresh"][:, e], e], asy["d"][asy["fresh"][:, e], e]
        k = min(len(rew), T_lock)
        assert np.array_equal(acts[:k], lock["a"][:k, e]) and np.array_equal(rew[:k], lock["r"][:k, e]) and np.array_equal(done[:k], lock["d"][:k, e]), e
        # Monitor's episode entries come with the call in which the episode's last step completed, and are the lockstep ones
        eps_l = [lock["ep"][t][e] for t in range(T_lock) if e in lock["ep"][t]]
        eps_a = [asy["ep"][t][e] for t in range(T_tick) if e in asy["ep"][t]]
        m = min(len(eps_l), len(eps_a))
        assert eps_a[:m] == eps_l[:m], e
        n_eps += m
    assert n_eps > 0


def _pairs(took, fresh, a, r, d):
    """One environment's calls -> its (action, reward, done) transitions in order; a step whose outcome no call reported (a flush
    between two calls finished it: a `took` call followed by another `took` call with no `fresh` one in between) gets None."""
    out, open_ = [], None
    for t in range(len(took)):
        if took[t]:
            if open_ is not None:
                out.append((open_, None, None))
            open_ = a[t]
        if fresh[t]:
            out.append((open_, r[t], d[t]))
            open_ = None
    return out


def _check_flushed_run(lock, asy, n_flushed_min=1):
    """Per environment the asynchronous run's transitions (with dropped outcomes) against the lockstep ones."""
    dropped = 0
    for e in range(lock["a"].shape[1]):
        pairs = _pairs(asy["took"][:, e], asy["fresh"][:, e], asy["a"][:, e], asy["r"][:, e], asy["d"][:, e])
        k = min(len(pairs), len(lock["a"]))
        for j in range(k):
            act, rew, done = pairs[j]
            assert act == lock["a"][j, e], ("action", e, j)
            if rew is None:
                dropped += 1
            else:
                assert rew == lock["r"][j, e] and done == lock["d"][j, e], ("outcome", e, j)
    assert dropped >= n_flushed_min, dropped


def test_make_vec_envs_async_ticks_across_a_flush():
    """adjust_param() with an unchanged value in the middle of an asynchronous run flushes the steps in flight.  The environments
    that had one take their action at the next call (`took`: read from the live pending state), the flushed steps' outcomes are
    dropped -- a `took` call followed by another `took` call -- and per environment the transitions are still the lockstep ones."""
    import torch
    from gym_pcgrl_amd.utils import make_vec_envs
    N, T_lock, T_tick, t_flush = 64, 24, 40, 6

    def policy(obs, n_act):
        flat = obs.reshape(obs.shape[0], -1).to(torch.int64)
        w = torch.arange(1, flat.shape[1] + 1, device=obs.device, dtype=torch.int64) % 89 + 1
        return (flat * w).sum(1) % n_act

    rec = []
    for budget in (None, 4):
        venv = make_vec_envs("sokoban-narrow-v0", "narrow", n_cpu=N, seed=29, device="cuda:0", async_ticks=budget, change_percentage=0.6)
        n_act = int(venv.action_space.n)
        obs = venv.reset()
        rows = dict(a=[], r=[], d=[], took=[], fresh=[])
        flushed, t_flushed = 0, None
        for t in range(T_lock if budget is None else T_tick):
            if budget is not None and t >= t_flush and t_flushed is None and not rows["fresh"][-1].all():   # the first call after t_flush
                pend = venv.env.pcgrl_env._async["pending"].cpu().numpy()                                  # with steps in flight
                flushed, t_flushed = int((pend != 0).sum()), t
                venv.env.adjust_param(change_percentage=0.6)          # unchanged: only the flush
                assert not venv.env.pcgrl_env._async["pending"].any()
            a = policy(obs, n_act)
            obs, rew, done, infos = venv.step(a)
            rows["a"].append(a.cpu().numpy()); rows["r"].append(rew.cpu().numpy()); rows["d"].append(done.cpu().numpy())
            rows["took"].append(infos.took.cpu().numpy() if budget else np.ones(N, bool))
            rows["fresh"].append(infos.fresh.cpu().numpy() if budget else np.ones(N, bool))
        rec.append({k: np.stack(v) for k, v in rows.items()})
        venv.close()
    assert flushed > 0, "nothing was in flight at the flush"
    lock, asy = rec
    assert asy["took"][t_flushed].sum() >= flushed
    _check_flushed_run(lock, asy, flushed)


def test_async_collector_across_a_flush():
    """RolloutCollector.collect(policy, pop_budget=4) with adjust_param() (unchanged value: a flush) called by the policy in the middle
    of the rollout: `took` comes from the live pending state, the flushed steps' outcomes are dropped, and per environment the
    transitions are the lockstep collector's."""
    import torch
    from gym_pcgrl_amd.rollout import RolloutCollector
    from gym_pcgrl_amd.utils import make_vec_envs
    N, T_lock, T_tick, t_flush = 64, 24, 40, 6
    out, flushed = [], [0]
    for budget in (None, 4):
        venv = make_vec_envs("sokoban-narrow-v0", "narrow", n_cpu=N, seed=31, device="cuda:0", change_percentage=0.6)
        n_act = int(venv.action_space.n)
        calls = [0]

        def policy(obs):
            if budget is not None and calls[0] == t_flush:
                flushed[0] = int((venv.env.pcgrl_env._async["pending"] != 0).sum().item())
                venv.env.adjust_param(change_percentage=0.6)           # unchanged: only the flush (finishes the images of obs too)
            calls[0] += 1
            flat = obs.reshape(obs.shape[0], -1).to(torch.int64)
            w = torch.arange(1, flat.shape[1] + 1, device=obs.device, dtype=torch.int64) % 97 + 1
            return (flat * w).sum(1) % n_act
        col = RolloutCollector(venv, T_lock if budget is None else T_tick)
        b = col.collect(policy, pop_budget=budget)
        torch.cuda.synchronize()
        d = {k: v.cpu().numpy() for k, v in b.as_dict().items() if k in ("actions", "rewards", "dones", "took", "fresh")}
        out.append(dict(a=d["actions"], r=d["rewards"], d=d["dones"], took=d["took"], fresh=d["fresh"]))
        venv.close()
    assert flushed[0] > 0, "nothing was in flight at the flush"
    _check_flushed_run(out[0], out[1], flushed[0])
