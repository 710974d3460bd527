"""narrowcast, narrowmulti and turtlecast -- the representations that change up to nine cells per step -- on every stepping route,
against the CPU oracle.  They run through an update kernel of their own, k_update_block (csrc/kernels_update.h): a second copy of
what k_update / update_env do for narrow, wide and turtle (action decoding and clamping, the clipped 3 x 3 write into byte map and
bit planes, the cursor move, the heat map, the unchanged-environment finish, the asynchronous preamble, the routing onto WL_CHG /
WL_RST), and the launch layer branches on `rep <= PCGRL_REP_TURTLE` around it.  Every comparison is parity_harness.run_config /
async_case against the oracle, bit for bit: reward, done, every info key, cursor, heat map, the map every few steps and at the end,
check_status().  The cases and what their tapes must contain are in block_reps_cases.py; test_block_reps_host.py asserts that
without a GPU, and `PYTHONPATH=. python tests/block_reps_cases.py` prints the figures.

  A  the geometry of the block write, as steps and as one rollout() tape: corners, clipped borders, 1 x 1 / 1 x N / N x 1 / 2 x N maps,
     the 32 / 64-bit mask boundary, 16 and 64 lanes, maps beyond 64 columns and rows (k_big: byte maps, no planes, no incremental
     route), three words per row, column 254, warp at the border
  B  auto_reset=False: stepping on past done, `changes` far beyond max_changes
  C  asynchronous ticks: the B.pending preamble of k_update_block, with lockstep steps mixed in, two slots, past done, the other launch form
  D  actions outside the action space: clamped like the numpy clamp written here, reported by check_status()
  E  the developer switches that change how the lists k_update_block fills are consumed

What the oracle's tapes hold (committed seeds; floors in block_reps_cases.A_CASES, terms in its docstring):
    binary narrowmulti 3x3     corners 4, writes on non-corner border cells 204, jumps from < max_changes - 1 to > max_changes 25, episodes 93
    binary narrowmulti 1x1     writes 95                      binary narrowcast 2x5     corners 4, changes of six 24
    binary narrowcast 1x6/6x1  both ends, changes of three 35 zelda narrowmulti 33x4    corners 4, multi-cell writes at column 31 / 32: 123, nine-cell 49
    zelda narrowcast 32x16     corners 4, nine-cell 168, episodes 17;  16x17: corners 4, nine-cell 160, episodes 34
    zelda turtlecast 5x4       warp: corners 4, nine-cell 84, moves that wrap 501;  no warp: moves stopped at the border 517
    binary narrowcast 66x3     corners 4, multi-cell writes at column 63..65: 16, episodes 25
    binary narrowmulti 3x66    writes at row 63 / 64 / 65: at least 13 each
    zelda narrowmulti 130x3    corners 4, multi-cell writes at column 63..65 / 127 / 128: 63 (84 with columns 31 / 32, no word edge here), nine-cell 42
    binary turtlecast 65x65    multi-cell writes at column 63..65: 9, writes on the border 19, episodes 17
    binary narrowcast 255x2    writes with the cursor in column 254: 5
    steps by change 0..9 over A: 9027, 3309, 944, 1071, 1299, 1316, 1329, 359, 415, 611
    B: every environment of every case takes 10 or more steps past its first done; `changes` ends 155 .. 371 above max_changes
The asynchronous counters seen on the MI355X (suspended / late / pending_env_ticks; floors 3 / 1 / 3), also next to each case of C:
    sokoban narrowmulti 924 / 324 / 1 066       sokoban narrowcast 7x6  8 584 / 586 / 8 647     mdungeon turtlecast 60 / 3 / 64
    ddave narrowcast 343 / 11 / 343             with lockstep steps 2 349 / 640 / 2 354         two slots 174 / 8 / 320, overflow 781
    past done 331 / 22 / 331                    other launch form: sokoban 9 184 / 562 / 9 241, mdungeon 451 / 38 / 461

What guards what (seven mutations of k_update_block, by reading the kernel; 2, 5, 6 and 7 were never run -- they change a bound, the
tiles other kernels index with, who acts, or a store):
  1 `change++` also for a cell that already holds the value: `changes`, done and the routing (chg) differ in any step that rewrites a
    cell with its own tile -- every case; first binary narrowmulti 3x3 (two tiles: half the written cells hold the value already).
    Run once on a scratch build: all 46 tests of A, B and D fail;
  2 the clip `xx >= W` narrowed to `xx >= W - 1` (and `yy`): the last column / row is never written -- the corner and border
    conditions are there for it: narrowmulti 3x3, narrowcast 2x5, 1x6 / 6x1 (W - 1 = 0: nothing is ever written), 1x1 (no write at all);
  3 the heat increment at the cursor before the move: the heat map differs at once in every narrowcast / narrowmulti case (the cursor
    moves at every step); turtlecast cannot tell (a step moves or writes, never both), nor can the 1 x 1 map.  Run once on a scratch
    build: the 34 narrowcast / narrowmulti tests of A, B and D fail, the 10 turtlecast ones and the two of 1x1 pass;
  4 `warp` ignored: zelda turtlecast 5x4 warp (501 wrapping moves) and binary turtlecast 65x65.  Run once on a scratch build: those
    four tests fail, nothing else does;
  5 `vals[i] = a - 1` from the raw action, without the clamp or without its `bad`: D's narrowmulti entries NT + 1, 255 and 2^31 - 1
    (a tile that does not exist is written) and -1 (no difference on the map: -2 < 0 is skipped all the same -- that one is caught
    by the IndexError check_status() owes);
  6 in the B.pending preamble an environment with pv == 2 also takes its action: it steps (iterations, changes, map) before the
    reset that is due: the library's `consumed` then counts an action the harness never saw taken (consumed == steps fails), and
    a narrowcast / narrowmulti environment draws its cursor move from the ring before the reset draws the new map -- C, every case
    with auto-reset (`late` > 0 with change budgets so small that most completed steps end the episode);
  7 the plane words written without `touched`.  As the kernel stands m0 .. m2 are declared behind both `continue`s, so a skipped row
    never reaches the store and a row in which nothing changed gets back the words just read: no difference, no case can tell.  The
    variant that does harm has the masks hoisted out of the dy loop, loaded only for rows that are not skipped and stored always:
    a write of the centre alone (narrowcast type 1, turtlecast type 4, a narrowmulti action with zeros above and below) then puts
    the cursor row's words -- or zeros -- on rows y - 1 and y + 1 of the planes while the byte map stays right, and the statistics
    computed from the planes differ from the oracle's.  Only problems with planes can tell (not the maps beyond 64 columns): zelda
    narrowcast 32x16 / 16x17 and zelda turtlecast 5x4 in A (a third / a sixth of their steps are such writes), mdungeon narrowcast
    and sokoban turtlecast in B, sokoban narrowcast 7x6 and ddave narrowcast in C, through every info column and the reward.
"""
import numpy as np
import pytest

import block_reps_cases as bc
import oracle_lib as ol
import parity_harness as ph
from test_gpu_async import FEW_SOK

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------- A
@pytest.mark.parametrize("how", ["steps", "rollout"])
@pytest.mark.parametrize("name", list(bc.A_CASES))
def test_block_geometry_vs_oracle(name, how):
    """A: see block_reps_cases.A_CASES.  The tape holds what the case is there for (asserted on the oracle first), then every step --
    or the whole tape as one rollout() -- against the oracle."""
    bc.check_case_a(name)
    c = bc.A_CASES[name]
    err = ph.run_config(c["prob"], c["rep"], c["calls"], c["E"], c["T"], c["seed"], None, how == "rollout", tape=bc.tape("A", name))
    assert err is None, err


# ---------------------------------------------------------------------------------------------------------------- B
@pytest.mark.parametrize("how", ["steps", "rollout"])
@pytest.mark.parametrize("name", list(bc.B_CASES))
def test_block_reps_past_done_vs_oracle(name, how):
    """B: auto_reset=False against the oracle stepped without reset(); the map at every step.  Only a block write takes `changes`
    from below max_changes - 1 to above max_changes in one step -- and then goes on."""
    bc.check_case_b(name)
    c = bc.B_CASES[name]
    err = ph.run_config(c["prob"], c["rep"], c["calls"], c["E"], c["T"], c["seed"], None, how == "rollout", auto_reset=False, map_every=1,
                        tape=bc.tape("B", name))
    assert err is None, err


# ---------------------------------------------------------------------------------------------------------------- C
def _cut(cnt, lockstep=0):
    """Searches really were cut short, and the library's count of actions taken at ticks is the harness's (which also counts the
    `lockstep` actions taken by step() calls on the same handle: those do not go through the tick's preamble)."""
    assert cnt["suspended"] >= 3 and cnt["late"] >= 1 and cnt["pending_env_ticks"] >= 3, cnt
    assert cnt["consumed"] + lockstep == cnt["steps"], (cnt, lockstep)


# (problem, representation, adjust_param calls, E, ticks, pop budget, slots): the budgets of test_gpu_async.py's narrow cases.
# Seen on the MI355X, of about 25 000 actions taken:   suspended   late   pending_env_ticks
ASYNC_CASES = [
    ("sokoban", "narrowmulti", (), 256, 100, 24, 256),                                      # 924    324    1 066
    ("sokoban", "narrowcast", (dict(width=7, height=6), FEW_SOK), 256, 100, 16, 256),       # 8 584  586    8 647   (17 076 actions taken)
    ("mdungeon", "turtlecast", (), 256, 100, 24, 256),                                      # 60     3      64
    ("ddave", "narrowcast", (), 256, 100, 5, 256),                                          # 343    11     343
]


@pytest.mark.parametrize("prob,rep,calls,E,ticks,budget,nslots", ASYNC_CASES, ids=lambda v: str(v) if isinstance(v, (str, int)) else "cfg")
def test_block_reps_async_ticks_vs_oracle(prob, rep, calls, E, ticks, budget, nslots):
    """C: k_update_block's own copy of the B.pending preamble.  Per environment the actions it took and the steps it completed are
    the oracle's."""
    rs = np.random.RandomState(8900 + len(prob) + 7 * len(rep))
    _cut(ph.async_case(prob, rep, list(calls), E, ticks, 8900, rs, budget, nslots))


def test_block_reps_async_ticks_mixed_with_lockstep_steps():
    """C: every seventh tick is a flush() and a lockstep step() on the same handle: 13 of the 91 are step() calls of all 256
    environments.  (Seen: suspended 2 349, late 640, pending_env_ticks 2 354, consumed 18 246 + 3 328 = steps 21 574.)"""
    _cut(ph.async_case("sokoban", "narrowcast", [dict(width=7, height=6), FEW_SOK], 256, 91, 8910, np.random.RandomState(8910), 12, 128, flush_every=7),
         lockstep=13 * 256)


def test_block_reps_async_ticks_with_two_slots():
    """C: two slots: most suspensions find none and run to their end inside the tick.  (Seen: suspended 174, late 8,
    pending_env_ticks 320, overflow 781.)"""
    cnt = ph.async_case("sokoban", "narrowcast", [dict(width=7, height=6), FEW_SOK], 256, 90, 8920, np.random.RandomState(8920), 12, 2)
    _cut(cnt)
    assert cnt["overflow"] >= 3, cnt


def test_block_reps_async_ticks_past_done():
    """C: auto_reset=False under ticks, against the oracle without reset().  (Seen: suspended 331, late 22, pending_env_ticks 331.)"""
    cnt = ph.async_case("sokoban", "narrowcast", [dict(width=7, height=6), dict(change_percentage=0.3), FEW_SOK], 128, 100, 8930, np.random.RandomState(8930), 12, 128,
                        auto_reset=False)
    _cut(cnt)


@pytest.mark.parametrize("prob,rep,calls,budget,split", [("sokoban", "narrowcast", (dict(width=7, height=6), FEW_SOK), 16, 0), ("mdungeon", "narrowcast", (), 6, 1)])
def test_block_reps_async_other_launch_form(prob, rep, calls, budget, split):
    """C: async_split at the value that is not the problem's default (sokoban: 1, mdungeon: 0).  (Seen: sokoban suspended 9 184,
    late 562, pending_env_ticks 9 241; mdungeon 451, 38, 461.)"""
    _cut(ph.async_case(prob, rep, list(calls), 256, 100, 8940, np.random.RandomState(8940), budget, 128, tuning={"async_split": split}))


# ---------------------------------------------------------------------------------------------------------------- D
I32_MAX = 2 ** 31 - 1


def clamp_block_action(rep, a, nt):
    """What the library does to an action outside the space, restated: type to 0..2 (narrowcast) or 0..5 (turtlecast), value to
    0..NT-1, each of narrowmulti's nine entries to 0..NT."""
    if rep == "narrowmulti":
        return np.clip(a, 0, nt)
    return np.stack([np.clip(a[..., 0], 0, 2 if rep == "narrowcast" else 5), np.clip(a[..., 1], 0, nt - 1)], -1)


def _bad_tape(prob, rep, E, T, rs):
    """A legal tape [T, E, k] with one bad field in one environment at a time -> (tape, {step: [environments]}).  A bad value rides a
    block write (so that the clamped value lands on the map), a bad type keeps its legal value."""
    nt = len(ol.TILES[prob])
    acts = ph.draw_actions(ph.action_dims(prob, rep, 0, 0), rs, T, E)
    if rep == "narrowmulti":
        plan = [(0, -1), (4, nt + 1), (8, 255), (2, I32_MAX), (6, -1), (3, nt + 1)]
    else:
        block = 2 if rep == "narrowcast" else 5
        plan = [(0, -1), (0, block + 1), (0, I32_MAX), (1, -1), (1, nt), (1, 255)]
    bad = {}
    for j, (field, value) in enumerate(plan):
        t, e = 1 + 2 * (j % 3), (5, 17, 31, 32, 47, 63)[j]         # steps 1, 3, 5; the steps between them are legal
        if rep != "narrowmulti" and field == 1:
            acts[t, e, 0] = block
        acts[t, e, field] = value
        bad.setdefault(t, []).append(e)
    return acts, bad


@pytest.mark.parametrize("rep", ["narrowcast", "narrowmulti", "turtlecast"])
@pytest.mark.parametrize("prob", ["binary", "zelda"])
def test_out_of_range_block_actions_are_clamped_and_reported(prob, rep):
    """D: 64 environments, 7 steps; six of them get one bad field each (type -1 / one past the last / 2^31 - 1, value -1 / NT / 255, a
    narrowmulti entry -1 / NT + 1 / 255 / 2^31 - 1), everyone else legal actions.  check_status() is 0 until the first bad step and
    raises IndexError after it; at every step EVERY environment is the oracle stepped with clamp_block_action of its action -- for
    the 58 with legal actions that is their own action: nothing of a neighbour's bad one reaches them.  A fresh handle stepped
    through the legal tape alone reports 0."""
    from gym_pcgrl_amd.envs import BatchedPcgrlEnv
    E, T, seed0 = 64, 7, 8950
    nt = len(ol.TILES[prob])
    acts, bad = _bad_tape(prob, rep, E, T, np.random.RandomState(seed0))
    legal = clamp_block_action(rep, acts, nt).astype(np.int32)
    assert sorted(bad) == [1, 3, 5] and all((legal[t] != acts[t]).any(1).nonzero()[0].tolist() == sorted(bad[t]) for t in bad)
    assert all((legal[t] == acts[t]).all() for t in (0, 2, 4, 6))
    exp = ph._oracle_rollouts(prob, rep, [], [seed0 + i for i in range(E)], [legal[:, i] for i in range(E)])
    for tape, clean in ((acts, False), (legal, True)):
        env = BatchedPcgrlEnv(prob=prob, rep=rep, num_envs=E, seed=seed0)
        try:
            env.reset()
            keys = list(env._prob.info_keys) + ["iterations", "changes"]
            for t in range(T):
                obs, rew, done, info = env.step(tape[t])
                where = (prob, rep, "bad tape" if not clean else "legal tape", "step", t)
                assert np.array_equal(done.cpu().numpy(), np.array([x["done"][t] for x in exp])), ("done",) + where
                assert np.array_equal(rew.cpu().numpy(), np.array([x["reward"][t] for x in exp])), ("reward",) + where
                assert np.array_equal(np.stack([info[k].cpu().numpy() for k in keys], 1).astype(np.int64), np.stack([x["info"][t] for x in exp])), ("info",) + where
                assert ph._obs_mismatch(obs, exp, t, True, map_every=1) is None, (ph._obs_mismatch(obs, exp, t, True, map_every=1),) + where
                if clean or t < 1:
                    assert env.check_status() == 0, where
                elif t in bad:
                    with pytest.raises(IndexError):
                        env.check_status()
        finally:
            env.close()


# ---------------------------------------------------------------------------------------------------------------- E
SOK_OPEN = dict(probs={"empty": 0.75, "solid": 0.1, "player": 0.03, "crate": 0.06, "target": 0.06})
BINARY_14 = ("binary", "narrowcast", (dict(width=14, height=14), dict(change_percentage=0.2)), 64, 120)
ZELDA_11 = ("zelda", "narrowmulti", (dict(width=11, height=16), dict(change_percentage=0.3)), 64, 100)
TALL = ("binary", "turtlecast", (dict(width=20, height=30), dict(change_percentage=0.05)), 64, 120)
SOKOBAN = ("sokoban", "narrowmulti", (dict(change_percentage=0.6), SOK_OPEN), 64, 100)
BIG = ("binary", "narrowmulti", (dict(width=90, height=70), dict(change_percentage=0.005), dict(bc.BIG_OPEN)), 32, 60)    # B's case, with auto-reset
SWITCH_CASES = [(c, sw) for c in (BINARY_14, ZELDA_11) for sw in ({"inline_reset": 0}, {"no_inc": 1}, {"no_fused": 1})] + \
               [(TALL, sw) for sw in ({"no_wide": 1}, {"wide_pairs": 0}, {"wide_waves": 4})] + \
               [(SOKOBAN, sw) for sw in ({"sok_generic": 1}, {"sok_spawn": 1}, {"sok_spawn": 16})] + \
               [(BIG, {"big_team": 0})]


@pytest.mark.parametrize("how", ["steps", "rollout"])
@pytest.mark.parametrize("case,switches", SWITCH_CASES, ids=["%s-%s-%s" % (c[0], c[1], "-".join("%s=%d" % kv for kv in sw.items())) for c, sw in SWITCH_CASES])
def test_block_reps_under_the_step_switches_vs_oracle(case, switches, how):
    """E: the switches that change how WL_CHG / WL_RST are consumed -- resets through the reset list (inline_reset=0), no incremental
    route and no fused kernel (both no-ops for these representations: the launch layer must treat them so), tall maps on one wavefront
    per map / without pairs / on four wavefronts, Sokoban's general search and early publishing, big maps a wavefront each."""
    prob, rep, calls, E, T = case
    err = ph.run_config(prob, rep, list(calls), E, T, 8960, np.random.RandomState(8960), how == "rollout", tuning=dict(switches))
    assert err is None, err


SMB_POWER = 300
_SMB_TAPE = []


def _smb_tape(calls, E, T, seed0):
    """smb takes solver_power as an attribute of the problem, not through adjust_param (smb_prob.py:40-53): the oracle's side is made
    here with OracleEnv.set_solver_power before the reset, the batch gets the same through run_config(setup=)."""
    if not _SMB_TAPE:
        acts = ph.draw_actions(ph.action_dims("smb", "narrowcast", 114, 14), np.random.RandomState(seed0), T, E)
        exp = []
        for i in range(E):
            o = ol.OracleEnv("smb", "narrowcast")
            for kw in calls:
                o.adjust_param(**kw)
            o.set_solver_power(SMB_POWER)
            o.seed(seed0 + i)
            o.reset()
            exp.append(o.rollout(acts[:, i]))
        _SMB_TAPE.append((acts, exp))
    return _SMB_TAPE[0]


def _smb_power(env):
    env._prob._solver_power = SMB_POWER
    env.adjust_param()


@pytest.mark.parametrize("how", ["steps", "rollout"])
def test_smb_narrowcast_vs_oracle(how):
    """E: smb at its default size (114 x 14), solver_power 300, through k_update_block: these representations keep no play-through
    between steps (the launch layer's `rep <= PCGRL_REP_TURTLE` in front of the champion buffer), every change is a full play-through.
    The tape must hold steps that change the map and steps whose play-through gets somewhere (dist-win differs between steps)."""
    calls, E, T, seed0 = [dict(change_percentage=0.05)], 8, 12, 8970
    acts, exp = _smb_tape(calls, E, T, seed0)
    info = np.concatenate([x["info"] for x in exp])
    assert (np.diff(np.stack([x["info"][:, -1] for x in exp]), axis=1) > 0).sum() >= 20 and len(set(info[:, ol.INFO_KEYS["smb"].index("dist-win")].tolist())) >= 3
    err = ph.run_config("smb", "narrowcast", calls, E, T, seed0, None, how == "rollout", tape=(acts, exp), setup=_smb_power)
    assert err is None, err
