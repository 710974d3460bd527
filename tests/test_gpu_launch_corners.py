"""The corners of the host launch layer's dispatch (csrc/pcgrl_abi.hip: with_prob, with_lanes, with_mask, with_rep) that the other
suites leave out: the search problems and smb on 64-row lane groups and on 64-bit row masks.  The smallest shapes that select each
(GROUP, MaskT) instantiation -- 17 rows for a lane group of 64, 40 columns for a 64-bit mask -- all within the compact searches (at most
256 bordered cells).  Every step, every statistics row, bit for bit against the CPU oracle.

Each stepping case ends at least one episode inside its tape IN THE ORACLE (asserted from the oracle's `done`; the change percentages
were chosen on the CPU for that), so that the reset launches run: k_reset<PROB, GROUP, MaskT>, k_smb's in-kernel reset."""
import numpy as np
import pytest

import oracle_lib as ol
import parity_harness as ph

pytestmark = pytest.mark.gpu

E, T, SEED0 = 24, 48, 4100
# about one player per map: a good share of the levels are ones a planner runs on
SPARSE = {"sokoban": {"empty": 0.9, "solid": 0.08, "player": 0.006, "crate": 0.007, "target": 0.007},
          "mdungeon": {"empty": 0.86, "solid": 0.06, "player": 0.006, "exit": 0.006, "potion": 0.02, "treasure": 0.02, "goblin": 0.02, "ogre": 0.012},
          "ddave": {"empty": 0.75, "solid": 0.2, "player": 0.006, "exit": 0.006, "diamond": 0.012, "key": 0.006, "spike": 0.02},
          # (mostly blocked levels: episodes do not end at once, smb_prob.py:191-192)
          "smb": {"empty": 0.5, "solid": 0.4, "tube": 0.05}}
POWER = 120

# id -> (prob, rep, width, height, change_percentage)
STEP_CASES = {
    # lane group of 64, 32-bit masks
    "sokoban-narrow-10x17": ("sokoban", "narrow", 10, 17, 0.04),
    "mdungeon-turtle-10x17": ("mdungeon", "turtle", 10, 17, 0.04),
    "ddave-wide-10x17": ("ddave", "wide", 10, 17, 0.04),
    # lane group of 16, 64-bit masks
    "sokoban-wide-40x4": ("sokoban", "wide", 40, 4, 0.04),
    "mdungeon-narrow-40x4": ("mdungeon", "narrow", 40, 4, 0.04),
    "ddave-narrow-40x4": ("ddave", "narrow", 40, 4, 0.04),
    # lane group of 64, 64-bit masks
    "zelda-narrow-40x20": ("zelda", "narrow", 40, 20, 0.02),
    # smb: k_reset<smb, 64, 32-bit / 64-bit>
    "smb-narrow-20x17": ("smb", "narrow", 20, 17, 0.03),
    "smb-wide-40x20": ("smb", "wide", 40, 20, 0.02),
}
_TAPES = {}


def _torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _calls(name):
    prob, rep, w, h, change = STEP_CASES[name]
    kw = dict(change_percentage=change)
    if prob in SPARSE:
        kw.update(probs=SPARSE[prob])
    if prob in ("sokoban", "mdungeon", "ddave"):
        kw.update(solver_power=POWER)
    return [dict(width=w, height=h), kw]


def _tape(name, auto_reset=True):
    """(acts, exp) of one case: the oracle's side, made once and shared by the tests that step it; an episode ends inside it."""
    key = (name, auto_reset)
    if key not in _TAPES:
        prob, rep, w, h, _ = STEP_CASES[name]
        rs = np.random.RandomState(sum(map(ord, name)))
        if auto_reset:
            acts, exp = ph.oracle_tape(prob, rep, _calls(name), E, T, SEED0, rs)
        else:
            acts = ph.draw_actions(ph.action_dims(prob, rep, w, h), rs, T, E)
            exp = ph._oracle_rollouts(prob, rep, _calls(name), [SEED0 + i for i in range(E)], [acts[:, i] for i in range(E)], auto_reset=False)
        assert any(x["done"][:-1].any() for x in exp), "no episode ends inside the tape: the reset launches would not run"
        _TAPES[key] = (acts, exp)
    return _TAPES[key]


def _run(name, use_rollout=False, auto_reset=True, tuning=None):
    _torch()
    prob, rep, _, _, _ = STEP_CASES[name]
    err = ph.run_config(prob, rep, _calls(name), E, T, SEED0, None, use_rollout, auto_reset=auto_reset, tuning=tuning, tape=_tape(name, auto_reset))
    assert err is None, err


@pytest.mark.parametrize("name", list(STEP_CASES))
def test_steps(name):
    _run(name)


@pytest.mark.parametrize("name", [n for n in STEP_CASES if n.endswith("40x4")])
def test_rollout_64bit_masks(name):
    """pcgrl_rollout on a lane group of 16: k_step_solver<PROB, REP, 64-bit masks>."""
    _run(name, use_rollout=True)


def test_search_without_auto_reset():
    """The `clr` arguments of a step whose last launch is the first search launch."""
    _run("mdungeon-turtle-10x17", auto_reset=False)


def test_zelda_separate_reset_pass():
    """inline_reset = 0: k_stats<zelda, 64, 64-bit> without the in-kernel reset, then k_reset<zelda, 64, 64-bit>."""
    _run("zelda-narrow-40x20", tuning={"inline_reset": 0})


# ------------------------------------------------------------------ evaluate() and solve(): k_get_stats<PROB, GROUP, MaskT>, the searches behind it
EVAL_POWER = 300
_MAPS = {}


def _reset_maps(prob, w, h):
    """Sixteen maps of the oracle's own resets and their statistics rows: of the resets of 1 500 seeds the first eight levels a planner
    ran on (solved ones first) and the first eight others."""
    if (prob, w, h) not in _MAPS:
        ran, rest = [], []
        for i in range(1500):
            o = ol.OracleEnv(prob, "wide")
            o.adjust_param(width=w, height=h, probs=SPARSE[prob])
            o.seed(SEED0 + 100 + i)
            m = o.reset()["map"].copy()
            st, iters = ol.get_stats(prob, m, solver_power=EVAL_POWER, with_iters=True)
            if iters.max() > 0:
                ran.append((m, st))
            elif len(rest) < 8:
                rest.append((m, st))
        ran.sort(key=lambda x: x[1][-1] <= 0)                      # (stable: solved levels -- sol-length > 0 -- first)
        pick = ran[:8] + rest
        assert len(pick) == 16
        _MAPS[prob, w, h] = (np.stack([m for m, _ in pick]), np.stack([st for _, st in pick]))
    return _MAPS[prob, w, h]


def _make(prob, w, h):
    from gym_pcgrl_amd.envs import BatchedPcgrlEnv
    env = BatchedPcgrlEnv(prob=prob, rep="wide", num_envs=3, seed=1000)
    env.adjust_param(width=w, height=h, solver_power=EVAL_POWER)
    return env


@pytest.mark.parametrize("w,h", [(10, 17), (40, 4)])
@pytest.mark.parametrize("prob", ["sokoban", "mdungeon", "ddave"])
def test_evaluate(prob, w, h):
    _torch()
    maps, want = _reset_maps(prob, w, h)                          # (eight of them parked for k_get_stats_search)
    env = _make(prob, w, h)
    got = env.evaluate(maps).stats.cpu().numpy().astype(np.int64)
    assert env.check_status() == 0
    assert np.array_equal(got, want), np.nonzero((got != want).any(1))[0][:5]
    env.close()


@pytest.mark.parametrize("w,h", [(10, 17), (40, 4)])
def test_solve_sokoban(w, h):
    torch = _torch()
    from gym_pcgrl_amd import replay_sokoban
    maps, want = _reset_maps("sokoban", w, h)
    assert (want[:, 5] > 0).sum() >= 4                           # solved levels: there are moves to check
    env = _make("sokoban", w, h)
    sol = env.solve(maps)
    assert env.check_status() == 0
    assert np.array_equal(sol.stats.cpu().numpy().astype(np.int64), want)
    assert torch.equal(sol.rows, env.evaluate(maps).rows)
    moves, length = sol.moves.cpu().numpy(), sol.length.cpu().numpy()
    assert np.array_equal(length, want[:, 5])                    # sol-length
    for i in np.nonzero(length > 0)[0]:                          # the moves, by the game's rules: a win in exactly `length` moves
        r = replay_sokoban(maps[i], moves[i])
        assert int((moves[i] >= 0).sum()) == length[i] and r.legal and r.won, i
    env.close()
