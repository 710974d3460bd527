"""Tile counts at 255 / 256 on every route that computes statistics, against the reference's fixtures (tests/golden/extremes_*.npz,
make_golden.py gen_extremes) and the CPU oracle.  Dave's row packs player, exit and key into one slot and col-diamonds into
another, MiniDungeons' its three collected counts: a row WITHIN LIMITS (every such count at most 255) must equal the reference bit
for bit and leave the status word at 0; BEYOND them check_status() must raise RuntimeError, the count is stored saturated at 255
and every column that owns a whole slot is still exact (extremes_fixtures.py).  One launch holds levels of both kinds.

Level sets: A 16 x 16 (16-row lane group, 32-bit masks), B 13 x 20 and 8 x 33 (the other lane group, 64-bit masks), C 4 x 65
(csrc/bigmap.h), D the 3 x 128 / 3 x 129 MiniDungeons serpentines that collect 255, 257, 256 and 255 treasures and the 3 x 130 Dave
serpentines that collect 257, 256 and 255 diamonds (bigmap.h and the planners of search_big.h).  zelda and sokoban share no slot: they are the control, exact with status 0 everywhere.

Which status write runs where:
  pcgrl_algos.h ddave_stats (through compute_item_stats)   the ddave cases of A and B in every test below
  bigmap.h big_item_stats, the ddave branch                 the ddave case of C in test_set_maps_stats_and_info, test_evaluate,
                                                            test_scripted_writes_across_the_limit, test_reset_with_all_weight_on_one_tile
  kernels_search_big.h, the mdungeon branch                 the 3 x 129 case of D in test_set_maps_stats_and_info and test_evaluate
  kernels_search_big.h, the ddave branch (col-diamonds)     the 3 x 130 case of D in the same two tests
The search problems' one-call evaluate kernels and asynchronous ticks exist only with the compact searches (at most 256 bordered
cells: no count can pass 255 there), so evaluate() scores the ddave / mdungeon / sokoban levels here through its scratch environment
and tick() steps them in lockstep; zelda's A and B are the one-call form (test_tile_extremes_host.py).
Handles hold three to eight environments; solver_power is 100, 1000 for D."""
import ctypes as C

import numpy as np
import pytest

import extremes_fixtures as xf
import oracle_lib as ol

pytestmark = pytest.mark.gpu
SEED = 8800
ABC = xf.cases(xf.SET_A + xf.SET_B, xf.ALL4) + xf.cases(xf.SET_C, xf.PACKED)
ABCD = ABC + xf.D_CASES


def _torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _calls(fx, **extra):
    kw = dict(change_percentage=1.0, **extra)
    if fx.prob != "zelda":
        kw["solver_power"] = fx.power
    return [dict(width=fx.w, height=fx.h), kw]


def _env(fx, n, calls=None):
    from gym_pcgrl_amd.envs import BatchedPcgrlEnv
    assert 3 <= n <= 8
    env = BatchedPcgrlEnv(prob=fx.prob, rep="wide", num_envs=n, seed=SEED)
    for kw in calls or _calls(fx):
        env.adjust_param(**kw)
    return env


def _oracle(fx, i, calls=None):
    o = ol.OracleEnv(fx.prob, "wide")
    for kw in calls or _calls(fx):
        o.adjust_param(**kw)
    o.seed(SEED + i)
    return o


def _clear(env):
    from gym_pcgrl_amd import _lib
    _lib.check(env._lib.pcgrl_clear_status(env._handle, env._stream()), "pcgrl_clear_status")


def _expect_status(env, beyond, what):
    """The sticky word of `env`: 0 when every level of the launches since the last look was within limits, else RuntimeError (bit 0
    alone); cleared for the next phase."""
    if beyond:
        with pytest.raises(RuntimeError):
            env.check_status()
        st = C.c_int32()
        env._lib.pcgrl_status(env._handle, env._stream(), C.byref(st))
        assert st.value in (0, 1), (what, st.value)        # (strict_actions handles clear it themselves)
        _clear(env)
    else:
        assert env.check_status() == 0, what


def _info_columns(prob, info):
    """The info columns of a step as [N, keys] in ol.INFO_KEYS order + iterations, changes."""
    keys = ol.INFO_KEYS[prob] + ["iterations", "changes"]
    return np.stack([info[k].cpu().numpy() for k in keys], 1).astype(np.int64)


def _info_mismatch(prob, got, want, ok, what):
    """Info rows of one step against the oracle's: all columns where `ok` (old and new row within limits, per environment), else the
    columns that own a slot (and the two counters)."""
    keys = ol.INFO_KEYS[prob] + ["iterations", "changes"]
    for i in range(len(want)):
        cols = list(range(len(keys))) if ok[i] else [j for j, k in enumerate(keys) if k in xf.OWN.get(prob, keys) or k in ("iterations", "changes")]
        if not np.array_equal(got[i, cols], want[i, cols]):
            return "%s environment %d (%s): info %s, the oracle %s (columns %s)" % (what, i, "within" if ok[i] else "beyond", got[i].tolist(), want[i].tolist(), [keys[j] for j in cols])
    return None


def _batches(fx, size=8):
    """The fixture's levels in order, `size` at a time (the last batch filled up from the front): the four counts of a once-only
    tile at both ends of the map are one batch -- levels of both kinds in one launch."""
    idx = list(range(len(fx.maps)))
    n = min(size, max(3, len(idx)))
    out = []
    for i in range(0, len(idx), n):
        out.append((idx[i:i + n] + idx * n)[:n])
    return out, n


# ------------------------------------------------------------------------------------------ set_maps() -> stats, info
@pytest.mark.parametrize("case", ABCD, ids=xf.case_id)
def test_set_maps_stats_and_info(case):
    """Every level through set_maps(): env.stats against the fixture, then a step that rewrites cell (0, 0) with its own tile: reward,
    done and info against OracleEnv (reset, set_map, the same step).  Then the levels within limits alone: status 0."""
    _torch()
    fx = xf.fixture(*case)
    batches, n = _batches(fx)
    ok_only = [i for i in range(len(fx.maps)) if fx.within[i]]
    batches += [(ok_only * n)[k:k + n] for k in range(0, len(ok_only), n)]
    env = _env(fx, n)
    oracles = [_oracle(fx, i) for i in range(n)]
    try:
        start = env.reset()["map"].cpu().numpy()
        for i, o in enumerate(oracles):
            assert np.array_equal(o.reset()["map"], start[i])
        assert env.check_status() == 0
        for b in batches:
            beyond = not fx.within[b].all()
            env.set_maps(fx.maps[b])
            got = env.stats.cpu().numpy()
            err = xf.mismatch(fx.prob, got, fx.stats[b], [fx.names[i] for i in b])
            assert err is None, err
            _expect_status(env, beyond, ("set_maps", [fx.names[i] for i in b]))
            acts = np.array([[0, 0, int(fx.maps[i][0, 0])] for i in b], np.int32)
            obs, rew, done, info = env.step(acts)
            want_r, want_d, want_i = [], [], []
            for k, i in enumerate(b):
                oracles[k].set_map(fx.maps[i])
                x = oracles[k].rollout(acts[k:k + 1])
                want_r.append(x["reward"][0]); want_d.append(x["done"][0]); want_i.append(x["info"][0])
                assert not x["done"][0], "the level ends the episode: the oracle's next map is a fresh one"
            assert np.array_equal(obs["map"].cpu().numpy(), fx.maps[b])
            ok = fx.within[b]
            assert np.array_equal(rew.cpu().numpy()[ok], np.array(want_r)[ok]) and np.array_equal(done.cpu().numpy()[ok], np.array(want_d)[ok])
            err = _info_mismatch(fx.prob, _info_columns(fx.prob, info), np.array(want_i), ok, "step after set_maps")
            assert err is None, err
            _clear(env)          # (a step that changes nothing may or may not compute the statistics again)
    finally:
        env.close()


# ------------------------------------------------------------------------------------------ evaluate()
def _pairs(fx):
    """(a, b) level indices that differ in one cell: n and n + 1 of a once-only tile, at either end of the map."""
    out = []
    for tile in xf.ONCE_ONLY[fx.prob]:
        for where in ("first", "last"):
            for n in (254, 255, 256):
                a, b = "%s-%s-%d" % (where, tile, n), "%s-%s-%d" % (where, tile, n + 1)
                if a in fx.names and b in fx.names:
                    out.append((fx.index(a), fx.index(b)))
    return out


@pytest.mark.parametrize("case", ABCD, ids=xf.case_id)
def test_evaluate(case):
    """evaluate() of the whole fixture in one call (a handle of three environments; the scratch environment of the fallback route
    takes eight maps at a time), then of the levels within limits alone; with `ref` rows, reward and over of every pair of levels one
    write apart against the oracle's step, where both rows are within limits."""
    torch = _torch()
    fx = xf.fixture(*case)
    env = _env(fx, 3)
    try:
        cfg = env._config()
        fast = int(env._lib.pcgrl_get_stats_bytes(C.byref(cfg), len(fx.maps))) > 0
        assert fast == (fx.prob == "zelda")
        word = lambda: env if fast else env._eval_scratch      # the handle whose status word the route reports to
        maps = fx.maps if len(fx.maps) >= 3 else np.concatenate([fx.maps] * 3)[:3]
        want = fx.stats if len(fx.maps) >= 3 else np.concatenate([fx.stats] * 3)[:3]
        ev = env.evaluate(maps, chunk=8)
        err = xf.mismatch(fx.prob, ev.stats.cpu().numpy(), want, fx.names if len(fx.maps) >= 3 else None)
        assert err is None, err
        _expect_status(word(), not xf.within(fx.prob, want).all(), "evaluate, every level")
        ok = np.nonzero(xf.within(fx.prob, want))[0]
        ok = ok if len(ok) >= 3 else np.concatenate([ok] * 3)[:3]
        got = env.evaluate(maps[ok], chunk=8).stats.cpu().numpy().astype(np.int64)
        assert np.array_equal(got, want[ok])
        _expect_status(word(), False, "evaluate, the levels within limits")
        pairs = _pairs(fx)
        if not pairs:
            assert case in xf.D_CASES
            return
        a0, reward, done = [], [], []
        for k, (a, b) in enumerate(pairs):
            d = np.argwhere(fx.maps[a] != fx.maps[b])
            assert len(d) == 1
            y, x = int(d[0, 0]), int(d[0, 1])
            o = _oracle(fx, k)
            a0.append(o.reset()["map"].copy())
            o.set_map(fx.maps[a])
            obs, r, _, _ = o.step([x, y, int(fx.maps[b][y, x])])
            assert np.array_equal(obs["map"], fx.maps[b])
            obs, _, dn, info = o.step([x, y, int(fx.maps[b][y, x])])        # rewrites the cell: `done` is the problem's criterion alone
            assert info["changes"] < info["max_changes"] and info["iterations"] < info["max_iterations"]
            reward.append(r); done.append(dn)
        ia, ib = [p[0] for p in pairs], [p[1] for p in pairs]
        both = fx.within[ia] & fx.within[ib]
        assert both.any()
        rows_a, rows_0 = env.evaluate(fx.maps[ia], chunk=8).rows.clone(), env.evaluate(np.stack(a0), chunk=8).rows.clone()
        got_r = env.evaluate(fx.maps[ib], ref=rows_a, chunk=8).reward.cpu().numpy()
        got_o = env.evaluate(fx.maps[ib], ref=rows_0, chunk=8).over.cpu().numpy()
        assert got_r.dtype == np.float64
        assert np.array_equal(got_r[both], np.array(reward)[both]), (got_r, reward, both)
        assert np.array_equal(got_o[both], np.array(done)[both]), (got_o, done, both)
        _clear(word())
    finally:
        env.close()


# ------------------------------------------------------------------------------------------ steps across the limit
def _tapes(fx):
    """One environment per once-only tile, from 254 of it on the first cells through the scripted writes (threshold_tape), and
    control environments that go through the same writes of `player` on an empty map (counts 1, 2, 3, 2, 1, 0 -- cells 254 ..
    256 are what is written, so the first write makes one player).  -> start maps [N, H, W], actions [6, N, 3], counts [6, N]."""
    start, acts, counts = [], [], []
    for tile in xf.ONCE_ONLY[fx.prob]:
        a, c = xf.threshold_tape(fx, tile)
        start.append(fx.maps[fx.index("first-%s-254" % tile)]); acts.append(a); counts.append(c)
    while len(start) < 3 or len(start) == len(xf.ONCE_ONLY[fx.prob]):
        a, c = xf.threshold_tape(fx, "player")
        start.append(np.zeros((fx.h, fx.w), np.uint8)); acts.append(a); counts.append([v - 254 for v in c])
    return np.stack(start), np.stack(acts, 1), np.array(counts).T


def _tape_expectations(fx):
    start, acts, counts = _tapes(fx)
    n = start.shape[0]
    exp = []
    for i in range(n):
        o = _oracle(fx, i)
        o.reset()
        o.set_map(start[i])
        exp.append(o.rollout(acts[:, i]))
        assert not exp[-1]["done"].any(), "an episode ends on the tape: the next map would be a fresh one"
    e_rew, e_done, e_info = (np.stack([x[k] for x in exp], 1) for k in ("reward", "done", "info"))
    shared = fx.prob in xf.PACKED and fx.prob == "ddave"          # (MiniDungeons' player and exit own their slots)
    new_ok = (counts <= 255) | (not shared)
    old_ok = np.concatenate([np.ones((1, n), bool), new_ok[:-1]])
    assert (old_ok & new_ok)[[0, 5]].all()                        # the first step and the last: both rows within limits
    if shared:
        assert not (old_ok & new_ok)[1:5, :len(xf.ONCE_ONLY[fx.prob])].any() and new_ok[:, len(xf.ONCE_ONLY[fx.prob]):].all()
    return start, acts, e_rew, e_done, e_info, old_ok, new_ok


def _check_step(fx, t, rew, done, info, e_rew, e_done, e_info, old_ok, new_ok, route):
    ok = old_ok[t] & new_ok[t]
    what = "%s %s %dx%d step %d" % (route, fx.prob, fx.h, fx.w, t)
    assert np.array_equal(np.asarray(rew)[ok], e_rew[t][ok]), (what, "reward", np.asarray(rew).tolist(), e_rew[t].tolist(), ok.tolist())
    assert np.array_equal(np.asarray(done)[ok] != 0, e_done[t][ok]), (what, "done")
    err = _info_mismatch(fx.prob, info, e_info[t], new_ok[t], what)      # (the info row is the new row: exact where IT is within limits)
    assert err is None, err


# (tick() is step() itself for the problems without a planner: Dave and MiniDungeons only)
ROUTES = [pytest.param(c, r, id="%s-%s" % (xf.case_id(c), r)) for c in ABC for r in ("step", "rollout", "tick") if r != "tick" or c[0] in xf.PACKED]


@pytest.mark.parametrize("case,route", ROUTES)
def test_scripted_writes_across_the_limit(case, route):
    """Wide representation, change_percentage 1.0: from 254 of a once-only tile six writes take the count across the limit and back.
    Reward, done and every info column at the steps whose old and new rows are both within limits (the first and the last; for the
    control environments and the problems that share no slot: every step), the columns that own a slot at every step; the status
    word is 0 after the first step, raised after the second and after every later step whose new row is beyond the limits.  The same
    tape as one rollout(), and for Dave and MiniDungeons as ticks with pop_budget 4."""
    torch = _torch()
    fx = xf.fixture(*case)
    start, acts, e_rew, e_done, e_info, old_ok, new_ok = _tape_expectations(fx)
    n = start.shape[0]
    env = _env(fx, n)
    try:
        env.reset()
        if route == "tick":
            # more than 256 bordered cells: the general searches, which have no asynchronous form -- a tick is a lockstep step and
            # nothing is ever pending.  (Should these shapes get one, the loop below needs a cursor per environment.)
            assert not env.enable_async(nslots=8)
        env.set_maps(start)
        assert env.check_status() == 0
        if route == "rollout":
            rew, done, info = env.rollout(torch.as_tensor(acts, device=env.device))
            keys = ol.INFO_KEYS[fx.prob] + ["iterations", "changes"]
            got_info = np.stack([info[k].view(6, n).cpu().numpy() for k in keys], 2).astype(np.int64)
            for t in range(6):
                _check_step(fx, t, rew[t].cpu().numpy(), done[t].cpu().numpy(), got_info[t], e_rew, e_done, e_info, old_ok, new_ok, route)
            _expect_status(env, not new_ok.all(), "rollout")
        else:
            for t in range(6):
                if route == "step":
                    obs, rew, done, info = env.step(acts[t])
                else:
                    obs, rew, done, info, pend = env.tick(acts[t], pop_budget=4)
                    assert not pend.any()
                _check_step(fx, t, rew.cpu().numpy(), done.cpu().numpy(), _info_columns(fx.prob, info), e_rew, e_done, e_info, old_ok, new_ok, route)
                _expect_status(env, not new_ok[t].all(), (route, t))
        final = start.copy()
        assert np.array_equal(env._bufs["map"].cpu().numpy(), final), "the tape ends on the maps it started from"
    finally:
        env.close()


# ------------------------------------------------------------------------------------------ reset() with all weight on one tile
@pytest.mark.parametrize("case", ABC, ids=xf.case_id)
def test_reset_with_all_weight_on_one_tile(case):
    """probs that put all weight on one once-only tile: the start map is the oracle's (that tile everywhere) and the start
    statistics are the fixture's all-<tile> row -- exact with status 0, or (Dave) reported and saturated."""
    _torch()
    fx = xf.fixture(*case)
    for tile in xf.ONCE_ONLY[fx.prob]:
        probs = {t: (1.0 if t == tile else 0.0) for t in ol.TILES[fx.prob]}
        calls = _calls(fx) + [dict(probs=probs)]
        env = _env(fx, 3, calls)
        try:
            got_map = env.reset()["map"].cpu().numpy()
            i = fx.index("all-" + tile)
            for k in range(3):
                assert np.array_equal(_oracle(fx, k, calls).reset()["map"], got_map[k]) and np.array_equal(got_map[k], fx.maps[i])
            err = xf.mismatch(fx.prob, env.stats.cpu().numpy(), fx.stats[[i] * 3], ["all-" + tile] * 3)
            assert err is None, err
            _expect_status(env, not fx.within[i], ("reset", tile))
        finally:
            env.close()
