"""A numpy model of one environment's representation stream, the event classes of the device's MT19937 draw paths, and the case
table of tests/test_stream_census_host.py (no GPU) and tests/test_gpu_stream_edges.py.  Test infrastructure.

The device draws numpy's randint(W), randint(H) (masked rejection, one 32-bit word a try) in three places, each with a fast path
of a fixed number of words and a fallback: the draw cache of the fused step (update_env_cursor, 8 words), the speculative draws of
k_update (PCGRL_SPEC_DRAWS = 6) and the whole-wavefront wave_draw_xy of the resets (8 words; lane 0 goes on alone).  Which path a
draw takes, where the ring cursor stands when a reset stages its part of the ring, whether the episode end was certain when the
step's update ran: all of that follows from the seed and the tape of actions, so it can be counted here, with numpy and the oracle
alone, before a GPU runs anything.  StreamModel is np.random.RandomState driven the way Representation.reset / NarrowRepresentation
.update drive it; trace_steps() keeps it in step with OracleEnv rollouts and asserts ring cursor and cursor position at every step.

Event classes (census()):
  S8-x, S8-y      a step draw the draw cache cannot finish: x not found in the 8 cached words / x found, y not (cache fallback)
  S8-x@8          x accepted exactly on word 8 (the fallback goes on with y alone)
  S6              a step draw that needs more than 6 words (k_update's fallback)
  TAG             a cache draw with fifo_tag != cursor: the step after an S8, after seed(), after load_state_dict()
  R8, R8-x        a reset's own cursor draw that needs more than 8 words (wave_draw_xy's lane-0 fallback) / x not among the 8
  R8-x@8          ... x accepted on word 8 (the ix >= 7 branch)
  R=8             a reset's cursor draw that takes exactly 8 words: lane 7's word is used, whose second operand is the last word a
                  partial staging has to hold without a draw cache (offset need; with a cache the rebuild reads on to need - 1)
                  suffix /p: the reset staged two stretches of the ring (RESTAGE re-stages the rest first); /f: the whole ring;
                  /b: block_reset_env, where thread 0 draws; /u: k_stats_wide, an episode end nobody foresaw (block_reset_env or
                  one wavefront's wave_reset_env, the model cannot tell)
  RS8             a certain reset of the fused step whose *step* draws (step_draws) need more than 8 words
  RS+R8           a certain reset whose step draws are fine and whose own draws need more than 8
  PEND            an episode end nobody foresaw in a step whose draw took k >= 1 cache words (patched into the staged ring)
  PEND-after-S8   ... in the same step as an S8 (the fallback wrote the ring; the reset stages it in the same launch)
  WRAP-a          the reset's stretch [cur, cur + need) of the ring crosses slot 623 -> 0
  WRAP-m          the stretch 397 words on crosses it (partial staging only: that stretch is staged on its own)
  WRAP-8          the eight candidate words of a cursor draw of a reset straddle it
  WRAP-8s         ... of a step draw (cache draw, speculative draw) / of the cache refill behind it (fifo_refill, cur0 + 8)
  AXIS            a draw on a map with W = 1 or H = 1: randint(1) draws nothing (rx == 0, ry == 0, ix = -1)
"""
import ctypes
import functools
import json
import os
from collections import namedtuple

import numpy as np

import oracle_lib as ol
import parity_harness as ph

MT_N, MT_M, FIFO_N, SPEC_DRAWS = 624, 397, 8, 6
FLOOR_COUNT, FLOOR_ENVS = 3, 2          # every class that applies: at least 3 times, in at least 2 environments
MAX_ENVS, MAX_STEPS = 512, 60
SEEDS_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "stream_seeds.json")
POOL_SEED0 = 900000


class StreamModel:
    """The representation stream of one environment: np.random.RandomState seeded as OracleEnv.seed seeds it, drawn from as
    Representation.reset (random_sample((H, W)): two words a cell -- what RandomState.choice(p=) draws --, then randint(W), randint(H)
    unless the representation is wide) and NarrowRepresentation.update (randint(W), randint(H)) draw.  `words` counts what was
    consumed; the ring cursor is words mod 624."""

    def __init__(self, seed, w, h, rep):
        self.w, self.h, self.rep = int(w), int(h), rep
        self.seed(seed)

    def seed(self, seed):
        self.seed_key(ol.seed_key(seed))

    def seed_key(self, key):
        self.key = key
        self.rs = np.random.RandomState(self.key)
        self.words = 0
        # get_state()[2], read where numpy keeps it instead of through a copy of the whole state, which costs 50 us a look -- three
        # looks a draw, two minutes over the case table.  This relies on a layout numpy does not promise: the bit generator's
        # ctypes.state_address pointing at mt19937_state { uint32_t key[624]; int pos; }.  It is taken only if it shows 624 right after
        # seeding as get_state() does; draw_xy() and reset() assert what it shows against the words counted, trace_steps() asserts
        # get_state()[2] itself at the end of every tape, and without it _pos() goes through get_state().
        self._pos_field = None
        try:
            self._pos_field = ctypes.c_int.from_address(self.rs._bit_generator.ctypes.state_address + 4 * MT_N)
            if self._pos_field.value != self.rs.get_state()[2]:
                self._pos_field = None
        except Exception:
            self._pos_field = None

    @property
    def cursor(self):
        return self.words % MT_N

    def _pos(self):
        pos = self._pos_field.value if self._pos_field is not None else int(self.rs.get_state()[2])
        return pos % MT_N          # (numpy: 624 = "make the next block first")

    def draw_xy(self):
        """randint(W), randint(H) -> (cursor before, words for x, words for y, x, y)"""
        c0 = self._pos()
        assert c0 == self.cursor
        x = int(self.rs.randint(self.w))
        c1 = self._pos()
        y = int(self.rs.randint(self.h))
        c2 = self._pos()
        kx, ky = (c1 - c0) % MT_N, (c2 - c1) % MT_N
        self.words += kx + ky
        return c0, kx, ky, x, y

    def clone(self):
        m = StreamModel.__new__(StreamModel)
        m.w, m.h, m.rep, m.key = self.w, self.h, self.rep, self.key
        m.seed_state(self.rs.get_state(), self.words)
        return m

    def seed_state(self, state, words):
        self.seed_key(self.key)
        self.rs.set_state(state)
        self.words = words

    def reset(self, gen_map=True):
        """-> (cursor before, words of the map, draw_xy() of the new cursor position or None)"""
        c0 = self.cursor
        nmap = 0
        if gen_map:
            self.rs.random_sample((self.h, self.w))
            nmap = 2 * self.w * self.h
            self.words += nmap
            assert self._pos() == self.cursor
        return c0, nmap, (self.draw_xy() if self.rep != "wide" else None)

    def step(self):
        """The cursor move of a narrow step (random_tile) -> draw_xy(), or None for the representations that draw nothing."""
        return self.draw_xy() if self.rep == "narrow" else None

    def ring_image(self):
        """The lazy ring the device keeps (csrc/mt19937.h): slot i below the cursor holds word i of the block of 624 being consumed,
        the slots from the cursor on still hold the previous block (block 0: the seeded state)."""
        def block(k):
            rs = np.random.RandomState(self.key)
            if k > 0:
                rs.random_sample(312 * (k - 1) + 1)          # two words each: the state array is block k from its first word on
            return np.asarray(rs.get_state()[1], dtype=np.uint32)
        b, c = divmod(self.words, MT_N)
        if c == 0:
            return block(b)
        return np.where(np.arange(MT_N) < c, block(b + 1), block(b)).astype(np.uint32)


# ------------------------------------------------------------------ the case table
# route: which kernels a shape takes, read off the launchers (csrc/pcgrl_abi.hip):
#   fused    fused_step_applies: binary / zelda, H <= 16, W <= 64, narrow / turtle / wide, auto-reset -> k_step.  Step draws: the draw
#            cache (update_env_cursor); resets: wave_reset_env<PARTIAL = false> with step_draws / pend.  With no_fused = 1 the same shapes
#            take k_update (speculative draws) + k_stats, whose resets are wave_reset_env<PARTIAL = true>: route "two".
#   block    binary, H > 16, at most 64 x 64: k_update + k_stats_wide.  Certain resets and those behind a full recomputation: block_reset_env
#            (thread 0 draws the cursor); an episode end nobody foresaw on an incremental item: wave_incremental_item ->
#            wave_reset_env<PARTIAL = true> from one wavefront.
#   big      W > 64 or H > 64: k_update + k_big, resets by wave_reset_env<PARTIAL = true> (no staging area for the tiles).
#   solver   sokoban / mdungeon / ddave on at most 256 bordered cells: k_step_solver (update_env without the cache, resets by
#            wave_reset_env<PARTIAL = true>); tick() runs k_update + the asynchronous searches + k_reset.
#   smb      k_update + k_smb (wave_reset_env<PARTIAL = true>).
# reset() itself is k_reset (k_big for the big maps) for every shape: wave_reset_env<PARTIAL = true>.
Case = namedtuple("Case", "name prob rep w h calls E T route note pre")

_GOAL_ZELDA = dict(target_enemy_dist=1, probs={"empty": 0.8, "solid": 0.1, "player": 0.02, "key": 0.02, "door": 0.02,
                                                "bat": 0.01, "scorpion": 0.01, "spider": 0.01})
_OPEN = {"sokoban": dict(probs={"empty": 0.8, "solid": 0.08, "player": 0.04, "crate": 0.04, "target": 0.04}),
         "mdungeon": dict(probs={"empty": 0.75, "solid": 0.05, "player": 0.05, "exit": 0.05, "goblin": 0.03, "ogre": 0.03}),
         "ddave": dict(probs={"empty": 0.7, "solid": 0.1, "player": 0.05, "exit": 0.05, "key": 0.05, "spike": 0.02})}


def _case(prob, rep, w, h, note, changes=2, E=MAX_ENVS, T=MAX_STEPS, extra=(), pre=0):
    """max_changes = `changes` (change_percentage just above changes / cells): certain resets every few steps; a goal random maps
    often meet (binary: a path one longer; zelda: the sparse tile mix of the fuzz harness's goal mode), so that episodes also end
    where the update could not know.  pre: reset() calls in front of the tape beyond the first -- a tape starts at ring cursor 0
    plus one reset, and where steps and resets take few words, or always the same number, it would never carry the cursor over the
    slots a wrap class needs."""
    cells = w * h
    pct = min(1.0, (changes + 0.5) / cells)
    assert max(int(pct * cells), 1) == (changes if cells > 1 else 1)
    calls = [dict(width=w, height=h), dict(change_percentage=pct)]
    if prob == "binary":
        calls.append(dict(target_path=1))
    elif prob == "zelda":
        calls.append(dict(target_path=1, **_GOAL_ZELDA))
    elif prob in _OPEN:
        calls.append(dict(solver_power=60, **_OPEN[prob]))
    calls.extend(extra)
    if w > 64 or h > 64:
        route = "big"
    elif prob == "smb":
        route = "smb"
    elif prob in _OPEN:
        route = "solver"
    elif h <= 16:
        route = "fused"
    else:
        route = "block" if prob == "binary" else "two"
    return Case("%s-%s-%dx%d" % (prob, rep, w, h), prob, rep, w, h, tuple(calls), E, T, route, note, pre)


CASES = [
    # high rejection: sizes just above a power of two
    _case("binary", "narrow", 9, 9, "7/16 of the words rejected on both axes"),
    _case("binary", "narrow", 5, 5, "3/8 rejected"),
    _case("binary", "narrow", 17, 3, "15/32 rejected for x, 1/4 for y"),
    _case("binary", "narrow", 33, 2, "64-bit rows; 31/64 rejected for x, y never: x alone can use up the eight words"),
    _case("zelda", "narrow", 9, 9, "three planes"),
    _case("zelda", "narrow", 5, 5, "three planes"),
    _case("zelda", "narrow", 17, 3, "wide, flat and still staged in part"),
    _case("zelda", "narrow", 33, 2, "64-bit rows, three planes", E=256),
    _case("binary", "narrow", 3, 17, "17 rows: block_reset_env on 102 words", E=256),
    # an axis of one cell: randint(1) draws nothing
    _case("binary", "narrow", 9, 1, "H = 1: ry == 0", E=256, pre=10),
    _case("binary", "narrow", 1, 9, "W = 1: rx == 0, ix = -1", E=256, pre=10),
    _case("binary", "narrow", 1, 1, "neither axis draws: a reset's cursor draw uses no word", changes=1, E=128, T=30),
    _case("zelda", "turtle", 1, 9, "W = 1 on the reset's draw alone (turtle steps draw nothing)", changes=1, E=256),
    # partial-staging threshold: pend + need + 2 <= 226, need = 2 * cells + 8 (+ 9 with a draw cache to rebuild)
    _case("zelda", "turtle", 12, 9, "108 cells: the last shape staged in part without a draw cache (226 words)", E=256),
    _case("zelda", "turtle", 11, 10, "110 cells: the whole ring", E=256),
    _case("binary", "turtle", 12, 9, "one plane", E=256, pre=12),
    _case("binary", "narrow", 17, 6, "102 cells: the last staged in part with a cache (223 words)", E=256),
    _case("binary", "narrow", 13, 8, "104 cells: the whole ring", E=256, pre=30),
    _case("zelda", "narrow", 17, 6, "three planes", E=256),
    # the 113-cell rounds (nA / nB)
    _case("binary", "narrow", 8, 8, "64 cells: nA = 64, nB = 0; no word is ever rejected", E=256),
    _case("binary", "narrow", 13, 5, "65 cells: nB = 1", E=256),
    _case("zelda", "narrow", 16, 7, "112 cells: nB = 48", E=256),
    _case("binary", "narrow", 19, 6, "114 cells: a second round of one cell", E=256),
    _case("zelda", "wide", 9, 9, "the reset without a cursor draw", E=256),
    # k_big
    _case("binary", "narrow", 113, 1, "113 cells: nB = 49, one full round; H = 1", E=64, T=40, pre=1),
    _case("binary", "narrow", 65, 1, "65 cells through k_big: staged in part there too; H = 1", E=64, T=30),
    _case("zelda", "turtle", 65, 1, "no draw cache: 140 words staged", E=64, T=30, pre=8),
    # block_reset_env: 454 words a round; words mod 454 = 2, 226, 228
    _case("binary", "narrow", 12, 19, "456 words: a second round of two words", E=128, T=40),
    _case("binary", "narrow", 17, 20, "680 words: 226 in the second round (adv = RW - 1)", E=128, T=40),
    _case("binary", "narrow", 11, 31, "682 words: 228 in the second round (adv = RW + 1)", E=128, T=40),
    _case("binary", "narrow", 6, 19, "228 words: adv > RW in the first round", E=128, T=40),
    _case("binary", "wide", 12, 19, "block_reset_env without a cursor draw", E=128, T=40),
    _case("binary", "wide", 6, 19, "block_reset_env without a cursor draw", E=128, T=40),
    # the search problems and smb
    _case("sokoban", "narrow", 5, 5, "k_step_solver / tick: 2 x 76 words staged", E=256, T=40),
    _case("mdungeon", "narrow", 9, 5, "k_step_solver / tick", E=256, T=40),
    _case("ddave", "narrow", 9, 5, "k_step_solver / tick", E=256, T=40),
    _case("smb", "narrow", 9, 3, "k_smb: 27 cells", E=128, T=30),
]
CASE = {c.name: c for c in CASES}
assert len(CASE) == len(CASES)
RESET_CALLS = 12          # reset() called this often moves the cursor through the wrap classes


def has_cache(case):
    return case.rep == "narrow"          # DevBufs::fifo: the narrow representation's draw cache (whichever kernel steps it)


def need_words(case, step_draws=False, gen_map=True):
    """wave_reset_env's `need`: what a reset reads of the ring from its cursor on."""
    return (8 if step_draws else 0) + (2 * case.w * case.h if gen_map else 0) + 8 + (FIFO_N + 1 if has_cache(case) else 0)


def is_partial(case, pend=0, step_draws=False):
    return pend + need_words(case, step_draws) + 2 <= 226


def seeds_of(case):
    """The seed of every environment: SEED0 + i, or, where a class is too rare among consecutive seeds, the seeds picked with the model
    from a larger pool (tests/stream_seeds.json, made by `python tests/stream_model.py --pick`) behind the first seeds of that pool."""
    picked = _picked().get(case.name)
    if picked is not None:
        assert len(picked) <= case.E and min(picked) >= POOL_SEED0 + case.E - len(picked), (case.name, len(picked))
        return [POOL_SEED0 + i for i in range(case.E - len(picked))] + [int(s) for s in picked]
    return [SEED0 + i for i in range(case.E)]


SEED0 = 52000


@functools.lru_cache(maxsize=None)
def _picked():
    if not os.path.exists(SEEDS_JSON):
        return {}
    with open(SEEDS_JSON) as f:
        return json.load(f)


# ------------------------------------------------------------------ traces
def case_actions(case, seeds, T=None):
    """[T, E, k] random actions, an environment's drawn from its own seed (a picked environment keeps its tape)."""
    dims = ph.action_dims(case.prob, case.rep, case.w, case.h)
    return np.concatenate([ph.draw_actions(dims, np.random.RandomState((int(s) * 2654435761 + 12345) % 2 ** 32), T or case.T, 1) for s in seeds], 1)


def make_oracle(case, seed):
    o = ol.OracleEnv(case.prob, case.rep)
    for kw in case.calls:
        o.adjust_param(**kw)
    o.seed(int(seed))
    return o


def _draw_cols(d):
    return (-1, 0, 0) if d is None else d[:3]


def trace_steps(case, seeds=None, acts=None, reseed=None):
    """The oracle and the model side by side: every environment of the case seeded, reset() and put through the tape (auto-reset).
    Asserts the model's ring cursor and cursor position against the oracle's after the first reset, after every step and after every
    reset.  reseed: {t: [a new seed per environment]}: seed() before step t, in the middle of the episodes.
    -> dict: exp (the oracle's rollouts, exp[i]["map0"] the first map), cursor0 [E] / cursor [T, E] (the ring cursor after reset() /
    after every step, reset included), words [E] (consumed in all), models, and the draw records
      step  [T, E, 3]   cursor before, words for x, words for y of the step's draw (-1, 0, 0: none)
      flag  [T, E, 3]   a tile changed, done, certain (changed and changes >= max_changes or iterations >= max_iterations)
      rst   [T, E, 5]   cursor before the reset, words of the map, cursor before / words for x / words for y of its cursor draw
      rst0  [E, 5]      the same for the reset() at the start"""
    seeds = seeds_of(case) if seeds is None else seeds
    acts = case_actions(case, seeds) if acts is None else acts
    T, E = acts.shape[:2]
    assert E == len(seeds)
    step = np.zeros((T, E, 3), np.int32)
    flag = np.zeros((T, E, 3), bool)
    rst = np.full((T, E, 5), -1, np.int32)
    rst0 = np.zeros((E, 5), np.int32)
    cursor = np.zeros((T, E), np.int32)
    cursor0 = np.zeros(E, np.int32)
    untag = np.zeros((T, E), bool)          # the draw cache was dropped before this step (seed())
    exp, models = [], []
    for i, seed in enumerate(seeds):
        o = make_oracle(case, seed)
        m = StreamModel(seed, case.w, case.h, case.rep)
        maxc, maxi = o.max_changes, o.max_iterations
        for _ in range(1 + case.pre):
            ob = o.reset()
            c0, nmap, d = m.reset()
        rst0[i] = (c0, nmap) + _draw_cols(d)
        assert o.rep_cursor() == m.cursor, ("cursor after reset()", case.name, seed)
        if d is not None:
            assert tuple(ob["pos"]) == d[3:], ("position after reset()", case.name, seed)
        cursor0[i] = m.cursor
        cuts = sorted(t for t in (reseed or {}) if 0 < t < T)
        parts = []
        for a, b in zip([0] + cuts, cuts + [T]):
            if a in cuts:
                o.seed(int(reseed[a][i]))
            parts.append(o.rollout(acts[a:b, i], want_stream=True))
        x = {k: np.concatenate([p[k] for p in parts]) for k in ("maps", "pos", "heatmap", "reward", "done", "info", "stream")}
        x["map0"] = ob["map"]
        prev_changes = 0
        for t in range(T):
            if t in cuts:
                m.seed(int(reseed[t][i]))
                untag[t, i] = True
            iters, changes = int(x["info"][t, -2]), int(x["info"][t, -1])
            chg, done = changes > prev_changes, bool(x["done"][t])
            d = m.step()
            step[t, i] = _draw_cols(d)
            flag[t, i] = (chg, done, chg and (changes >= maxc or iters >= maxi))
            assert m.cursor == x["stream"][t, 0], ("cursor after step", case.name, seed, t)
            if d is not None:
                assert d[3:] == tuple(x["stream"][t, 1:3]), ("position after step", case.name, seed, t)
            prev_changes = changes
            if done:
                c0, nmap, d = m.reset()
                rst[t, i] = (c0, nmap) + _draw_cols(d)
                assert m.cursor == x["stream"][t, 3], ("cursor after the reset", case.name, seed, t)
                if d is not None:
                    assert d[3:] == tuple(x["pos"][t]), ("position after the reset", case.name, seed, t)
                prev_changes = 0
            cursor[t, i] = m.cursor
        assert int(m.rs.get_state()[2]) % MT_N == m.cursor
        exp.append(x)
        models.append(m)
    return dict(reseeded=bool(reseed), exp=exp, cursor0=cursor0, cursor=cursor, words=np.array([m.words for m in models]), models=models,
                step=step, flag=flag, rst=rst, rst0=rst0, acts=acts, seeds=list(seeds), untag=untag)


@functools.lru_cache(maxsize=None)
def case_trace(name):
    return trace_steps(CASE[name])


def trace_resets(case, tr, calls=RESET_CALLS):
    """reset() called `calls` times on every environment at the end of the tape `tr` (trace_steps; where the ring cursors of the
    environments have drifted apart -- from seed() on they would pass the same few slots) -> rst [calls, E, 5] (as trace_steps),
    cursor [calls, E], maps / pos of the oracle after every call, models, words.  Oracles of their own are put through the tape
    again and then through the same calls, their ring cursor and cursor position asserted; `tr` is left as it is."""
    assert not tr["reseeded"]
    E = len(tr["seeds"])
    rst = np.zeros((calls, E, 5), np.int32)
    cursor = np.zeros((calls, E), np.int32)
    maps = np.zeros((calls, E, case.h, case.w), np.uint8)
    pos = np.zeros((calls, E, 2), np.int64)
    models = []
    for i, seed in enumerate(tr["seeds"]):
        o = make_oracle(case, seed)
        for _ in range(1 + case.pre):
            o.reset()
        o.rollout(tr["acts"][:, i], want_maps=False, want_heat=False)
        m = tr["models"][i].clone()
        assert o.rep_cursor() == m.cursor, ("cursor at the end of the tape", case.name, seed)
        for k in range(calls):
            c0, nmap, d = m.reset()
            rst[k, i] = (c0, nmap) + _draw_cols(d)
            cursor[k, i] = m.cursor
            ob = o.reset()
            assert o.rep_cursor() == m.cursor, ("cursor after reset()", case.name, tr["seeds"][i], k)
            if d is not None:
                pos[k, i] = d[3:]
                assert tuple(ob["pos"]) == d[3:], ("position after reset()", case.name, tr["seeds"][i], k)
            maps[k, i] = ob["map"]
        models.append(m)
    return dict(rst=rst, cursor=cursor, maps=maps, pos=pos, models=models, words=np.array([m.words for m in models]))


@functools.lru_cache(maxsize=None)
def case_resets(name):
    return trace_resets(CASE[name], case_trace(name))


# ------------------------------------------------------------------ the census
def _reset_classes(case, out, rows, envs, kind, pend=None, sdraw=None):
    """The classes of resets `rows` [n, 5] (environment envs[n]).  kind (one, or one per reset): "p" -- "/p" or "/f" by the reset's
    own staging rule; "f", "b", "u" -- that suffix, the whole ring;
    pend [n]: cache words patched in; sdraw [n, 3]: the step draw the reset consumes itself (step_draws)."""
    n = len(rows)
    pend = np.zeros(n, np.int64) if pend is None else pend
    for j in range(n):
        c0, nmap, dc, kx, ky = (int(v) for v in rows[j])
        e = int(envs[j])
        sd = sdraw is not None and sdraw[j][0] >= 0
        kj = kind if isinstance(kind, str) else kind[j]
        if kj != "p":
            sfx, partial = "/" + kj, False
        else:
            partial = is_partial(case, int(pend[j]), sd)
            sfx = "/p" if partial else "/f"
        start = (int(sdraw[j][0]) if sd else c0)
        base = (start - int(pend[j])) % MT_N
        length = int(pend[j]) + need_words(case, sd) + 2
        if base + length > MT_N:
            out["WRAP-a"].append(e)
        if partial and (base + MT_M) % MT_N + length > MT_N:
            out["WRAP-m"].append(e)
        draws = [(dc, kx, ky, "R8")] if dc >= 0 else []
        if sd:
            skx, sky = int(sdraw[j][1]), int(sdraw[j][2])
            draws.append((int(sdraw[j][0]), skx, sky, "RS8"))
            if skx + sky <= FIFO_N and kx + ky > FIFO_N:
                out["RS+R8"].append(e)
        for c, kx_, ky_, cls in draws:
            if c + FIFO_N > MT_N:
                out["WRAP-8"].append(e)
            if case.w == 1 or case.h == 1:
                out["AXIS"].append(e)
            if kx_ + ky_ > FIFO_N:
                if cls == "RS8":
                    out["RS8"].append(e)
                else:
                    out["R8" + sfx].append(e)
                    if kx_ > FIFO_N:
                        out["R8-x" + sfx].append(e)
            if cls == "R8" and kx_ == FIFO_N and case.h > 1:
                out["R8-x@8" + sfx].append(e)
            if cls == "R8" and kx_ + ky_ == FIFO_N:
                out["R=8" + sfx].append(e)


def census(case, route, tr=None):
    """{class: [environment of every occurrence]} for one case on one route:
      reset    reset() called RESET_CALLS times (k_reset; k_big for the big maps)
      fused    step() / rollout() on k_step           two      the same tape with no_fused = 1 (k_update + k_stats)
      block / big / solver / smb / async              step() (tick()) on the kernels of that route"""
    from collections import defaultdict
    out = defaultdict(list)
    if route == "reset":
        tr = case_resets(case.name) if tr is None else tr
        calls, E = tr["rst"].shape[:2]
        _reset_classes(case, out, tr["rst"].reshape(calls * E, 5), np.tile(np.arange(E), calls), "p")
        return dict(out)
    tr = case_trace(case.name) if tr is None else tr
    T, E = tr["step"].shape[:2]
    step, flag, rst = tr["step"], tr["flag"], tr["rst"]
    k = step[..., 1] + step[..., 2]
    draws = step[..., 0] >= 0
    chg, done, certain = flag[..., 0], flag[..., 1], flag[..., 2]
    foreseen = certain | (done & ~chg)          # k_step: the update knows (sure_done, or nothing changed and the episode is over)
    tt, ee = np.nonzero(done)
    if route != "fused":
        for t, e in zip(*np.nonzero(draws)):
            if k[t, e] > SPEC_DRAWS:
                out["S6"].append(int(e))
            if step[t, e, 0] + SPEC_DRAWS + 1 > MT_N:
                out["WRAP-8s"].append(int(e))
            if case.w == 1 or case.h == 1:
                out["AXIS"].append(int(e))
        # k_stats_wide: a reset the update foresaw (a lone item) and one at the end of a full recomputation go through block_reset_env;
        # an episode end nobody foresaw on an incremental item is reset by one wavefront (wave_incremental_item -> wave_reset_env).
        # Which of the two an unforeseen end takes depends on the champion component, which the model does not know: "/u"
        _reset_classes(case, out, rst[tt, ee], ee, np.where(foreseen[tt, ee], "b", "u") if route == "block" else "p")
        return dict(out)
    # k_step: the draw cache.  tag_ok: fifo_tag == cursor when the step starts (a reset rebuilds the cache; a fallback leaves -1)
    pend = np.zeros((T, E), np.int64)
    for e in range(E):
        tag_ok = True
        for t in range(T):
            if tr["untag"][t, e]:
                tag_ok = False
            if draws[t, e] and not foreseen[t, e]:
                if not tag_ok:
                    out["TAG"].append(e)
                c0, kx, ky = (int(v) for v in step[t, e])
                s8 = kx + ky > FIFO_N
                if kx > FIFO_N:
                    out["S8-x"].append(e)
                elif s8:
                    out["S8-y"].append(e)
                if kx == FIFO_N and case.h > 1:
                    out["S8-x@8"].append(e)
                if c0 + FIFO_N > MT_N or (not s8 and (c0 + FIFO_N) % MT_N + FIFO_N + 1 > MT_N):
                    out["WRAP-8s"].append(e)
                if case.w == 1 or case.h == 1:
                    out["AXIS"].append(e)
                tag_ok = not s8
                if done[t, e]:          # nobody foresaw it
                    if s8:
                        out["PEND-after-S8"].append(e)
                    elif kx + ky >= 1:
                        out["PEND"].append(e)
                        pend[t, e] = kx + ky
            if done[t, e]:
                tag_ok = True
    sdraw = np.where((foreseen & draws)[tt, ee][:, None], step[tt, ee], -1)
    _reset_classes(case, out, rst[tt, ee], ee, "f", pend=pend[tt, ee], sdraw=sdraw)
    return dict(out)


def _p_more_than(case, n, x_only=False, exactly_x=None):
    """Probability that randint(W), randint(H) need more than n words / that x alone does / that x is accepted on word exactly_x."""
    def rej(v):
        if v <= 1:
            return None
        m = 1
        while m < v:
            m *= 2
        return 1.0 - v / m
    qx, qy = rej(case.w), rej(case.h)
    if exactly_x is not None:
        return 0.0 if qx is None or case.h == 1 else qx ** (exactly_x - 1) * (1 - qx)
    if qx is None:
        return 0.0 if (x_only or qy is None) else qy ** n
    if x_only:
        return qx ** n
    if qy is None:
        return qx ** n
    # P(kx + ky > n) = P(kx > n) + sum_{i <= n} P(kx = i) P(ky > n - i)
    return qx ** n + sum(qx ** (i - 1) * (1 - qx) * qy ** (n - i) for i in range(1, n + 1))


def applicable(case, route):
    """{class: None (must meet the floor) or the reason it is out of reach} for a case on a route.
    A class tied to rejection is out of reach where its probability per draw, worked out from the shape's rejection rates, times the
    largest budget a case may have (512 environments x 60 steps, were every step a draw of that kind) stays below 6, twice the floor:
    no choice of seeds within the limits gets there.  The rest follows from the route and the shape."""
    budget = MAX_ENVS * MAX_STEPS

    def rare(p, what):
        if p == 0.0:
            return "cannot occur: %s" % what
        if p * budget < 2 * FLOOR_COUNT:
            return "out of reach: %.1e a draw (%s), %.2f expected in %d draws" % (p, what, p * budget, budget)
        return None

    cursor = case.rep != "wide"
    axis = case.w == 1 or case.h == 1
    pow2 = all(v & (v - 1) == 0 for v in (case.w, case.h))
    why_rej = "%d x %d rejects %s" % (case.w, case.h, "no word" if pow2 else "too few words")
    out = {}
    no_cursor = "the wide representation draws no cursor position"
    kinds = {"reset": "p", "fused": "f", "block": "b"}.get(route, "p")
    if kinds == "p":
        part = is_partial(case)
        sfx, other = ("/p", "/f") if part else ("/f", "/p")
    else:
        part, sfx, other = False, "/" + kinds, None
    whole = "counted, no floor: the whole ring is staged, its length does not hang on the eighth word"
    unforeseen = ("counted, no floor: an episode end nobody foresaw is reset by block_reset_env behind a full recomputation and by one "
                  "wavefront (wave_incremental_item -> wave_reset_env) on an incremental item; the model does not tell them apart, and the "
                  "tall cases have 0 to 10 such resets each, so those two sites are barely exercised")
    for cls, p in (("R8", _p_more_than(case, FIFO_N)), ("R8-x", _p_more_than(case, FIFO_N, x_only=True)), ("R8-x@8", _p_more_than(case, 0, exactly_x=FIFO_N)),
                   ("R=8", _p_more_than(case, FIFO_N - 1) - _p_more_than(case, FIFO_N))):
        out[cls + sfx] = no_cursor if not cursor else (whole if cls == "R=8" and sfx != "/p" else rare(p, why_rej))
        if route == "block":
            out[cls + "/u"] = unforeseen
        if other:
            out[cls + other] = ("k_step compiles PARTIAL = false" if route == "fused" else
                                "%d words: staged %s on every reset of this route" % (need_words(case) + 2, "in part" if part else "whole"))
    if route == "fused":
        out["R8/p"] = out["R8-x/p"] = out["R8-x@8/p"] = out["R=8/p"] = "partial staging in the fused kernel: it compiles PARTIAL = false"
    tiny = "a reset takes 2 words and a step none: %d steps and %d reset() calls stay below slot 623" % (MAX_STEPS, RESET_CALLS)
    out["WRAP-a"] = tiny if case.w * case.h == 1 else None
    out["WRAP-m"] = tiny if case.w * case.h == 1 else None if part else ("the whole ring is staged" if kinds != "b" else "block_reset_env stages the whole ring")
    out["WRAP-8"] = (no_cursor if not cursor else
                     ("neither axis draws: no candidate words" if case.w == 1 and case.h == 1 else None))
    out["AXIS"] = "no axis of one cell" if not axis else (None if cursor else no_cursor)
    narrow = case.rep == "narrow"
    no_draw = "the %s representation's steps draw nothing" % case.rep
    if route == "reset":
        pass
    elif route == "fused":
        ps8 = _p_more_than(case, FIFO_N)
        out["S8-x"] = no_draw if not narrow else rare(_p_more_than(case, FIFO_N, x_only=True), why_rej)
        out["S8-y"] = no_draw if not narrow else rare(ps8 - _p_more_than(case, FIFO_N, x_only=True), why_rej + " for y after x")
        out["S8-x@8"] = no_draw if not narrow else rare(_p_more_than(case, 0, exactly_x=FIFO_N), why_rej)
        out["TAG"] = no_draw if not narrow else rare(ps8, why_rej + "; seed() and load_state_dict() have a test of their own")
        out["RS8"] = no_draw if not narrow else rare(ps8, why_rej)
        out["RS+R8"] = no_draw if not narrow else rare(ps8, why_rej)
        out["PEND"] = no_draw if not narrow else ("neither axis draws: no cache word is ever taken" if case.w == 1 and case.h == 1 else None)
        # (an S8 and an episode end nobody foresaw in one step: on the oracle's tapes of these cases 2 to 12 steps in 1 000 end that
        #  way; one in twenty is taken as the bound)
        out["PEND-after-S8"] = no_draw if not narrow else rare(ps8 / 20, why_rej + ", and at most one step in twenty ends an episode unforeseen")
        out["WRAP-8s"] = no_draw if not narrow else out["WRAP-8"]
    else:
        out["S6"] = no_draw if not narrow else rare(_p_more_than(case, SPEC_DRAWS), why_rej)
        out["WRAP-8s"] = no_draw if not narrow else out["WRAP-8"]
    for (name, r, cls), why in OUT_OF_REACH.items():
        if name == case.name and r == route:
            out[cls] = "out of reach: " + why
    return out


# What the model shows to be out of reach of a case although the class applies to its route, with the reasoning.
OUT_OF_REACH = {
    ("binary-narrow-8x8", "reset", "WRAP-8"):
        "8 x 8 rejects no word: a step takes exactly 2 words, a reset 130, and every environment's cursor is 130 r + 2 s after r resets "
        "and s steps; behind a tape of 60 steps the reset draws start at 130 r + 248 mod 624, which is 618, 620 or 622 for no r "
        "(130 r mod 624 is a multiple of 26; 370, 372, 374 are not).  The step routes reach it: there s varies",
}


def routes_of(case):
    """The routes a case is run on (and counted for)."""
    r = ["reset", case.route]
    if case.route == "fused":
        r.append("two")
    return r


def check_floor(case, route, counts=None):
    """-> (table rows [(class, count, environments, reason or None)], the classes that apply and miss the floor)"""
    counts = census(case, route) if counts is None else counts
    rows, missing = [], []
    app = applicable(case, route)
    for cls in sorted(set(app) | set(counts)):
        n, ne = len(counts.get(cls, ())), len(set(counts.get(cls, ())))
        reason = app.get(cls, "not a class of this route")
        rows.append((cls, n, ne, reason))
        if reason is None and (n < FLOOR_COUNT or ne < FLOOR_ENVS):
            missing.append((cls, n, ne))
    return rows, missing


def format_table(case, route, rows):
    head = "%-22s %-7s %s" % (case.name, route, case.note)
    return "\n".join([head] + ["    %-16s %6d in %4d envs%s" % (c, n, ne, "" if why is None else "   [%s]" % why) for c, n, ne, why in rows])


# ------------------------------------------------------------------ picking seeds from a pool
def beyond_prefix(seeds):
    """The seeds of a sorted list that are not part of its run POOL_SEED0, POOL_SEED0 + 1, ... (what seeds_of() fills in itself)."""
    k = 0
    while k < len(seeds) and seeds[k] == POOL_SEED0 + k:
        k += 1
    return [int(v) for v in seeds[k:]]


def pick_seeds(case, pool=8192, chunk=1024, seed0=POOL_SEED0):
    """Where consecutive seeds miss a class that applies: seeds from a pool `pool` wide whose environments hold the missing classes
    (up to twice the floor of each), filled up with the first seeds of the pool to the case's E.  -> (seeds, classes still short)"""
    want = 2 * FLOOR_COUNT
    chosen, have = [], {}
    routes = routes_of(case)
    short = []
    for c0 in range(0, pool, chunk):
        seeds = [seed0 + c0 + i for i in range(chunk)]
        tr = trace_steps(case, seeds=seeds)
        per_route = {r: census(case, r, tr=tr) for r in routes[1:]}
        per_route["reset"] = census(case, "reset", tr=trace_resets(case, tr))
        short = []
        for route in routes:
            for cls, why in applicable(case, route).items():
                if why is not None:
                    continue
                for e in per_route[route].get(cls, ()):
                    if have.get((route, cls), 0) >= want:
                        break
                    s_ = seeds[e]
                    if s_ not in chosen:
                        chosen.append(s_)
                        for r2 in routes:          # what else this environment brings
                            for cls2, envs in per_route[r2].items():
                                have[(r2, cls2)] = have.get((r2, cls2), 0) + envs.count(e)
                if have.get((route, cls), 0) < want:
                    short.append((route, cls, have.get((route, cls), 0)))
        if not short:
            break
    assert len(chosen) <= case.E, (case.name, len(chosen))
    fill = [seed0 + i for i in range(pool) if seed0 + i not in set(chosen)]
    return sorted(chosen + fill[:case.E - len(chosen)]), short


if __name__ == "__main__":
    import sys
    if "--pick" in sys.argv:
        names = [a for a in sys.argv[1:] if not a.startswith("--")]
        picked = dict(_picked())
        for name in names or [c.name for c in CASES]:
            if any(check_floor(CASE[name], r)[1] for r in routes_of(CASE[name])):
                seeds, short = pick_seeds(CASE[name])
                picked[name] = beyond_prefix(seeds)
                print(name, "picked", len(picked[name]), "still short:", short, flush=True)
                with open(SEEDS_JSON, "w") as f:
                    json.dump(picked, f, indent=0)
    else:
        for c in CASES:
            for r in routes_of(c):
                rows, missing = check_floor(c, r)
                print(format_table(c, r, rows))
                if missing:
                    print("    MISSING", missing)
