"""Maps beyond 64 x 64 (csrc/bigmap.h, bigmap_team.h, kernels_big.h, the big-map branch of kernels_update.h, k_obs on byte maps) at
the edges of their word, row and work-item layout, every step against the CPU oracle (parity_harness.run_config: reward, done, every
info key, cursor, heat map; the map every few steps and at the end).  None of that code runs on the host simulator, so this is its check.

  A  binary, a matrix of shapes around KW = ceil(W / 64) = 2 | 3 | 4 | 16 | 64, H = 128 | 129, full and one-bit last words, the
     largest cursor maps and the two sides of the incremental route's size limit -- each with the default tile mix and an open one,
     with one wavefront per map and by whole blocks (big_team), with and without the incremental route (no_inc)
  B  the environment field of the incremental work item: 32 768 environments (route on) and 32 769 (off)
  C  zelda and the search problems with a map side above 64
  E  the size limits themselves
(D, the bound observation on such maps, is in test_gpu_parity.py::test_bound_observation_every_step.)

The cases would prove little if no episode ended, no change fell into the upper rows / words or all changes took one route of the
update kernel, so each case states what its tape has to contain (coverage_a, coverage_c): computed from the ORACLE's maps alone,
before the library is asked anything.  `PYTHONPATH=. python tests/test_gpu_bigmap_edges.py` prints those figures on a machine without a GPU.
With the committed seeds the oracle gave (A, summed over both mixes of the named shapes):
    changed cells with row >= 128:            128x129 + 255x255                 148
    changed cells with column >= 192:         193x70 + 255x255                   68
    changed cells with column in 128..191:    129x128 + 192x70 + 193x70         232
    share of changed cells in or next to the largest region, per case: open mix 0.40 .. 0.98, default mix 0.08 .. 0.41
    (with the problem's default random_probs only an environment's first map follows `probs`, the later ones draw their own tile
    probabilities -- hence 0.4 .. 0.65 on the two-dimensional shapes; the maps of one or two rows / columns get THIN_OPEN instead)
    zelda: steps with nearest-enemy > 0: 1 514, with path-length > 0: 137
    steps in which the planner ran: sokoban 50, mdungeon 66x12 213, mdungeon 100x100 37, ddave 40
The oracle is the cost of this module: 0.4 s a step on 255 x 255, about 1 s on 1000 x 70 and 4096 x 15; the 255 x 255 case is as long
as the column >= 192 condition needs (193x70 gave none of those cells), the two widest ones are a few steps long.

What guards what (the three mutations of the issue, by reading the kernels):
  * WL_INCBIG_ENV_MASK narrowed to 0x3FFF sends the items of environments >= 16 384 to e - 16 384: B's sample 16 352 .. 16 415 and the twin;
  * G.magic without the "+ 1" is wrong only where KW does not divide 65 536, i.e. KW = 3 ((3 * 21 845) >> 16 = 0): 129x128 and 192x70
    in A, 129x20 and 193x66 in C;
  * the "!inc &&" in front of WL_RESET_ONLY in k_big cannot be caught by any test: an incremental item leaves the loop (continue)
    before reset_only is read, so the guard changes nothing that runs.  Rows >= 128 of incremental items (bit 30) are what the
    row >= 128 cases step through all the same.
"""
import os
import re

import numpy as np
import pytest

import oracle_lib as ol
import parity_harness as ph

pytestmark = pytest.mark.gpu

OPEN = {"empty": 0.9, "solid": 0.1}
NO_INC_ABOVE = 256            # champ_bytes(): the incremental route exists up to 256 per side ...
INC_MAX_ENVS = 32768          # ... and up to that many environments (the work item's 15-bit field)


def _cp(w, h, changes):
    """change_percentage for which max_changes = int(cp * w * h) is `changes`, half a change away from either neighbour."""
    return (changes + 0.5) / (w * h)


# ---------------------------------------------------------------------------------------------------------------- A
# (w, h, representation, further adjust_param calls, max_changes, E, T, also by one wavefront per map)
A_SHAPES = [
    (65, 1, "narrow", {}, 6, 8, 100, False),
    (1, 65, "turtle", {}, 5, 8, 150, False),
    (65, 64, "turtle", {}, 5, 8, 150, False),
    (64, 65, "narrow", {}, 6, 8, 100, False),
    (128, 128, "narrow", {}, 8, 6, 100, True),
    (129, 128, "turtle", {"warp": True}, 5, 8, 150, True),
    (128, 129, "narrow", {}, 8, 6, 100, True),
    (192, 70, "narrow", {}, 8, 6, 100, True),
    (193, 70, "narrow", {}, 8, 6, 100, True),
    (255, 255, "narrow", {}, 10, 4, 120, True),
    (255, 2, "turtle", {}, 5, 8, 150, False),
    (2, 255, "narrow", {}, 6, 8, 100, False),
    (256, 66, "wide", {}, 8, 5, 80, False),
    (257, 66, "wide", {}, 8, 5, 80, False),
    (1000, 70, "wide", {}, 4, 2, 16, False),       # (the oracle takes about 1 s per step on maps of this size: few steps, short episodes)
    (4096, 15, "wide", {}, 4, 2, 16, False),
]
A_SEED = 4100


def _a_cases():
    out = []
    for w, h, rep, extra, mc, E, T, lone in A_SHAPES:
        for mix in ("default", "open"):
            variants = ["default"] + (["wave_per_map"] if lone else []) + (["no_inc"] if max(w, h) <= NO_INC_ABOVE else [])
            for v in variants:
                out.append(pytest.param(w, h, rep, mix, v, id="%dx%d-%s-%s-%s" % (w, h, rep, mix, v)))
    return out


# The open mix of the maps of one or two rows / columns.  A line of cells has no giant region at 10 % of solid (its regions are runs of
# about ten cells), and with the problem's default random_probs only an environment's FIRST map follows `probs` at all (problem.py:
# reset() draws new tile probabilities for the next one): 1 % of solid on every map, and episodes too short to chop the line up.
THIN_OPEN = dict(probs={"empty": 0.99, "solid": 0.01}, random_probs=False)
THIN_OPEN_CHANGES = 4


def a_config(w, h, rep, mix):
    extra, mc, E, T = next((s[3], s[4], s[5], s[6]) for s in A_SHAPES if (s[0], s[1], s[2]) == (w, h, rep))
    thin_open = mix == "open" and min(w, h) <= 2
    calls = [dict(width=w, height=h), dict(change_percentage=_cp(w, h, THIN_OPEN_CHANGES if thin_open else mc), **extra)]
    if mix == "open":
        calls.append(dict(THIN_OPEN) if thin_open else dict(probs=dict(OPEN)))
    return "binary", rep, calls, E, T, A_SEED + 7 * w + h


_TAPES, _BIG_TAPE = {}, {}
_KEEP_BYTES = 48 << 20


def _tape(key, prob, rep, calls, E, T, seed0, sample=None):
    """The oracle's side of a case, made once per process whatever the order of the tests; only the tapes of the largest maps (tens of
    megabytes each) are kept one at a time, for the variants of the same case that follow."""
    if key in _TAPES:
        return _TAPES[key]
    if key not in _BIG_TAPE:
        _BIG_TAPE.clear()
        tape = ph.oracle_tape(prob, rep, calls, E, T, seed0, np.random.RandomState(seed0), sample)
        if sum(x["maps"].nbytes + x["heatmap"].nbytes for x in tape[1]) <= _KEEP_BYTES:
            _TAPES[key] = tape
            return tape
        _BIG_TAPE[key] = tape
    return _BIG_TAPE[key]


def changed_cells(x):
    """The cells one oracle rollout changed, from its maps: [(step, row, column)] for the steps that did not end an episode (the map
    a step ended on is replaced by the fresh one before anyone sees it)."""
    out = []
    prev = x["map0"]
    for t in range(len(x["done"])):
        cur = x["maps"][t]
        if not x["done"][t]:
            d = np.argwhere(cur != prev)
            assert len(d) <= 1, "a step changes at most one cell"
            if len(d):
                out.append((t, int(d[0, 0]), int(d[0, 1])))
        prev = cur
    return out


def largest_region(passable):
    """Mask of the largest 4-connected region of `passable` [H, W] (the first in row-major order among equals): every cell starts
    with its own index as label and takes the smallest label of its horizontal run, then of its vertical run, until nothing moves."""
    H, W = passable.shape
    n = int(passable.sum())
    if n == 0:
        return np.zeros_like(passable)
    cid = np.full((H, W), -1, np.int64)
    cid[passable] = np.arange(n)

    def runs(p):        # cells of p in row-major order: where each run along a row starts, and the run of each cell
        first = p.copy()
        first[:, 1:] &= ~p[:, :-1]
        f = first[p]
        return np.flatnonzero(f), np.cumsum(f) - 1

    h_start, h_run = runs(passable)
    order_v = cid.T[passable.T]                      # the same cells in column-major order
    v_start, v_run = runs(passable.T)
    lab = np.arange(n)
    while True:
        before = lab
        lab = np.minimum.reduceat(lab, h_start)[h_run]
        lv = lab[order_v]
        lab = lab.copy()
        lab[order_v] = np.minimum.reduceat(lv, v_start)[v_run]
        if np.array_equal(lab, before):
            break
    ids, counts = np.unique(lab, return_counts=True)
    out = np.zeros((H, W), bool)
    out[passable] = lab == ids[np.argmax(counts)]
    return out


def coverage_a(exp):
    """What the tape of one case of A contains, from the oracle's rollouts: episodes ended, changed cells (all, with row >= 128, with
    column in 128..191, with column >= 192) and how many of them were inside or 4-adjacent to the largest region of the map before
    the change -- the update kernel's routing decision (kernels_update.h: in or next to the champion = full recomputation)."""
    c = dict(done=0, changed=0, row128=0, col128=0, col192=0, near=0)
    for x in exp:
        c["done"] += int(x["done"].sum())
        for t, r, q in changed_cells(x):
            before = x["maps"][t - 1] if t else x["map0"]
            big = largest_region(before == 0)
            H, W = big.shape
            near = any(0 <= rr < H and 0 <= qq < W and big[rr, qq] for rr, qq in ((r, q), (r - 1, q), (r + 1, q), (r, q - 1), (r, q + 1)))
            c["changed"] += 1
            c["row128"] += r >= 128
            c["col128"] += 128 <= q < 192
            c["col192"] += q >= 192
            c["near"] += near
    return c


_COVER_A = {}      # (w, h, mix) -> coverage_a of the case's tape


def cover_a(w, h, mix):
    """coverage_a of one case, computed once per process (the tape may be gone by the time the sums are asked for)."""
    if (w, h, mix) not in _COVER_A:
        rep = next(s[2] for s in A_SHAPES if (s[0], s[1]) == (w, h))
        prob, rep, calls, E, T, seed0 = a_config(w, h, rep, mix)
        _COVER_A[(w, h, mix)] = coverage_a(_tape(("A", w, h, mix), prob, rep, calls, E, T, seed0)[1])
    return _COVER_A[(w, h, mix)]


def check_case_a(w, h, mix):
    """What every case of A has to contain by itself: an episode that ends, a changed cell, and its mix's side of the routing decision."""
    c = cover_a(w, h, mix)
    assert c["done"] >= 1 and c["changed"] >= 1, ("the tape ends no episode / changes no cell", w, h, mix, c)
    if mix == "open":
        assert 3 * c["near"] >= c["changed"], ("open mix: under a third of the changes in or next to the largest region", w, h, c)
    else:
        assert 3 * (c["changed"] - c["near"]) >= c["changed"], ("default mix: under a third of the changes away from the largest region", w, h, c)


A_SUMS = ((((128, 129), (255, 255)), "row128", "row >= 128"), (((193, 70), (255, 255)), "col192", "column >= 192"),
          (((129, 128), (192, 70), (193, 70)), "col128", "column in 128..191"))


def check_sums_a():
    for shapes, field, what in A_SUMS:
        n = sum(cover_a(w, h, m)[field] for w, h in shapes for m in ("default", "open"))
        assert n >= 50, ("under 50 changed cells with " + what, shapes, n)
    # the two border shapes by themselves: the one row beyond 128 and the one column beyond 128 are changed at all
    assert sum(cover_a(128, 129, m)["row128"] for m in ("default", "open")) >= 1 and sum(cover_a(129, 128, m)["col128"] for m in ("default", "open")) >= 1


@pytest.mark.parametrize("w,h,rep,mix,variant", _a_cases())
def test_binary_geometry_matrix_vs_oracle(w, h, rep, mix, variant):
    """A: see the module's docstring and A_SHAPES.  65x1 .. 64x65: the smallest such maps, a one-bit last word, one row / one column.
    128x128: the last size of the register-resident sweep (big128_fits), a full last word.  129x128 / 128x129: the first sizes off it.
    192x70 / 193x70: KW 3 -> 4.  255x255, 255x2, 2x255: rows and columns up to 254 (work-item bits 22 and 30).  256x66 / 257x66:
    with / without the incremental route.  1000x70: KW = 16.  4096x15: KW = 64, NW * KW = 61 440, the top of big_row's range."""
    prob, rep, calls, E, T, seed0 = a_config(w, h, rep, mix)
    check_case_a(w, h, mix)
    acts, exp = _tape(("A", w, h, mix), prob, rep, calls, E, T, seed0)
    tuning = {"default": None, "wave_per_map": {"big_team": 0}, "no_inc": {"no_inc": 1}}[variant]
    err = ph.run_config(prob, rep, calls, E, T, seed0, None, False, tuning=tuning, tape=(acts, exp))
    assert err is None, err


def test_binary_geometry_tapes_reach_the_upper_rows_and_words():
    """A: over the cases of 128x129 and 255x255 at least 50 changed cells have row >= 128 (bit 30 of the work item, WL_RESET_ONLY on the
    other lists), over 193x70 and 255x255 at least 50 a column >= 192, over 129x128, 192x70, 193x70 at least 50 a column in 128..191
    -- from the oracle's tapes, whichever of the cases ran in this process (their coverage is kept, else made here)."""
    check_sums_a()


# ---------------------------------------------------------------------------------------------------------------- B
def _b_calls():
    return [dict(width=65, height=2), dict(change_percentage=_cp(65, 2, 4))]


def _b_sample(N):
    return np.unique(np.concatenate([np.arange(0, 32), np.arange(16352, 16416), np.arange(32736, N), np.linspace(0, N - 1, 200).astype(int)]))


@pytest.mark.parametrize("N", [INC_MAX_ENVS, INC_MAX_ENVS + 1])
def test_environment_field_of_the_work_item_vs_oracle(N):
    """B: binary narrow 65 x 2 with 32 768 environments (the incremental route is on: indices up to 0x7FFF in the item's 15 bits) and
    with 32 769 (champ_bytes switches it off); the first, the middle (around 16 384: the field's top bit), the last and 200 spread
    environments against the oracle at every step."""
    calls, T, seed0 = _b_calls(), 40, 5200
    sample = _b_sample(N)
    acts, exp = _tape(("B", N), "binary", "narrow", calls, N, T, seed0, sample)
    assert sum(int(x["done"].sum()) for x in exp) >= len(exp) and sum(len(changed_cells(x)) for x in exp) >= len(exp)
    err = ph.run_config("binary", "narrow", calls, N, T, seed0, None, False, sample=sample, tape=(acts, exp))
    assert err is None, err


def test_environment_field_of_the_work_item_twin_without_the_route():
    """B: the oracle sample cannot see an item that lands on an environment outside it; the same batch with the route off
    (no_inc) can: map, reward, done, info and counters of ALL 32 768 environments, bitwise, every tenth step and at the end."""
    import torch
    from gym_pcgrl_amd.envs import BatchedPcgrlEnv
    N, T, seed0 = INC_MAX_ENVS, 40, 5200
    a = BatchedPcgrlEnv(prob="binary", rep="narrow", num_envs=N, seed=seed0)
    b = BatchedPcgrlEnv(prob="binary", rep="narrow", num_envs=N, seed=seed0, tuning={"no_inc": 1})
    try:
        for kw in _b_calls():
            a.adjust_param(**kw); b.adjust_param(**kw)
        a.reset(); b.reset()
        acts = ph.draw_actions([a.single_action_space.n], np.random.RandomState(seed0), T, N)[:, :, 0]
        for t in range(T):
            a.step(acts[t]); b.step(acts[t])
            if t % 10 == 9 or t == T - 1:
                for name in ("map", "reward", "done", "info", "counters"):
                    x, y = a._bufs[name], b._bufs[name]
                    if not torch.equal(x, y):
                        bad = torch.nonzero((x != y).reshape(N, -1).any(1))[:, 0]
                        raise AssertionError((name, "step", t, "environments", bad[:8].tolist(), "of", int(bad.numel())))
        a.check_status(); b.check_status()
    finally:
        a.close(); b.close()


# ---------------------------------------------------------------------------------------------------------------- C
def _zelda_sparse(w, h):
    one = 1.0 / (w * h)       # player, key and door: one of each expected on a fresh map
    return {"empty": 0.93 - 3 * one, "solid": 0.04, "player": one, "key": one, "door": one, "bat": 0.01, "scorpion": 0.01, "spider": 0.01}


# (w, h, representation, max_changes, E, T)
C_ZELDA = [(129, 20, "narrow", 6, 16, 100), (20, 129, "turtle", 4, 16, 150), (193, 66, "wide", 6, 8, 80), (255, 255, "narrow", 6, 3, 60)]
C_SEED = 6300


def c_zelda_config(w, h, rep, mix):
    mc, E, T = next((s[3], s[4], s[5]) for s in C_ZELDA if (s[0], s[1], s[2]) == (w, h, rep))
    calls = [dict(width=w, height=h), dict(change_percentage=_cp(w, h, mc))]
    if mix == "sparse":
        calls.append(dict(probs=_zelda_sparse(w, h)))
    return "zelda", rep, calls, E, T, C_SEED + 3 * w + h


def _few(w, h):
    return 1.0 / (w * h)


def c_search_config(name):
    """sokoban 70 x 8 narrow, mdungeon 66 x 12 turtle, ddave 90 x 6 wide, mdungeon 100 x 100 narrow (10 404 bordered cells): the open
    mixes of parity_harness.draw_config_extra, the things a level must have exactly one of expected about once."""
    if name == "sokoban":
        w, h, rep, E, T, power = 70, 8, "narrow", 12, 80, 150
        f = _few(w, h)
        probs = {"empty": 0.96 - 3 * f, "solid": 0.04, "player": f, "crate": f, "target": f}
    elif name == "mdungeon":
        w, h, rep, E, T, power = 66, 12, "turtle", 12, 120, 200
        f = _few(w, h)
        probs = {"empty": 0.91 - 2 * f, "solid": 0.05, "player": f, "exit": f, "potion": 0.01, "treasure": 0.01, "goblin": 0.01, "ogre": 0.01}
    elif name == "ddave":
        w, h, rep, E, T, power = 90, 6, "wide", 16, 80, 200
        f = _few(w, h)         # (little solid: the planner only runs on a level of one region, which 17 % of solid leaves to few 90 x 6 levels)
        probs = {"empty": 0.962 - 3 * f, "solid": 0.03, "player": f, "exit": f, "diamond": 0.004, "key": f, "spike": 0.004}
    else:
        w, h, rep, E, T, power = 100, 100, "narrow", 5, 60, 60
        f = _few(w, h)
        probs = {"empty": 0.91 - 2 * f, "solid": 0.05, "player": f, "exit": f, "potion": 0.01, "treasure": 0.01, "goblin": 0.01, "ogre": 0.01}
    prob = "mdungeon" if name == "mdungeon100" else name
    calls = [dict(width=w, height=h), dict(change_percentage=_cp(w, h, 5), solver_power=power), dict(probs=probs)]
    return prob, rep, calls, E, T, C_SEED + 11 * w + h


C_SEARCH = ["sokoban", "mdungeon", "ddave", "mdungeon100"]


def coverage_c(prob, exp, wh=(0, 0)):
    """zelda: steps with nearest-enemy > 0 and with path-length > 0; the search problems: steps in which the planner ran (a solution
    length, or a dist-win other than the one a level without a search reports: width * height, sokoban width * height * (width + height))."""
    keys = ol.INFO_KEYS[prob]
    info = np.concatenate([x["info"] for x in exp])
    done = sum(int(x["done"].sum()) for x in exp)
    if prob == "zelda":
        return dict(done=done, enemy=int((info[:, keys.index("nearest-enemy")] > 0).sum()), path=int((info[:, keys.index("path-length")] > 0).sum()))
    unsearched = wh[0] * wh[1] * (wh[0] + wh[1] if prob == "sokoban" else 1)
    return dict(done=done, ran=int(((info[:, keys.index("dist-win")] != unsearched) | (info[:, keys.index("sol-length")] > 0)).sum()))


_COVER_C = {}


def cover_c(key):
    """coverage_c of a case of C, ("Z", w, h, mix) or ("S", name), computed once per process."""
    if key not in _COVER_C:
        if key[0] == "Z":
            rep = next(s[2] for s in C_ZELDA if (s[0], s[1]) == key[1:3])
            prob, rep, calls, E, T, seed0 = c_zelda_config(key[1], key[2], rep, key[3])
        else:
            prob, rep, calls, E, T, seed0 = c_search_config(key[1])
        exp = _tape(key, prob, rep, calls, E, T, seed0)[1]
        _COVER_C[key] = coverage_c(prob, exp, (calls[0]["width"], calls[0]["height"]))
    return _COVER_C[key]


@pytest.mark.parametrize("w,h,rep,mix", [pytest.param(s[0], s[1], s[2], m, id="%dx%d-%s-%s" % (s[0], s[1], s[2], m)) for s in C_ZELDA for m in ("default", "sparse")])
def test_zelda_large_maps_vs_oracle(w, h, rep, mix):
    """C: big_item_stats<ZELDA> (three planes, big_bfs_dist, nearest enemy) with KW = 3 and 4, H = 129 and on 255 x 255.  (The default
    mix puts dozens of players on such maps: those cases check the counting statistics and the regions, the sparse ones the paths.)"""
    prob, rep, calls, E, T, seed0 = c_zelda_config(w, h, rep, mix)
    key = ("Z", w, h, mix)
    assert cover_c(key)["done"] >= 1, ("the tape ends no episode", key)
    acts, exp = _tape(key, prob, rep, calls, E, T, seed0)
    err = ph.run_config(prob, rep, calls, E, T, seed0, None, False, tape=(acts, exp))
    assert err is None, err


def check_sums_zelda():
    c = [cover_c(("Z", s[0], s[1], m)) for s in C_ZELDA for m in ("default", "sparse")]
    assert sum(x["enemy"] for x in c) >= 30 and sum(x["path"] for x in c) >= 30, ("zelda: under 30 steps with a nearest enemy / a key-door path", c)


def test_zelda_tapes_hold_enemy_distances_and_paths():
    """C: over the zelda cases at least 30 steps with nearest-enemy > 0 and 30 with path-length > 0 in the oracle's info."""
    check_sums_zelda()


@pytest.mark.parametrize("how", ["steps", "rollout"])
@pytest.mark.parametrize("name", C_SEARCH)
def test_search_problems_with_a_side_above_64_vs_oracle(name, how):
    """C: big_map and big_search together (k_big parks the levels that need the planner, k_search_big finishes them), as single
    steps and as one rollout() tape.  In every case the planner ran in at least 20 steps of the oracle's tape."""
    prob, rep, calls, E, T, seed0 = c_search_config(name)
    key = ("S", name)
    c = cover_c(key)
    assert c["done"] >= 1 and c["ran"] >= 20, ("the tape ends no episode / the planner ran in under 20 steps", name, c)
    acts, exp = _tape(key, prob, rep, calls, E, T, seed0)
    err = ph.run_config(prob, rep, calls, E, T, seed0, None, how == "rollout", tape=(acts, exp))
    assert err is None, err


# ---------------------------------------------------------------------------------------------------------------- E
def _csrc(name):
    return open(os.path.join(ol.ROOT, "gym_pcgrl_amd", "csrc", name)).read()


def tallest_map_at(kw):
    """The largest H the library's LDS budget admits for maps of `kw` words per row, from big_wave_lds()'s formula (bigmap.h):
    bytes = PCGRL_MT_N * 4 + (BIG_NARRAYS * H * KW + 8) * 8 <= PCGRL_BIG_LDS_BUDGET, the constants read from the sources."""
    narrays = int(re.search(r"#define BIG_NARRAYS (\d+)", _csrc("bigmap.h")).group(1))
    kib = int(re.search(r"#define PCGRL_BIG_LDS_BUDGET \(\(size_t\)(\d+) \* 1024\)", _csrc("pcgrl_abi.hip")).group(1))
    mt_n = int(re.search(r"#define PCGRL_MT_N (\d+)", _csrc("pcgrl_common.h")).group(1))
    assert "(size_t)PCGRL_MT_N * 4 + ((size_t)BIG_NARRAYS * big_words(W, H) + 8) * 8" in _csrc("bigmap.h"), "big_wave_lds() changed: restate it here"
    h = ((kib * 1024 - mt_n * 4) // 8 - 8) // (narrays * kw)
    assert h * kw * kw < 65536, "big_row's range ends before the LDS budget does"
    return h


def test_largest_maps_are_taken_and_the_next_sizes_refused():
    """E: 255 x 255 narrow, 4096 x 15 wide and the tallest wide map of 16 words per row are accepted and stepped once, the
    statistics against the oracle's of the resulting maps; one more column / row is refused with ValueError."""
    from gym_pcgrl_amd.envs import BatchedPcgrlEnv
    h16 = tallest_map_at(16)
    for rep, (w, h), (w_no, h_no) in (("narrow", (255, 255), (256, 255)), ("wide", (4096, 15), (4096, 16)), ("wide", (1024, h16), (1024, h16 + 1))):
        n = 2
        env = BatchedPcgrlEnv(prob="binary", rep=rep, num_envs=n, seed=31)
        try:
            env.adjust_param(width=w, height=h)
            env.adjust_param(change_percentage=_cp(w, h, 3))
            env.reset()
            sp = env.single_action_space
            a = np.array([1] * n, np.int32) if rep == "narrow" else np.array([[w - 1, h - 1, 0], [0, 0, 1]], np.int32)
            assert hasattr(sp, "n") == (rep == "narrow")
            obs, rew, done, info = env.step(a)
            maps = obs["map"].cpu().numpy()
            for i in range(n):
                want = ol.get_stats("binary", maps[i])
                got = [int(info[k][i]) for k in ("regions", "path-length")]
                assert got == [int(want[0]), int(want[1])], (rep, w, h, i, got, want)
            assert env.check_status() == 0
        finally:
            env.close()
        env = BatchedPcgrlEnv(prob="binary", rep=rep, num_envs=n, seed=31)
        try:
            env.reset()
            with pytest.raises(ValueError):
                env.adjust_param(width=w_no, height=h_no)
                env.reset()
        finally:
            env.close()


# ---------------------------------------------------------------------------------------------------------------- the figures
def coverage_report(out=print, only=None):
    """The coverage conditions of A and C on the oracle alone (no GPU): prints every case's figures and asserts what the tests assert."""
    import time
    t0 = time.time()
    for w, h, rep in [(s[0], s[1], s[2]) for s in A_SHAPES]:
        for mix in ("default", "open"):
            if only and (w, h) not in only:
                continue
            t1 = time.time()
            c = cover_a(w, h, mix)
            out("A %4dx%-3d %-6s %-7s %5.1fs %s share %.2f" % (w, h, rep, mix, time.time() - t1, c, c["near"] / max(c["changed"], 1)))
            check_case_a(w, h, mix)
    if not only:
        check_sums_a()
        out("sums over A: " + ", ".join("%s %d" % (what, sum(cover_a(w, h, m)[f] for w, h in shapes for m in ("default", "open"))) for shapes, f, what in A_SUMS))
    for s in C_ZELDA:
        for mix in ("default", "sparse"):
            out("C zelda %dx%d %s %s %s" % (s[0], s[1], s[2], mix, cover_c(("Z", s[0], s[1], mix))))
    check_sums_zelda()
    for name in C_SEARCH:
        out("C %s %s" % (name, cover_c(("S", name))))
        assert cover_c(("S", name))["ran"] >= 20
    for N in (INC_MAX_ENVS, INC_MAX_ENVS + 1):
        _, exp = ph.oracle_tape("binary", "narrow", _b_calls(), N, 40, 5200, np.random.RandomState(5200), _b_sample(N))
        out("B N %d sample %d done %d changed %d" % (N, len(exp), sum(int(x["done"].sum()) for x in exp), sum(len(changed_cells(x)) for x in exp)))
    out("tallest map at KW = 16: %d rows; total %.0f s" % (tallest_map_at(16), time.time() - t0))


if __name__ == "__main__":
    coverage_report()
