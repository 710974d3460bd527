"""smb's play-through (csrc/kernels_smb.h: smb_search_two_label, smb_search, smb_seen_accumulate; the `cheap` rule of kernels_update.h) against
the CPU oracle, on levels chosen by what the oracle says their game does, and on every one-cell change of some of them.  All comparisons
are exact: integers and float64 rewards.  (tests/test_gpu_search_games.py does the same for sokoban, mdungeon and ddave.)

Levels.  Per (size, solver_power) a pool is mined from a fixed RandomState seed (POOLS: seed, draws, generators in turn -- random tiles
with the default weights, with `blocked` ones or nearly `open`; obstacle `course`s: floor segments, pits, walls of 1 .. H-2 cells of
solid / brick / tube, ceilings 2 .. 4 rows above the floor, stairs, a closing wall; `terraces`: blocks strewn over a floor that the
player climbs, ending in a pit too wide to cross) and classified from the oracle's output alone -- oracle_lib.get_stats(with_iters,
with_trace): the pops, the longest queue and the expansions of the two agents, the result node, the expanded states' cells:
  none_needed  H = 3: no exit column (exit_x = -1), the first pop wins
  win0         agent 0 (balance 1) won            win1      agent 0 stopped at the cap, agent 1 (balance 0) won
  out_out      both agents ran out of states      cap_cap   both stopped at the cap
  nojump       jumps = 0                          tail / gap   jumps-dist is width - the last jump's column / a wider gap between two jumps
  last_pop     the oracle's row at solver_power - 1 is another one: the last pop before the cap decides
  fell         lost, the best node in or at the left edge of a pit (the course generators say where their pits are)
  q<=255 .. q>4095   the longest balance-1 queue, counted after an expansion's four pushes: smb_search_two_label gives up (status 2, the
               search is done again by smb_search) exactly when it passes the cap -- 255 / 1 023 with smb_lds_heap 256 / 1 024, 4 095 from
               2 048 on (the label bits); 2 048 .. 4 095 are the slots in the arena, the labels in lab.b and the q >= 2048 branch of smb_climb
  left_rim     draws taken whatever the quotas say (LEFT_RIM)        flip_tells / flip_ends   the one flip the routes make changes
               jumps / jumps-dist / dist-win / makes a lost level winnable (the episode ends: in-kernel reset, MODE_START play-through)
POOLS holds the least count of every class per pool: 4 of each class the pool's size and power allow, 8 levels of tier 2 048 .. 4 095 in
the deep pools, 4 beyond 4 095 at 250 x 8.  What they do not allow, on the oracle:
  cap_out / out_cap  never: visited is keyed by (x, y, airTime), which is all a state's children depend on, so both agents expand the same
               set of states and run out of them after the same 4 * states + 1 pops -- one at the cap and one out cannot be.
  out_out      not at H <= 6: rows above the screen are free, a jump from the start rises four rows, so the player gets over any wall and
               only a pit wider than a jump stops it -- no level in 1 500 .. 6 000 draws runs out of states there.  At 24 x 8 walls confine.
  win1, cap_*  not at power 10 000 on 30 x 8 (none in 600 draws: every search ends long before) -- nor at 114 x 14 / 122 x 32 with random
               tiles; the terraces give cap_cap there.  win1 needs a cap that agent 0 reaches: the pools of power 60 .. 2 000.
  q>4095       not at W <= 122 (no level found; the terraces reach 3 535 at 122 x 20): the redo at the 4 095 cap cannot be reached with the
               default heap, only through smb_lds_heap 256 and 1 024.  250 x 8 and 200 x 20 pass it, where smb_search plays agent 0 anyway.
  node indices at power 16 383 are bounded by 4 * 16 383 + 1 = 65 533; one pop in three is an expansion at best, and the most nodes a level
               of 200x20-p16383 makes is 19 549 (beyond 2^14 in 6 levels).
test_census_of_every_pool checks all that without a GPU and that the table below is the one it measures:
  9x4-p60        seed 201, 1500 draws, N  36: cap_cap=16 fell=6 flip_ends=7 flip_tells=27 gap=18 last_pop=6 nojump=10 q<=255=36 tail=8 win0=12 win1=8
  9x4-p300       seed 202, 1500 draws, N  13: cap_cap=1 fell=1 flip_tells=10 gap=6 nojump=1 q<=255=13 tail=6 win0=12
  16x6-p60       seed 203, 1500 draws, N  32: cap_cap=20 fell=7 flip_ends=4 flip_tells=21 gap=10 last_pop=7 nojump=6 q<=255=32 tail=16 win0=6 win1=6
  16x6-p300      seed 204, 6000 draws, N  37: cap_cap=6 fell=6 flip_ends=4 flip_tells=23 gap=24 last_pop=1 left_rim=6 nojump=6 q256..1023=6 q<=255=31 tail=7 win0=25 win1=6
  24x8-p200      seed 205, 1500 draws, N  42: cap_cap=15 fell=6 flip_ends=5 flip_tells=24 gap=21 last_pop=6 left_rim=6 nojump=6 out_out=9 q256..1023=15 q<=255=27 tail=15 win0=12 win1=6
  30x8-p10000    seed 206,  600 draws, N  24: fell=6 flip_ends=3 flip_tells=11 gap=7 nojump=8 out_out=16 q256..1023=12 q<=255=12 tail=9 win0=8
  7x3-p50        seed 207,   24 draws, N   6: none_needed=6 q<=255=6
  114x14-p10000  seed 208,  160 draws, N  20: cap_cap=6 fell=9 flip_tells=8 gap=7 nojump=3 out_out=7 q1024..2047=6 q2048..4095=10 q256..1023=1 q<=255=3 tail=10 win0=7
  122x32-p16382  seed 209,   80 draws, N  19: cap_cap=6 fell=7 flip_tells=4 gap=6 nojump=2 out_out=6 q1024..2047=5 q2048..4095=9 q256..1023=2 q<=255=3 tail=11 win0=7
  123x5-p2000    seed 210,  300 draws, N  24: cap_cap=6 fell=12 flip_ends=3 flip_tells=14 gap=12 nojump=3 out_out=6 q1024..2047=12 q256..1023=8 q<=255=4 tail=9 win0=6 win1=6
  250x8-p10000   seed 211,  200 draws, N  19: cap_cap=6 fell=7 flip_tells=9 gap=9 nojump=5 out_out=6 q1024..2047=1 q2048..4095=6 q256..1023=3 q<=255=3 q>4095=6 tail=5 win0=6 win1=1
  122x20-p16383  seed 212,   60 draws, N  12: fell=1 flip_tells=5 gap=5 nojump=3 out_out=6 q1024..2047=3 q2048..4095=3 q256..1023=2 q<=255=4 tail=4 win0=6
  200x20-p16383  seed 213,   60 draws, N  18: cap_cap=6 fell=6 flip_tells=7 gap=7 nojump=3 out_out=6 q2048..4095=4 q256..1023=4 q<=255=2 q>4095=8 tail=8 win0=6
  heap 114x14-p10000  smb_lds_heap 2048: fit=20 redone=0
  heap 114x14-p10000  smb_lds_heap 4096: fit=20 redone=0
  heap 122x32-p16382  smb_lds_heap 2048: fit=19 redone=0
  heap 122x32-p16382  smb_lds_heap 4096: fit=19 redone=0
  heap 30x8-p10000    smb_lds_heap  256: fit=12 redone=12
  heap 30x8-p10000    smb_lds_heap 1024: fit=24 redone=0
  heap 114x14-p10000  smb_lds_heap 1024: fit=4 redone=16
  every cell 9x4-p60    levels won=6 lost=6: flips=432 telling=229 silent=203; kept writes=966 telling=0
                        telling flips only in the read set by the term: above=0 left=0 stayed=8; silent flips in the read set=123, outside=80
  every cell 16x6-p300  levels won=6 lost=6: flips=1728 telling=793 silent=935; kept writes=2459 telling=0
                        telling flips only in the read set by the term: above=12 left=12 stayed=25; silent flips in the read set=372, outside=563
  every cell 24x8-p200  levels won=4 lost=4: flips=2688 telling=1014 silent=1674; kept writes=3310 telling=0
                        telling flips only in the read set by the term: above=13 left=15 stayed=29; silent flips in the read set=822, outside=852

The drivers.  _stats_routes: set_maps() -> env.stats and evaluate() -> stats of the whole pool against the oracle's rows.
parity_harness.smb_game_case: one handle of N wide environments, change_percentage 1.0, solver_power set as smb's is (prob._solver_power,
adjust_param()); set_maps() puts every environment one write away from its level (write_tape), four actions write the level's tile, the
other one, and both again; reward, done, every info column (iterations and changes too) of every step and the map against OracleEnv
(set_solver_power, seeded, reset(), set_map(), the four steps with auto-reset, or without: oracle_noreset), check_status() == 0.

Which test speaks for what:
  test_route_set_maps_and_evaluate   every pool: k_smb in MODE_SETMAP, both searches, the two agents' order, best node, jumps-dist
  test_route_steps / _rollout        one empty <-> solid flip per level (for every other level one that changes the play-through): k_update's
                                     changed list and `cheap`, k_smb in MODE_STEP, keep_play, the in-kernel reset after a flip that wins
  test_route_without_auto_reset      16x6-p60 on past done
  test_heap_splits                   smb_lds_heap 2 048 / 4 096 on the deep pools (arena slots / all in LDS), 256 and 1 024 on 30 x 8, 1 024 on
                                     114 x 14: levels that fit and levels that are redone in one batch (the `heap` lines of the table)
  test_every_cell_kind_flip          every cell of 12 / 18 / 14 levels to the other kind, set_maps() the level, then the new tile, the old, both
                                     again: a read set that misses a cell keeps a stale play-through on a telling flip.  The same with no_inc (every
                                     change played through): failing there too is a wrong search, failing only in the default a wrong keep
  test_every_cell_kind_kept          every free cell to enemy and coin, every blocking one to brick, tube, question: kept, the other statistics move
  test_tail_rule_takes_the_problems_width   the tail of jumps-dist after adjust_param(width=) without a reset()
The census also restates the read-set rule on the oracle's expanded states (read_set) and checks the rule itself: no telling flip lies
outside the set; and it counts the telling flips that only one term of the rule covers (`above`: wide >> 1, `left`: left & ~col, `stayed`:
left & col) -- the writes on the rim that the random steps of test_smb_kept_play_throughs_change_nothing may or may not hit.

Checked once against builds of the library with one value changed (not kept in the tree), this module and test_gpu_round5's smb test:
  smb_seen_accumulate without `wide >> 1`: fails test_route_steps / _rollout [16x6-p300, 24x8-p200, 122x20-p16383], test_every_cell_kind_flip
      [16x6-p300-keep, 24x8-p200-keep] (not no_inc: a wrong keep), test_every_cell_kind_kept [16x6-p300, 24x8-p200] (after the reset of a won
      level); passes 9x4-p60, whose census has above=0.  test_smb_kept_play_throughs_change_nothing fails too.
  smb_seen_accumulate without the `left & ~col` widening: NOT determined on the GPU -- the one run of that build did not come back from
      test_route_steps[9x4-p60] and was not repeated; no cause was found in the changed line.  By the census the rule less that term
      takes 12 + 15 telling flips of test_every_cell_kind_flip[16x6-p300-keep, 24x8-p200-keep] for harmless and none of 9x4-p60; before
      LEFT_RIM added its levels it was one flip in all.
  smb_seen_accumulate with `stayed` dropped: fails every stepping test of the module but 7x3, 122x32, 122x20, 200x20, and the round-5 test.
  `ground` in smb_child_win without `s.y >= -1`: passes everything, and no level can catch it: the term that follows reads the window's
      bit of row y + 1, rows above the screen carry no blocked bit, so it is false there with or without the test.
  the best-node tie `s.depth < best.depth` dropped in smb_search: fails test_every_cell_kind_flip[9x4-p60, 24x8-p200] with and without
      no_inc and test_every_cell_kind_kept[9x4-p60, 24x8-p200]; no pool level of the routes catches it.  The same tie in
      smb_search_two_label: passes everything, and cannot be caught -- with balance 1 pops come in non-decreasing exit distance + depth,
      so a later node at the same distance is never shallower.
  the tail rule with P.width for P.prob_width: fails test_tail_rule_takes_the_problems_width and nothing else.
With the library as it is every case passes: this module found no fault in kernels_smb.h or in the `cheap` rule.
"""
import collections
import functools

import numpy as np
import pytest

import oracle_lib as ol

EMPTY, SOLID, ENEMY, BRICK, QUESTION, COIN, TUBE = range(7)
BLOCKS = np.array([0, 1, 0, 1, 1, 0, 1], bool)            # " # ## #": solid, brick, question and tube block (engine.py)
DEFAULT_WEIGHTS = (0.75, 0.1, 0.01, 0.04, 0.01, 0.02, 0.02)
BLOCKED_WEIGHTS = (0.5, 0.4, 0.01, 0.02, 0.01, 0.01, 0.05)
OPEN_WEIGHTS = (0.97, 0.01, 0.004, 0.004, 0.004, 0.004, 0.004)


# ------------------------------------------------------------------ levels
def gen_random(rs, w, h, weights):
    return rs.choice(7, size=(h, w), p=np.array(weights) / np.sum(weights)).astype(np.uint8), np.zeros(w, bool)


def gen_terraces(rs, w, h):
    """Blocks strewn over a floor (one cell in 12, in 7 or in 4), which the player climbs: the levels with the most states, hence the
    longest searches and queues.  Where the map is wide enough its last h + 16 columns are one pit, too wide to cross from any height."""
    m = (rs.rand(h, w) < (0.08, 0.15, 0.25)[rs.randint(3)]).astype(np.uint8)
    m[max(h - 2, 1):, :] = SOLID
    pit = np.zeros(w, bool)
    if w >= h + 16 + 40 and rs.rand() < 0.75:
        m[:, w - (h + 16):] = EMPTY
        pit[w - (h + 16):] = True
    return m, pit


def gen_course(rs, w, h):
    """An obstacle course on a floor two rows deep: floor segments, pits, walls of 1 .. H-2 cells of solid / brick / tube, ceilings 2 .. 4
    rows above the floor, stairs; one course in three ends at a wall up to the top row.  A few enemies and coins in the free cells.
    -> the map and the columns of its pits."""
    m = np.zeros((h, w), np.uint8)
    pit = np.zeros(w, bool)
    f = max(h - 2, 1)                      # the floor's top row (the padding columns of the engine's grid are solid from there down)
    m[f:, :] = SOLID
    long_pits = rs.rand() < 0.3
    x = int(rs.randint(0, 3))
    while x < w:
        kind = rs.choice(5, p=[0.3, 0.25, 0.2, 0.15, 0.1])
        if kind == 0:
            x += int(rs.randint(1, 5))
        elif kind == 1:
            n = int(rs.randint(1, 13 if long_pits else 6))
            m[f:, x:x + n] = EMPTY
            pit[x:x + n] = True
            x += n + 1
        elif kind == 2 and f >= 1:
            ht, n = int(rs.randint(1, max(h - 2, 1) + 1)), int(rs.randint(1, 3))
            m[max(f - ht, 0):f, x:x + n] = (SOLID, BRICK, TUBE)[rs.randint(3)]
            x += n + int(rs.randint(0, 3))
        elif kind == 3:
            row, n = f - 1 - int(rs.randint(2, 5)), int(rs.randint(2, 8))
            if row >= 0:
                m[row, x:x + n] = (SOLID, BRICK, QUESTION)[rs.randint(3)]
            x += int(rs.randint(1, n + 1))
        else:
            n = int(rs.randint(2, min(5, max(h - 2, 2)) + 1))
            for i in range(n):
                if x + i < w:
                    m[max(f - 1 - i, 0):f, x + i] = SOLID
            x += n + int(rs.randint(0, 2))
    if rs.rand() < 0.33 and f >= 1:
        m[:f, w - int(rs.randint(1, min(4, w) + 1))] = SOLID
    free = m == EMPTY
    r = rs.rand(h, w)
    m[free & (r < 0.03)] = ENEMY
    m[free & (r > 0.97)] = COIN
    return m, pit


@functools.lru_cache(maxsize=None)
def _draws(w, h, seed, n, gens):
    """n levels from RandomState(seed), the generators `gens` in turn: 'default' / 'blocked' / 'open' random tiles, 'course', 'terraces'.
    -> maps [n, h, w], pits [n, w]."""
    rs = np.random.RandomState(seed)
    maps, pits = [], []
    for i in range(n):
        g = gens[i % len(gens)]
        m, pit = gen_course(rs, w, h) if g == "course" else gen_terraces(rs, w, h) if g == "terraces" else gen_random(rs, w, h, {"default": DEFAULT_WEIGHTS, "blocked": BLOCKED_WEIGHTS, "open": OPEN_WEIGHTS}[g])
        maps.append(m); pits.append(pit)
    return np.stack(maps), np.stack(pits)


def play(m, power):
    """The oracle's row, the pops of the two agents and the trace of the play-through (oracle_lib.get_stats)."""
    row, it, tr = ol.get_stats("smb", m, solver_power=power, with_iters=True, with_trace=True)
    return row, it.astype(np.int64)[:2].copy(), tr


# ------------------------------------------------------------------ classes, from the oracle's output alone
GAME = ("win0", "win1", "out_out", "cap_cap", "cap_out")
TIERS = ("q<=255", "q256..1023", "q1024..2047", "q2048..4095", "q>4095")


def tier(queue):
    """By the longest balance-1 queue, counted after an expansion's four pushes: smb_search_two_label gives up (status 2) exactly when
    that passes its cap -- 255 and 1 023 with smb_lds_heap 256 and 1 024, 4 095 from 2 048 on (the queue before the pushes: 4 091)."""
    return TIERS[(queue > 255) + (queue > 1023) + (queue > 2047) + (queue > 4095)]


def classify(m, pit, power, row, it, tr, row_less):
    """-> the names of the classes (module docstring) of level `m`; row_less: the oracle's row at power - 1."""
    h, w = m.shape
    t = {tier(tr["queue0"])}
    won = int(row[7]) == 0
    assert won == bool(tr["won"])
    if h == 3:
        assert won and tuple(it) == (1, 0)
        return t | {"none_needed"}
    assert (it[1] > 0) == (not (won and tr["pops1"] == 0)) and it[0] == tr["pops0"] and it[1] == tr["pops1"]
    if it[1] == 0:
        t.add("win0")
    else:
        end0 = "cap" if it[0] >= power else "out"
        if won:
            assert end0 == "cap"              # what agent 0 cannot reach in all its states, agent 1 cannot either
            t.add("win1")
        else:
            t.add("%s_%s" % (end0, "cap" if it[1] >= power else "out"))
    jumps, jumps_dist = int(row[5]), int(row[6])
    tail = w - tr["prev_jump_x"]
    assert jumps_dist == max(tr["max_gap"], tail)
    if jumps == 0:
        t.add("nojump")
    elif tr["max_gap"] > tail:
        t.add("gap")
    else:
        t.add("tail")
    if (row != row_less).any():
        t.add("last_pop")
    c = tr["x"] - 3                          # the best node's map column
    if not won and ((0 <= c < w and pit[c]) or (0 <= c + 1 < w and pit[c + 1])):
        t.add("fell")
    return t


# name -> (width, height, solver_power, kind, seed, draws, generators, {class: least count})
POOLS = {}
RANDOM_AND_COURSE = ("default", "course", "blocked", "course")
FOUR = lambda *names: {k: 4 for k in names}          # noqa: E731


def _add(name, *spec):
    POOLS[name] = spec


# The minima: 4 of every class the pool's size and power allow (module docstring: what they do not allow, and why)
_add("9x4-p60", 9, 4, 60, "stepped", 201, 1500, RANDOM_AND_COURSE, FOUR("win0", "win1", "cap_cap", "nojump", "tail", "gap", "last_pop", "fell"))
_add("9x4-p300", 9, 4, 300, "stepped", 202, 1500, RANDOM_AND_COURSE, FOUR("win0", "tail", "gap"))
_add("16x6-p60", 16, 6, 60, "stepped", 203, 1500, RANDOM_AND_COURSE, FOUR("win0", "win1", "cap_cap", "nojump", "tail", "gap", "last_pop", "fell"))
_add("16x6-p300", 16, 6, 300, "stepped", 204, 6000, RANDOM_AND_COURSE, FOUR("win0", "win1", "cap_cap", "nojump", "tail", "gap", "fell", "q256..1023"))
_add("24x8-p200", 24, 8, 200, "stepped", 205, 1500, RANDOM_AND_COURSE, FOUR("win0", "win1", "cap_cap", "out_out", "nojump", "tail", "gap", "last_pop", "fell", "q256..1023"))
_add("30x8-p10000", 30, 8, 10000, "stepped", 206, 600, RANDOM_AND_COURSE, FOUR("win0", "out_out", "nojump", "tail", "gap", "fell", "q<=255", "q256..1023"))
_add("7x3-p50", 7, 3, 50, "stepped", 207, 24, RANDOM_AND_COURSE, FOUR("none_needed"))
_add("114x14-p10000", 114, 14, 10000, "deep", 208, 160, ("default", "terraces", "course", "open"), {"q2048..4095": 8, "win0": 4, "out_out": 4})
_add("122x32-p16382", 122, 32, 16382, "deep", 209, 80, ("terraces", "default", "course", "open"), {"q2048..4095": 8, "win0": 4, "out_out": 4})
_add("123x5-p2000", 123, 5, 2000, "wide", 210, 300, RANDOM_AND_COURSE, FOUR("win0", "win1", "cap_cap", "out_out"))
_add("250x8-p10000", 250, 8, 10000, "wide", 211, 200, ("open", "terraces", "course", "default"), {"q>4095": 4, "win0": 4, "out_out": 4, "cap_cap": 4})
_add("122x20-p16383", 122, 20, 16383, "top", 212, 60, ("terraces", "open", "course", "default"), {"win0": 4, "out_out": 4})
_add("200x20-p16383", 200, 20, 16383, "top", 213, 60, ("terraces", "open", "course", "terraces"), {"win0": 4, "cap_cap": 4})

# Draws taken whatever the quotas say (class left_rim): levels with two or three telling flips that only the `left & ~col` term of
# the read set covers -- one draw in 16 has one, the levels the quotas pick happen to have two between them.  Found by sweeping
# every draw of the two pools with every_cell's own arithmetic; the census counts what they give.
LEFT_RIM = {"16x6-p300": (124, 447, 510, 924, 1440, 1576), "24x8-p200": (56, 164, 228, 1092, 1313, 1403)}
QUOTA = 6              # levels taken per class
MAX_LEVELS = {"stepped": 400, "deep": 24, "wide": 48, "top": 24}
SEED0 = 7000


@functools.lru_cache(maxsize=None)
def pool(name):
    """-> dict(w, h, power, maps [N, h, w], pits, rows, its, traces, tags, cell [N, 2] (x, y of the cell the driver flips), census)."""
    w, h, power, kind, seed, ndraw, gens, need = POOLS[name]
    maps, pits = _draws(w, h, seed, ndraw, gens)
    have = collections.Counter()
    picked = []
    for i in range(ndraw):
        if not (maps[i] <= SOLID).any():
            continue                          # the driver needs a cell to flip between empty and solid
        row, it, tr = play(maps[i], power)
        tg = classify(maps[i], pits[i], power, row, it, tr, play(maps[i], power - 1)[0])
        quota = {k: max(QUOTA, need.get(k, 0)) for k in tg}
        if kind in ("deep", "wide", "top"):       # few levels: only what the pool is there for, and the game classes
            quota = {k: v for k, v in quota.items() if k in need or k in GAME}
        if i in LEFT_RIM.get(name, ()):
            tg.add("left_rim")
        if "left_rim" in tg or (any(have[k] < v for k, v in quota.items()) and len(picked) < MAX_LEVELS[kind]):
            picked.append((i, row, it, tr, tg))
            have.update(tg)
    sel = [p[0] for p in picked]
    out_maps = maps[sel]
    # the cell the driver flips between empty and solid: for every other level one whose flip changes the play-through, where one of
    # eight tries finds it
    rs = np.random.RandomState(seed + 7)
    cell, tells = [], []
    for k, (i, row, _it, _tr, _tg) in enumerate(picked):
        ys, xs = np.nonzero(maps[i] <= SOLID)
        for _try in range(8 if k % 2 == 0 else 1):
            j = rs.randint(len(ys))
            nb = maps[i].copy()
            nb[ys[j], xs[j]] ^= 1
            other = play(nb, power)[0]
            if (other[5:8] != row[5:8]).any():
                break
        cell.append((xs[j], ys[j]))
        tells.append(("flip_tells",) * bool((other[5:8] != row[5:8]).any()) + ("flip_ends",) * bool(row[7] != 0 and other[7] == 0))
    census = collections.Counter()
    for p, tl in zip(picked, tells):
        census.update(p[4]); census.update(tl)
    return dict(name=name, w=w, h=h, power=power, kind=kind, maps=out_maps, pits=pits[sel], rows=np.stack([p[1] for p in picked]),
                its=np.stack([p[2] for p in picked]), traces=[p[3] for p in picked], tags=[p[4] for p in picked],
                cell=np.array(cell, np.int32), census=dict(census))


def census_shortfall(name):
    p = pool(name)
    need = POOLS[name][7]
    return {k: (p["census"].get(k, 0), v) for k, v in need.items() if p["census"].get(k, 0) < v}


def census_table():
    lines = []
    for name in POOLS:
        p = pool(name)
        lines.append("  %-14s seed %d, %4d draws, N %3d: %s" % (name, POOLS[name][4], POOLS[name][5], len(p["maps"]),
                                                               " ".join("%s=%d" % kv for kv in sorted(p["census"].items()))))
    return "\n".join(lines)


STEPPED = [n for n, s in POOLS.items() if s[3] == "stepped"]
DEEP = [n for n, s in POOLS.items() if s[3] == "deep"]
WIDE = [n for n, s in POOLS.items() if s[3] == "wide"]
TOP = [n for n, s in POOLS.items() if s[3] == "top"]
HEAP_SPLITS = [(n, hp) for n in DEEP for hp in (2048, 4096)] + [("30x8-p10000", 256), ("30x8-p10000", 1024), ("114x14-p10000", 1024)]


def heap_census(name, lds_heap):
    """How many levels of the pool smb_search_two_label finishes with `lds_heap` heap words in LDS, and how many outgrow its cap and
    are searched again by smb_search -> (fit, redone)."""
    cap = 4095 if lds_heap >= 2048 else lds_heap - 1
    q = np.array([tr["queue0"] for tr in pool(name)["traces"]])
    return int((q <= cap).sum()), int((q > cap).sum())


# ------------------------------------------------------------------ every one-cell change
EVERY_CELL = {"9x4-p60": 12, "16x6-p300": 12, "24x8-p200": 8}          # pool -> levels taken (the first ones: a few of every class)
KEPT_TILES = {False: (ENEMY, COIN), True: (BRICK, TUBE, QUESTION)}          # the writes that keep a free / a blocking cell's kind


RIMS = ("above", "left", "stayed")


def read_set(m, expanded, without=None):
    """The cells of level `m` its play-through read, by the rule of kernels_smb.h (smb_seen_accumulate) from the oracle's expanded
    states (oracle_lib.get_stats, trace["expanded"]) -> bool [h, w].  An expansion at (x, y) reads column x in the rows y - 1 .. y + 1,
    of column x + 1 the row y and -- where that cell is free -- the rows y - 1 and y + 1.  without: the rule less one term --
    'above' the row y - 1 (`wide >> 1`), 'left' the rows y - 1 and y + 1 of column x + 1 (`left & ~col`), 'stayed' the row y of a
    blocked cell of column x + 1 (`left & col`)."""
    h, w = m.shape

    def blocked(x, y):                     # the engine's grid: free above the screen, blocked below it, three padding columns either side
        if y < 0 or y >= h:
            return y >= h
        if 3 <= x < w + 3:
            return bool(BLOCKS[m[y, x - 3]])
        return y > h - 3 or (y == h - 3 and x == w + 4)

    seen = np.zeros((h, w), bool)
    for c in range(w):
        x = c + 3
        own = [y for y in range(-8, h) if (int(expanded[x]) >> (y + 8)) & 1]
        left = [y for y in range(-8, h) if (int(expanded[x - 1]) >> (y + 8)) & 1]
        wide = set(own) | (set() if without == "left" else {y for y in left if not blocked(x, y)})
        rows = wide | {y + 1 for y in wide} | (set() if without == "above" else {y - 1 for y in wide})
        rows |= set() if without == "stayed" else {y for y in left if blocked(x, y)}
        for y in rows:
            if 0 <= y < h:
                seen[y, c] = True
    return seen


@functools.lru_cache(maxsize=None)
def every_cell(name, family):
    """One case per (level, cell, new tile) -> dict(maps [M, h, w] the levels, cells [M, 2], tiles [M] the new tile, level [M], tells [M]:
    jumps / jumps-dist / dist-win of the level with the new tile are not the level's).  family 'flip': every cell to empty if it
    blocks, to solid if it does not; 'kept': every free cell to enemy and to coin, every blocking one to brick, tube and question."""
    p = pool(name)
    n = EVERY_CELL[name]
    # lost levels and won ones: the first n / 2 of either
    won = [i for i in range(len(p["maps"])) if p["rows"][i][7] == 0][:n // 2]
    lost = [i for i in range(len(p["maps"])) if p["rows"][i][7] != 0][:n - len(won)]
    rim = [i for i in range(len(p["maps"])) if "left_rim" in p["tags"][i] and i not in won + lost] if family == "flip" else []
    maps, cells, tiles, level, tells, read = [], [], [], [], [], {k: [] for k in (None,) + RIMS}
    for i in sorted(won + lost + rim):
        m = p["maps"][i]
        seen = {k: read_set(m, p["traces"][i]["expanded"], k) for k in read}
        for y in range(p["h"]):
            for x in range(p["w"]):
                b = bool(BLOCKS[m[y, x]])
                for t in ((EMPTY if b else SOLID,) if family == "flip" else KEPT_TILES[b]):
                    if t == m[y, x]:
                        continue
                    nb = m.copy()
                    nb[y, x] = t
                    maps.append(m); cells.append((x, y)); tiles.append(t); level.append(i)
                    tells.append(bool((play(nb, p["power"])[0][5:8] != p["rows"][i][5:8]).any()))
                    for k in read:
                        read[k].append(seen[k][y, x])
    tells = np.array(tells)
    # read: the cell is in the level's read set; rim[k]: a telling write that only term k of the rule puts there
    return dict(maps=np.stack(maps), cells=np.array(cells, np.int32), tiles=np.array(tiles, np.uint8), level=np.array(level), tells=tells,
                read=np.array(read[None]), rim={k: tells & ~np.array(read[k]) for k in RIMS}, nwon=len(won), nlost=len(lost))


def test_census_of_every_pool():
    """No GPU: every pool holds what its cases need, by the oracle alone -- the minima of POOLS, at least 100 telling and 100 silent
    kind flips per swept pool, no kind-preserving write that tells -- so that a change to a generator, a seed or a power cannot quietly
    empty a class.  Prints the table of the module docstring."""
    table = census_table()
    lines = [table]
    short = {name: census_shortfall(name) for name in POOLS}
    short = {k: v for k, v in short.items() if v}
    for name, hp in HEAP_SPLITS:
        lines.append("  heap %-14s smb_lds_heap %4d: fit=%d redone=%d" % ((name, hp) + heap_census(name, hp)))
    for name in EVERY_CELL:
        f, k = every_cell(name, "flip"), every_cell(name, "kept")
        lines.append("  every cell %-10s levels won=%d lost=%d: flips=%d telling=%d silent=%d; kept writes=%d telling=%d"
                     % (name, f["nwon"], f["nlost"], len(f["tells"]), f["tells"].sum(), (~f["tells"]).sum(), len(k["tells"]), k["tells"].sum()))
        lines.append("             %-10s telling flips only in the read set by the term: %s; silent flips in the read set=%d, outside=%d"
                     % ("", " ".join("%s=%d" % (r, f["rim"][r].sum()) for r in RIMS), (~f["tells"] & f["read"]).sum(), (~f["tells"] & ~f["read"]).sum()))
        assert not (f["tells"] & ~f["read"]).any(), lines[-2:]          # the rule itself: no write outside the read set tells
        assert f["tells"].sum() >= 100 and (~f["tells"]).sum() >= 100, lines[-2]
        # the rim of the read set: telling flips that a rule less one term would take for harmless (where LEFT_RIM adds levels for it)
        assert name not in LEFT_RIM or all(f["rim"][r].sum() >= 8 for r in RIMS), lines[-1]
        assert f["nwon"] >= 2 and f["nlost"] >= 2, lines[-2]
        assert not k["tells"].any(), lines[-1]           # the play-through reads a cell only as blocked / free
    print("\n".join(lines))
    stale = [ln for ln in lines for ln in ln.split("\n") if ln.rstrip() not in __doc__]
    assert not stale, "the module docstring's table is not the one measured; these lines differ:\n" + "\n".join(stale)
    assert not short, "classes with too few levels {pool: {class: (count, least)}}: %s\n%s" % (short, table)
    for name, (w, h, power, kind, _seed, _n, _g, _need) in POOLS.items():
        p = pool(name)
        assert 4 <= len(p["maps"]) <= MAX_LEVELS[kind], (name, len(p["maps"]))
        # which search plays agent 0 (kernels_smb.h, smb_job: two_label = width + 6 <= 128 && solver_power < 16383)
        assert (w + 6 <= 128 and power < 16383) == (kind in ("stepped", "deep")), name
    # the redo of a search that outgrows its heap: both kinds of level in one batch
    for name, hp in (("30x8-p10000", 256), ("114x14-p10000", 1024), ("114x14-p10000", 2048), ("122x32-p16382", 2048)):
        fit, redone = heap_census(name, hp)
        assert fit >= 4 and (redone >= 4 or hp >= 2048), (name, hp, fit, redone)
    # power 16 383: node indices of smb_search (16 bits of a heap word) are bounded by 4 * 16 383 + 1 = 65 533; a pop in three is an
    # expansion at best (the rest: states seen before), so what levels reach is a third of that -- at least four go beyond 2^14
    nodes = [4 * max(tr["expansions0"], tr["expansions1"]) + 1 for tr in pool("200x20-p16383")["traces"]]
    print("  200x20-p16383: most nodes of a search %d, beyond 16 384 in %d levels" % (max(nodes), sum(n > 16384 for n in nodes)))
    assert sum(n > 16384 for n in nodes) >= 4


def test_oracle_steps_smb_at_the_power_set():
    """No GPU: OracleEnv.set_solver_power is what the stepped oracle plays with (adjust_param leaves smb's alone, as the reference
    does), and the trace agrees with the row: the statistics a step reports are get_stats of the stepped map at that power."""
    p = pool("16x6-p60")
    differ = 0
    for i in range(len(p["maps"])):
        m = p["maps"][i]
        o = ol.OracleEnv("smb", "wide")
        o.adjust_param(width=p["w"], height=p["h"])
        o.adjust_param(change_percentage=1.0, solver_power=7)          # (ignored: smb_prob.py:40-53)
        o.set_solver_power(p["power"])
        o.seed(SEED0 + i)
        o.reset()
        nb = m.copy()
        x, y = p["cell"][i]
        nb[y, x] ^= 1
        o.set_map(nb)
        _obs, _rew, _done, info = o.step([x, y, m[y, x]])
        got = np.array([info[k] for k in ol.INFO_KEYS["smb"]])
        assert np.array_equal(got, p["rows"][i]), (i, got, p["rows"][i])
        differ += bool((ol.get_stats("smb", m, solver_power=10000) != p["rows"][i]).any())
        tr = p["traces"][i]
        assert tr["expansions0"] <= tr["pops0"] <= p["power"] and tr["queue0"] <= 3 * tr["expansions0"] + 1
    assert differ >= 8          # the default power gives other rows: the setter is what made them equal


# ------------------------------------------------------------------ the routes, on the GPU
def _torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _labels(p):
    return ["pops %d/%d queue %d %s" % (it[0], it[1], tr["queue0"], ",".join(sorted(t))) for it, tr, t in zip(p["its"], p["traces"], p["tags"])]


def _env(p, n, tuning=None):
    from gym_pcgrl_amd.envs import BatchedPcgrlEnv
    env = BatchedPcgrlEnv(prob="smb", rep="wide", num_envs=n, seed=1000, tuning=tuning)
    env.adjust_param(width=p["w"], height=p["h"])
    env.adjust_param(change_percentage=1.0)
    env._prob._solver_power = p["power"]          # smb_prob.py:40-53: an attribute, not an adjust_param key
    env.adjust_param()
    return env


def _stats_routes(name, tuning=None):
    """set_maps() -> env.stats and evaluate() -> stats against the oracle's rows of the whole pool."""
    _torch()
    p = pool(name)
    lab = _labels(p)
    env = _env(p, len(p["maps"]), tuning)
    try:
        env.reset()
        env.set_maps(p["maps"])
        for what, got in (("set_maps", env.stats), ("evaluate", env.evaluate(p["maps"][::-1].copy()).stats.flip(0))):
            got = got.cpu().numpy().astype(np.int64)
            bad = np.nonzero((got != p["rows"]).any(1))[0]
            assert bad.size == 0, (what, name, tuning, [(int(i), lab[i], got[i].tolist(), p["rows"][i].tolist()) for i in bad[:6]])
        assert env.check_status() == 0
        assert np.array_equal(env._bufs["map"].cpu().numpy(), p["maps"])
    finally:
        env.close()


@functools.lru_cache(maxsize=None)
def _expected(name, auto_reset=True):
    """The oracle's four steps of the pool's one flip per level: computed once for the routes that share it."""
    import parity_harness as ph
    p = pool(name)
    x, y = p["cell"][:, 0], p["cell"][:, 1]
    return ph.smb_game_expected(p["w"], p["h"], p["power"], p["maps"], p["cell"], 1 - p["maps"][np.arange(len(x)), y, x], SEED0, auto_reset)


def _route(name, route, tuning=None, auto_reset=True):
    _torch()
    import parity_harness as ph
    p = pool(name)
    E = _expected(name, auto_reset)
    return ph.smb_game_case(p["w"], p["h"], p["power"], p["maps"], p["cell"], E["start"][np.arange(len(p["maps"])), p["cell"][:, 1], p["cell"][:, 0]],
                            route, tuning=tuning, auto_reset=auto_reset, seed0=SEED0, labels=_labels(p), expected=E)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(POOLS))
def test_route_set_maps_and_evaluate(name):
    """The statistics of the whole pool from set_maps() (k_smb, MODE_SETMAP) and from evaluate() against ol.get_stats."""
    _stats_routes(name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", STEPPED + DEEP + WIDE + TOP)
def test_route_steps(name):
    """step() four times: k_update's changed list, k_smb in MODE_STEP, the in-kernel reset and MODE_START play-through of the
    environments whose flip makes the level winnable (flip_ends in the census)."""
    _route(name, "step")


@pytest.mark.gpu
@pytest.mark.parametrize("name", STEPPED + DEEP + WIDE + TOP)
def test_route_rollout(name):
    """The four actions as one rollout()."""
    _route(name, "rollout")


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["step", "rollout"])
def test_route_without_auto_reset(route):
    """One stepped pool without auto-reset: the episode goes on past a won level (parity_harness.oracle_noreset)."""
    _route("16x6-p60", route, auto_reset=False)


@pytest.mark.gpu
@pytest.mark.parametrize("name,lds_heap", HEAP_SPLITS, ids=["%s-heap%d" % s for s in HEAP_SPLITS])
def test_heap_splits(name, lds_heap):
    """smb_lds_heap: the deep pools with 2 048 heap words in LDS (the deepest level of the two-label heap in the arena) and with all
    4 096 in LDS; the 30 x 8 pool at 256 -- the levels whose queue stays within 255 and those that outgrow it (status 2) and are
    searched again by smb_search in one batch (heap_census: 12 and 12) -- and at 1 024.  Statistics, then the four steps."""
    tuning = {"smb_lds_heap": lds_heap}
    _stats_routes(name, tuning)
    _route(name, "step", tuning)


# ------------------------------------------------------------------ every one-cell change, on the GPU
BATCH = 1536


def _every_cell(name, family, tuning=None):
    """set_maps() puts the level, the tape writes the new tile, the old one, and both again (write_tape with the roles swapped: the
    `maps` handed over hold the new tile, the `tiles` the level's own)."""
    _torch()
    import parity_harness as ph
    p = pool(name)
    c = every_cell(name, family)
    n = len(c["tiles"])
    x, y = c["cells"][:, 0], c["cells"][:, 1]
    old = c["maps"][np.arange(n), y, x]
    nb = c["maps"].copy()
    nb[np.arange(n), y, x] = c["tiles"]
    lab = ["level %d %s%s" % (lv, ",".join(sorted(p["tags"][lv])), " telling" if tl else "") for lv, tl in zip(c["level"], c["tells"])]
    for a in range(0, n, BATCH):
        s = slice(a, min(n, a + BATCH))
        ph.smb_game_case(p["w"], p["h"], p["power"], nb[s], c["cells"][s], old[s], "step", tuning=tuning, seed0=SEED0 + a, labels=lab[s])


@pytest.mark.gpu
@pytest.mark.parametrize("tuning", [None, {"no_inc": 1}], ids=["keep", "no_inc"])
@pytest.mark.parametrize("name", list(EVERY_CELL))
def test_every_cell_kind_flip(name, tuning):
    """Every cell of the swept levels to empty if it blocks, to solid if it does not: k_update keeps the play-through of a write to a
    cell no search read (`cheap`), so a read set (smb_seen_accumulate) that misses a cell shows as a stale jumps / jumps-dist /
    dist-win on one of the telling flips.  With no_inc every change is played through: a failure there is a wrong search, one only
    in the default a wrong keep."""
    _every_cell(name, "flip", tuning)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(EVERY_CELL))
def test_every_cell_kind_kept(name):
    """Every free cell to enemy and to coin, every blocking one to brick, tube and question: the play-through is kept (the census: no
    such write tells) while dist-floor, enemies, noise and disjoint-tubes move."""
    _every_cell(name, "kept")


@pytest.mark.gpu
def test_tail_rule_takes_the_problems_width():
    """jumps-dist's tail is `self._width - last jump column` (smb_prob.py:166): the problem's width, which after adjust_param(width=)
    without a reset() is not the maps'.  The tail and gap levels of a stepped pool, the width raised by 9 under them, the four steps
    without auto-reset (a reset would make maps of the new size)."""
    _torch()
    import torch
    import parity_harness as ph
    from gym_pcgrl_amd.envs import BatchedPcgrlEnv
    p = pool("16x6-p60")
    sel = [i for i, t in enumerate(p["tags"]) if t & {"tail", "gap"}]
    assert sum("tail" in p["tags"][i] for i in sel) >= 4
    maps, cell = p["maps"][sel], p["cell"][sel]
    n = len(sel)
    start, acts = ph.write_tape(maps, cell, 1 - maps[np.arange(n), cell[:, 1], cell[:, 0]])
    wider = p["w"] + 9
    exp = []
    for i in range(n):
        o = ol.OracleEnv("smb", "wide")
        o.adjust_param(width=p["w"], height=p["h"])
        o.adjust_param(change_percentage=1.0)
        o.set_solver_power(p["power"])
        o.seed(SEED0 + i)
        o.reset()
        o.adjust_param(width=wider)
        o.set_map(start[i])
        exp.append(ph.oracle_noreset(o, acts[:, i]))
    assert any(x["info"][0][6] == wider - (p["w"] - r[6]) for x, r in zip(exp, p["rows"][sel]))      # a tail measured from the new width
    env = BatchedPcgrlEnv(prob="smb", rep="wide", num_envs=n, seed=SEED0, auto_reset=False)
    try:
        env.adjust_param(width=p["w"], height=p["h"])
        env.adjust_param(change_percentage=1.0)
        env._prob._solver_power = p["power"]
        env.adjust_param()
        env.reset()
        env.adjust_param(width=wider)
        env.set_maps(start)
        keys = list(env._prob.info_keys) + ["iterations", "changes"]
        for t in range(4):
            _obs, rew, done, info = env.step(acts[t])
            got = np.stack([info[k].cpu().numpy() for k in keys], 1).astype(np.int64)
            want = np.stack([x["info"][t] for x in exp])
            bad = np.nonzero((got != want).any(1))[0]
            assert bad.size == 0, (t, bad.tolist(), got[bad[0]].tolist(), want[bad[0]].tolist())
            assert np.array_equal(rew.cpu().numpy(), np.array([x["reward"][t] for x in exp])), t
            assert np.array_equal(done.cpu().numpy(), np.array([x["done"][t] for x in exp])), t
        assert env.check_status() == 0
        del torch
    finally:
        env.close()
