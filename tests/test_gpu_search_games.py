"""Every decision of a search problem's _run_game (csrc/search_game.h, SearchGame<PROB>) on every kernel family that plays it --
k_sokoban, k_mdungeon / k_ddave, k_step_solver, k_search_async, k_search_big -- against the CPU oracle, on levels chosen by what the
oracle says their game does.  All comparisons are exact: integers and float64 rewards.

Levels.  Per (problem, size, solver_power) a pool is mined from fixed RandomState seeds (POOLS: seed and number of draws per pool;
gen_level: player, exit / targets / key, a few things, some solid cells; one draw in four a small room in a solid map, mdungeon
also maps crowded with enemies) and classified from the oracle's tape alone -- get_stats(with_iters=True): the pops of the four
agents, 0 = did not run, and the problem's dist-win / sol-length columns (WIN_COLS) for the win:
  none        no search ran (the solver's precondition is unmet)
  a0          agent 0 won below the cap, nobody else ran
  all_cap     all four agents ran into the cap          all_nocap   all four ran, none into the cap
  win1..3     sokoban: agent 1 / 2 / 3 won after every earlier agent hit the cap      bfs_out   BFS ran out of states without a win
  tape01..    mdungeon: agents {0,1}, {0,1,2}, {0,1,2,3} ran, the earlier ones into the cap   astar_out   an A* agent ran out of states
  mid         ddave: the game ended at agent 1 or 2      won_after_out   ddave: an agent won after an earlier one ran out of states
  cap / below some agent / no agent hit the cap          near256 / beyond256   the longest agent took 250..262 / more than 256 pops
  last_pop    (tier pools) the oracle's row at solver_power - 1 is another one: the last pop before the cap decides
  heavy       8..12 crates / more than 48 things / more than 48 diamonds: the compact searches refuse it (heavy_ran: its search ran)
minima() says how many of each a pool must hold (4 of each class a stepped pool needs, 2 of ddave's mid, 8 heavy of which 4 ran, 64
beyond256 in the first block of the power-1000 pools); test_census_of_every_pool checks that without a GPU.  Measured:
  ddave-11x7     seed 101, 12000 draws, N  71: a0=6 all_cap=6 all_nocap=7 below=17 beyond256=42 cap=39 heavy=9 heavy_ran=8 mid=10 none=6 won_after_out=6
  ddave-15x15    seed 102,  4000 draws, N  53: a0=6 all_cap=6 all_nocap=6 below=16 beyond256=23 cap=23 heavy=8 heavy_ran=8 mid=6 none=6 won_after_out=4
  ddave-p1000    seed 104,  6000 draws, N 115: a0=5 all_cap=5 all_nocap=59 below=69 beyond256=91 cap=34 heavy=8 heavy_ran=8 mid=9 near256=6 none=4 won_after_out=7
  ddave-p255     seed 103,  6000 draws, N  69: a0=4 all_cap=18 all_nocap=4 below=12 cap=45 heavy=8 heavy_ran=8 last_pop=12 mid=8 near256=1 none=4 won_after_out=4
  ddave-p256     seed 103,  6000 draws, N  69: a0=4 all_cap=17 all_nocap=4 below=12 cap=45 heavy=8 heavy_ran=8 last_pop=12 mid=8 near256=1 none=4 won_after_out=4
  ddave-p257     seed 103,  6000 draws, N  65: a0=4 all_cap=14 all_nocap=4 below=12 beyond256=41 cap=41 heavy=8 heavy_ran=8 last_pop=8 mid=8 near256=1 none=4 won_after_out=4
  ddave-p5001    seed 105,  3000 draws, N  29: a0=9 all_cap=5 all_nocap=5 below=18 beyond256=9 cap=5 heavy=8 heavy_ran=8 mid=4 none=6 won_after_out=5
  mdungeon-15x15 seed 102,  6000 draws, N  45: a0=6 all_cap=6 all_nocap=6 astar_out=6 below=12 beyond256=19 cap=19 heavy=8 heavy_ran=8 none=6 tape01=6 tape012=6 tape0123=7
  mdungeon-7x11  seed 101,  6000 draws, N  48: a0=6 all_cap=6 all_nocap=6 astar_out=6 below=12 beyond256=20 cap=20 heavy=10 heavy_ran=8 none=6 tape01=6 tape012=6 tape0123=8
  mdungeon-p1000 seed 104,  6000 draws, N  90: a0=40 all_cap=18 all_nocap=5 astar_out=5 below=45 beyond256=65 cap=33 heavy=8 heavy_ran=8 near256=6 none=4 tape01=9 tape012=5 tape0123=19
  mdungeon-p255  seed 103,  6000 draws, N  37: a0=6 all_cap=4 all_nocap=4 astar_out=4 below=10 cap=15 heavy=8 heavy_ran=8 last_pop=2 near256=1 none=4 tape01=4 tape012=5 tape0123=6
  mdungeon-p256  seed 103,  6000 draws, N  36: a0=6 all_cap=4 all_nocap=4 astar_out=4 below=10 cap=14 heavy=8 heavy_ran=8 last_pop=1 near256=1 none=4 tape01=4 tape012=4 tape0123=6
  mdungeon-p257  seed 103,  6000 draws, N  36: a0=5 all_cap=5 all_nocap=4 astar_out=4 below=9 beyond256=15 cap=15 heavy=8 heavy_ran=8 last_pop=1 none=4 tape01=4 tape012=4 tape0123=7
  mdungeon-p5001 seed 105,  3000 draws, N  34: a0=14 all_cap=4 all_nocap=4 astar_out=4 below=18 beyond256=14 cap=10 heavy=8 heavy_ran=8 none=6 tape01=3 tape012=3 tape0123=4
  sokoban-15x15  seed 102,  4000 draws, N  54: a0=6 all_cap=6 all_nocap=6 below=12 beyond256=24 bfs_out=6 cap=24 heavy=12 heavy_ran=8 none=6 win1=6 win2=6 win3=6
  sokoban-5x5    seed 101,  6000 draws, N  51: a0=6 all_cap=6 all_nocap=6 below=12 beyond256=24 bfs_out=6 cap=24 heavy=9 heavy_ran=8 none=6 win1=6 win2=6 win3=6
  sokoban-6x6    seed 101,  4000 draws, N  52: a0=6 all_cap=6 all_nocap=6 below=12 beyond256=24 bfs_out=6 cap=24 heavy=10 heavy_ran=8 none=6 win1=6 win2=6 win3=6
  sokoban-6x7    seed 101,  4000 draws, N  53: a0=6 all_cap=6 all_nocap=6 below=12 beyond256=24 bfs_out=6 cap=24 heavy=11 heavy_ran=8 none=6 win1=6 win2=6 win3=6
  sokoban-p1000  seed 104,  6000 draws, N  92: a0=28 all_cap=18 all_nocap=9 below=37 beyond256=66 bfs_out=9 cap=41 heavy=10 heavy_ran=8 near256=6 none=4 win1=6 win2=11 win3=6
  sokoban-p255   seed 103,  6000 draws, N  45: a0=4 all_cap=7 all_nocap=6 below=10 bfs_out=6 cap=19 heavy=12 heavy_ran=8 last_pop=3 none=4 win1=4 win2=4 win3=4
  sokoban-p256   seed 103,  6000 draws, N  46: a0=4 all_cap=7 all_nocap=6 below=10 bfs_out=6 cap=20 heavy=12 heavy_ran=8 last_pop=5 none=4 win1=4 win2=4 win3=5
  sokoban-p257   seed 103,  6000 draws, N  44: a0=4 all_cap=4 all_nocap=6 below=10 beyond256=18 bfs_out=6 cap=18 heavy=12 heavy_ran=8 last_pop=2 none=4 win1=4 win2=4 win3=6
  sokoban-p5001  seed 105,  3000 draws, N  44: a0=6 all_cap=5 all_nocap=12 below=18 beyond256=21 bfs_out=12 cap=17 heavy=11 heavy_ran=8 near256=1 none=9 win1=4 win2=4 win3=4
(the heavy levels are counted under heavy only, except in the p5001 pools, where every level takes the generic search).  The powers:
300 for every full pool -- at 16 or 50 no mdungeon or ddave level has all four agents run out of states, at 1000 and more nearly
every mdungeon level ends at agent 0.

The driver (parity_harness.search_game_case): one handle of N wide environments, change_percentage 1.0; set_maps() puts every
environment one write away from its level (one empty or solid cell flipped), four actions write the cell back, flip it, and both again,
so that the level is what steps 1 and 3 compute and its neighbour steps 2 and 4; reward, done, every info column (iterations and
changes too) of every step and the map against OracleEnv (seeded seed0 + i, reset(), set_map(), auto-reset), check_status() == 0.

Which test speaks for which rule of search_game.h:
  SearchGame::next (the agent order, first winner, sokoban's exhausted BFS, mdungeon's exhausted A* -> BFS, ddave's "exhaustion says
      nothing") in the sequential loop: test_route_c_rollout, test_small_tier_of_the_rollout (search_game_run in k_step_solver) and
      test_route_d_async_ticks (k_search_async, suspended inside and between agents at 4 pops a tick) -- classes win1..3, bfs_out,
      tape01.., astar_out, mid, won_after_out, all_cap, all_nocap.
  stop_update / stopped (the stop word polled every 32 pops) and the selection of the record, encode / decode of word 3: the concurrent
      kernels -- test_route_a_set_maps (MODE_SETMAP) and test_route_b_steps (MODE_STEP) -- classes win1..3 and tape01.. (a later agent wins
      while the earlier ones run to the cap), bfs_out / astar_out (MD_STOP_EXHAUSTED), mid / won_after_out (ddave).
  the parked row (finish_search_item: B.info in MODE_STEP, B.stats otherwise): route B against route A; routes C and D park in B.info too.
  the compact-or-generic choice (build, S.fast): the heavy levels in the same batch as the others on every route;
      test_route_e_generic_search_in_lds (sok_generic = 1) and test_route_e_global_arena (solver_power 5001) for agent_generic alone;
      sokoban-6x6 / -6x7 for sok_search_fast<1> / <4> (S.L.cells <= 64).
  the small-tier `final` rule of search_game_run (power < P.solver_power): test_small_tier_of_the_rollout -- at 255 and 256 a capped
      search is final in the small region, at 257 it is stopped one pop short and redone; p1000: searches of 250..262 pops finish on
      either side of the limit, and the 64 environments of block 0 all go to s_big.
  k_search_big (more than 256 bordered cells): test_route_f_beyond_256_cells.

Checked once against builds of the library with one rule changed (not kept in the tree): `power + 1 < P.solver_power` in
search_game_run fails test_small_tier_of_the_rollout[*-p257] for all three problems, on the last_pop levels and only there (the rest of
the suite's search tests pass with it); ddave's next() taking exhaustion for the end of the game fails the ddave cases of routes C and D,
of the generic rollout and of the tiers; stopped() answering yes to any winner fails routes A and B (sokoban-5x5, mdungeon, ddave), both
route E tests and route D.  With the library as it is every case passes: this module found no fault in search_game.h.
"""
import collections
import functools

import numpy as np
import pytest

import oracle_lib as ol

PROBLEMS = ("sokoban", "mdungeon", "ddave")
# where dist-win and sol-length sit in the row of oracle_lib.get_stats
WIN_COLS = {"sokoban": (4, 5), "mdungeon": (9, 10), "ddave": (9, 10)}
HEAVY_MIN = {"sokoban": 8, "mdungeon": 49, "ddave": 49}      # crates beyond SOKF_MAXC = 7, things beyond MDF_MAXI = 48, diamonds beyond DDF_MAXD = 48


# ------------------------------------------------------------------ levels
def _things_sokoban(rs, w, h, heavy, room=False):
    """Player, k crates, k targets, a few solid cells; one draw in eight breaks the solver's precondition."""
    area = w * h
    m = np.zeros((h, w), np.uint8)
    cells = rs.permutation(area)
    k = int(rs.randint(8, min(12, (area - 3) // 2) + 1)) if heavy else int(rs.randint(1, min(4, (area - 1) // 2) + 1))
    m.flat[cells[0]] = 2
    m.flat[cells[1:1 + k]] = 3
    m.flat[cells[1 + k:1 + 2 * k]] = 4
    free = area - 1 - 2 * k
    ns = int(rs.randint(0, max(1, min(free - 1, area // 5)) + 1)) if free > 1 else 0
    m.flat[cells[1 + 2 * k:1 + 2 * k + ns]] = 1
    if not heavy and rs.rand() < 0.125:
        m.flat[cells[1]] = (0, 2)[rs.randint(2)]            # a crate less than targets, or a second player
    return m


def _things_mdungeon(rs, w, h, heavy, room=False):
    """Player, exit, potions / treasures / goblins / ogres, some solid cells; three draws in ten (six in a small room) are crowded with enemies (the
    way to the exit costs more health than there is: long searches, agents that run out of states); one in eight has a second exit."""
    area = w * h
    m = np.zeros((h, w), np.uint8)
    cells = rs.permutation(area)
    m.flat[cells[0]] = 2
    m.flat[cells[1]] = 3
    crowded = not heavy and rs.rand() < (0.6 if room else 0.3)
    if heavy:
        k = int(rs.randint(49, min(60, area - 6) + 1))
    elif crowded:
        k = int(rs.randint(min(area - 2, area * 3 // 5 if room else area // 5), min(48, area - 2) + 1))
    else:
        k = int(rs.randint(0, min(8, area - 2) + 1))
    m.flat[cells[2:2 + k]] = rs.choice([4, 5, 6, 7], size=k, p=[0.1, 0.2, 0.2, 0.5] if crowded else [0.3, 0.3, 0.25, 0.15])
    room = area - 2 - k
    ns = int(rs.randint(0, min(8 if heavy else area // 4, max(0, room - 1)) + 1))
    m.flat[cells[2 + k:2 + k + ns]] = 1
    if not heavy and room - ns > 0 and rs.rand() < 0.125:
        m.flat[cells[2 + k + ns]] = 3
    return m


def _things_ddave(rs, w, h, heavy, room=False):
    """Ledges, then player, exit, key, diamonds and spikes anywhere; one draw in eight has no key."""
    area = w * h
    m = np.zeros((h, w), np.uint8)
    for _k in range(rs.randint(1, 5) if h > 1 else 0):
        y = rs.randint(1, h); x0 = rs.randint(0, w); x1 = rs.randint(x0, min(w, x0 + 8)) + 1
        m[y, x0:x1] = 1
    cells = rs.permutation(area)
    m.flat[cells[0]] = 2; m.flat[cells[1]] = 3; m.flat[cells[2]] = 5
    k = int(rs.randint(49, min(58, area - 8) + 1)) if heavy else int(rs.randint(0, min(4, area - 3) + 1))
    m.flat[cells[3:3 + k]] = 4
    m.flat[cells[3 + k:3 + k + rs.randint(0, 4)]] = 6
    if not heavy and rs.rand() < 0.125:
        m.flat[cells[2]] = 0
    return m


THINGS = {"sokoban": _things_sokoban, "mdungeon": _things_mdungeon, "ddave": _things_ddave}


def gen_level(prob, rs, w, h, heavy):
    """One level.  One draw in four (never a heavy one) is a small room of 3..25 cells somewhere in a solid map: few states, so
    that agents run out of them below any cap -- at every map size."""
    if heavy or rs.rand() >= 0.25:
        return THINGS[prob](rs, w, h, heavy)
    while True:
        rw, rh = int(rs.randint(1, min(w, 5) + 1)), int(rs.randint(1, min(h, 5) + 1))
        if rw * rh >= 3:
            break
    m = np.ones((h, w), np.uint8)
    x0, y0 = int(rs.randint(0, w - rw + 1)), int(rs.randint(0, h - rh + 1))
    m[y0:y0 + rh, x0:x0 + rw] = THINGS[prob](rs, rw, rh, False, room=True)
    return m


@functools.lru_cache(maxsize=None)
def _draws(prob, w, h, seed, n, heavy):
    rs = np.random.RandomState(seed)
    out = []
    while len(out) < n:
        m = gen_level(prob, rs, w, h, heavy)
        if ((m == 0) | (m == 1)).any():       # the driver needs a cell to flip between empty and solid
            out.append(m)
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def _tape(prob, w, h, seed, n, heavy, power):
    """The oracle's rows and per-agent pops of the draws at `power`."""
    maps = _draws(prob, w, h, seed, n, heavy)
    rows, its = [], []
    for m in maps:
        r, it = ol.get_stats(prob, m, solver_power=power, with_iters=True)
        rows.append(r); its.append(it.copy())
    return np.stack(rows), np.stack(its).astype(np.int64)


# ------------------------------------------------------------------ classes, from the oracle's tape alone
def classify(prob, row, it, power):
    """last: the last agent that ran (None: no search); end: how it ended -- 'won', 'out' (ran out of states: pops < power, no
    win) or 'cap' (pops >= power, no win); capped[a]: agent a ran and hit the cap.  The oracle runs the agents in sequence until
    one wins, so the agents that ran are a prefix of the order."""
    it = [int(p) for p in it]
    n = sum(1 for p in it if p > 0)
    assert all(p > 0 for p in it[:n]) and not any(it[n:]), it
    dw, sl = WIN_COLS[prob]
    win = n > 0 and int(row[dw]) == 0 and int(row[sl]) > 0
    capped = [a < n and it[a] >= power and not (win and a == n - 1) for a in range(4)]
    end = None if n == 0 else ("won" if win else ("cap" if capped[n - 1] else "out"))
    return dict(n=n, last=n - 1 if n else None, end=end, win=win, capped=capped, it=it, power=power,
                ran="".join("1" if a < n else "0" for a in range(4)), cap="".join("1" if c else "0" for c in capped))


def tags(prob, c):
    """The names of the classes (module docstring) a classified level belongs to."""
    n, it, power, cap, win = c["n"], c["it"], c["power"], c["capped"], c["win"]
    if n == 0:
        return {"none"}
    t = set()
    early = all(cap[:n - 1])                  # every agent before the last one hit the cap
    out = [a < n and it[a] < power and not (win and a == n - 1) for a in range(4)]       # ran out of states without a win
    if n == 1 and not cap[0]:
        t.add("a0")                           # (then it won: an agent that does not win is followed by the next)
    if n == 4 and all(cap):
        t.add("all_cap")
    if n == 4 and not any(cap):
        t.add("all_nocap")
    if prob == "sokoban":
        if win and n >= 2 and early:
            t.add("win%d" % (n - 1))
        if out[0]:
            t.add("bfs_out")
    elif prob == "mdungeon":
        if n >= 2 and early:
            t.add("tape" + "0123"[:n])
        if any(out[:3]):
            t.add("astar_out")
    else:
        if n in (2, 3):
            t.add("mid")
        if win and any(out[:n - 1]):
            t.add("won_after_out")            # exhaustion says nothing: a later agent won after an earlier one ran out
    t.add("cap" if any(cap) else "below")
    if not any(cap) and 250 <= max(it) <= 262:
        t.add("near256")
    if max(it) > 256:
        t.add("beyond256")
    return t


BASE = ("none", "a0", "all_cap", "all_nocap")
OWN = {"sokoban": ("win1", "win2", "win3", "bfs_out"), "mdungeon": ("tape01", "tape012", "tape0123", "astar_out"), "ddave": ("mid",)}


def minima(prob, kind):
    """The least count of every class a pool of this kind must hold."""
    need = {"heavy": 8, "heavy_ran": 4}
    if kind == "full":
        need.update({k: 4 for k in BASE + OWN[prob]})
        if prob == "ddave":
            need["mid"] = 2
    elif kind == "tier":
        # last_pop: the oracle's row at solver_power - 1 is another one -- the only levels on which a cap that is off by one shows.
        # About one draw in 2 000 (sokoban, mdungeon), so one is asked for and every one found is taken.
        need.update(cap=4, below=4, last_pop=1)
    elif kind == "p1000":
        need.update(near256=4, beyond256=64)
    elif kind == "arena":
        need.update(none=4, a0=4, cap=4, below=4)
    return need


# name -> (problem, width, height, solver_power, kind, seed, draws)
POOLS = {}


def _add(name, *spec):
    POOLS[name] = spec


for _p, _w, _h, _pw, _n in (("sokoban", 5, 5, 300, 6000), ("sokoban", 6, 6, 300, 4000), ("sokoban", 6, 7, 300, 4000),
                            ("mdungeon", 7, 11, 300, 6000), ("ddave", 11, 7, 300, 12000)):
    _add("%s-%dx%d" % (_p, _w, _h), _p, _w, _h, _pw, "full", 101, _n)
for _p, _w, _h, _pw, _n in (("sokoban", 15, 15, 300, 4000), ("mdungeon", 15, 15, 300, 6000), ("ddave", 15, 15, 300, 4000)):
    _add("%s-%dx%d" % (_p, _w, _h), _p, _w, _h, _pw, "full", 102, _n)
for _p, _w, _h in (("sokoban", 6, 6), ("mdungeon", 7, 11), ("ddave", 11, 7)):
    for _pw in (255, 256, 257):
        _add("%s-p%d" % (_p, _pw), _p, _w, _h, _pw, "tier", 103, 6000)
    _add("%s-p1000" % _p, _p, _w, _h, 1000, "p1000", 104, 6000)
    _add("%s-p5001" % _p, _p, _w, _h, 5001, "arena", 105, 3000)

QUOTA = 6            # levels taken per class (the minima are 4)
N_HEAVY_DRAWS = 40


@functools.lru_cache(maxsize=None)
def pool(name):
    """-> dict(prob, w, h, power, maps [N, h, w], rows, its, cls, tags, cell [N, 2] (x, y of the cell the driver flips), census)."""
    prob, w, h, power, kind, seed, ndraw = POOLS[name]
    maps = _draws(prob, w, h, seed, ndraw, False)
    rows, its = _tape(prob, w, h, seed, ndraw, False, power)
    need = minima(prob, kind)
    rows_less = _tape(prob, w, h, seed, ndraw, False, power - 1)[0] if kind == "tier" else rows
    last_pop = (rows != rows_less).any(1)
    quota = {k: 4 for k in BASE + OWN[prob] + ("cap", "below")}       # some of every class in every pool, asked for or not
    quota.update({k: max(QUOTA, v) for k, v in need.items()})
    quota["last_pop"] = 12
    have = collections.Counter()
    picked = []
    for i in range(ndraw):
        c = classify(prob, rows[i], its[i], power)
        tg = tags(prob, c)
        tg.add("tape:%s/%s%s" % (c["ran"], c["cap"], "w" if c["win"] else ""))        # and two of every tape there is
        if last_pop[i]:
            tg.add("last_pop")
        if any(have[k] < quota.get(k, 2 if k.startswith("tape:") else 0) for k in tg):
            picked.append((i, False))
            have.update(tg)
    if kind == "p1000":         # the block of the first 64 environments: every one of them beyond the small tier
        far = [p for p in picked if max(its[p[0]]) > 256]
        picked = far[:64] + [p for p in picked if p not in far[:64]]
    hmaps = _draws(prob, w, h, seed + 1000, N_HEAVY_DRAWS, True)
    hrows, hits = _tape(prob, w, h, seed + 1000, N_HEAVY_DRAWS, True, power)
    n_ran = n_idle = 0
    for i in range(N_HEAVY_DRAWS):
        ran = hits[i].max() > 0
        if (ran and n_ran < 8) or (not ran and n_idle < 4):
            picked.append((i, True))
            n_ran += ran; n_idle += not ran
    out_maps = np.stack([(hmaps if hv else maps)[i] for i, hv in picked])
    out_rows = np.stack([(hrows if hv else rows)[i] for i, hv in picked])
    out_its = np.stack([(hits if hv else its)[i] for i, hv in picked])
    cls = [classify(prob, r, it, power) for r, it in zip(out_rows, out_its)]
    tgs = []
    for (i, hv), m, c in zip(picked, out_maps, cls):
        tg = tags(prob, c)
        if not hv and last_pop[i]:
            tg.add("last_pop")
        if hv:
            assert {"sokoban": (m == 3).sum(), "mdungeon": (m >= 4).sum(), "ddave": (m == 4).sum()}[prob] >= HEAVY_MIN[prob]
            # counted apart: the classes above are the compact searches' -- but for the global arena, where every level takes the generic one
            tg = (tg if kind == "arena" else set()) | {"heavy"} | ({"heavy_ran"} if c["n"] else set())
        tgs.append(tg)
    census = collections.Counter()
    for tg in tgs:
        census.update(tg)
    rs = np.random.RandomState(seed + 7)
    cell = []
    for m in out_maps:
        ys, xs = np.nonzero(m <= 1)
        j = rs.randint(len(ys))
        cell.append((xs[j], ys[j]))
    return dict(name=name, prob=prob, w=w, h=h, power=power, kind=kind, maps=out_maps, rows=out_rows, its=out_its, cls=cls, tags=tgs,
                cell=np.array(cell, np.int32), census=dict(census), heavy=np.array([hv for _i, hv in picked]))


def census_shortfall(name):
    """-> the classes this pool holds too few of, {class: (count, least)}."""
    p = pool(name)
    need = minima(p["prob"], p["kind"])
    short = {k: (p["census"].get(k, 0), v) for k, v in need.items() if p["census"].get(k, 0) < v}
    if p["kind"] == "p1000" and not all("beyond256" in tg for tg in p["tags"][:64]):
        short["beyond256 in the first block"] = (sum("beyond256" in tg for tg in p["tags"][:64]), 64)
    if p["kind"] == "tier":
        exact = all(c["it"][a] == p["power"] for c in p["cls"] for a in range(4) if c["capped"][a])
        if not exact:
            short["capped at exactly the power"] = (0, 1)
    return short


def census_table(names=None):
    """The count of every class in every pool, one line per pool."""
    lines = []
    for name in names or sorted(POOLS):
        p = pool(name)
        lines.append("%-15s power %4d N %3d  %s" % (name, p["power"], len(p["maps"]), " ".join("%s=%d" % kv for kv in sorted(p["census"].items()))))
    return "\n".join(lines)


FULL = ["sokoban-5x5", "sokoban-6x6", "sokoban-6x7", "mdungeon-7x11", "ddave-11x7"]
BIG = ["sokoban-15x15", "mdungeon-15x15", "ddave-15x15"]
ARENA = ["sokoban-p5001", "mdungeon-p5001", "ddave-p5001"]
GENERIC = ["sokoban-6x6", "mdungeon-7x11", "ddave-11x7"]
TIERS = ["%s-p%d" % (p, pw) for p in PROBLEMS for pw in (255, 256, 257)]
P1000 = ["%s-p1000" % p for p in PROBLEMS]


def test_census_of_every_pool():
    """No GPU: every pool holds what its cases need -- the minima of minima() -- so that a change to a generator, a seed or a power
    cannot quietly empty a class.  On failure the whole table."""
    assert sorted(FULL + BIG + ARENA + TIERS + P1000) == sorted(POOLS)
    short = {name: census_shortfall(name) for name in sorted(POOLS)}
    short = {k: v for k, v in short.items() if v}
    assert not short, "classes with too few levels {pool: {class: (count, least)}}: %s\n%s" % (short, census_table())
    for name in POOLS:
        p = pool(name)
        assert 24 <= len(p["maps"]) <= 400
        big = ol.needs_big(p["prob"], p["w"], p["h"])
        assert big == (name in BIG)
        if name in FULL + TIERS + P1000:          # what pcgrl_rollout needs for k_step_solver
            assert p["power"] <= 5000 and p["h"] <= 16 and not big
    # both sides of S.L.cells <= 64 (sok_search_fast<1> / <4>)
    assert (6 + 2) * (6 + 2) == 64 and (6 + 2) * (7 + 2) > 64


# ------------------------------------------------------------------ the routes, on the GPU
def _torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _labels(p):
    return ["%s/%s%s %s" % (c["ran"], c["cap"], "w" if c["win"] else "", ",".join(sorted(t))) for c, t in zip(p["cls"], p["tags"])]


def _stats_route(name, tuning=None):
    """Route A: set_maps(M) -> env.stats against the oracle's rows."""
    _torch()
    from gym_pcgrl_amd.envs import BatchedPcgrlEnv
    p = pool(name)
    env = BatchedPcgrlEnv(prob=p["prob"], rep="wide", num_envs=len(p["maps"]), seed=1000, tuning=tuning)
    try:
        env.adjust_param(width=p["w"], height=p["h"])
        env.adjust_param(change_percentage=1.0, solver_power=p["power"])
        env.reset()
        env.set_maps(p["maps"])
        got = env.stats.cpu().numpy().astype(np.int64)
        assert env.check_status() == 0
        bad = np.nonzero((got != p["rows"]).any(1))[0]
        lab = _labels(p)
        assert bad.size == 0, [(int(i), lab[i], got[i].tolist(), p["rows"][i].tolist()) for i in bad[:6]]
        assert np.array_equal(env._bufs["map"].cpu().numpy(), p["maps"])
    finally:
        env.close()


def _route(name, route, tuning=None, **kw):
    _torch()
    import parity_harness as ph
    p = pool(name)
    return ph.search_game_case(p["prob"], p["w"], p["h"], p["power"], p["maps"], p["cell"], route, tuning=tuning, labels=_labels(p), **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("name", FULL)
def test_route_a_set_maps(name):
    """set_maps -> env.stats: the four concurrent agents (k_sokoban / k_mdungeon / k_ddave, MODE_SETMAP), the row parked in B.stats."""
    _stats_route(name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", FULL)
def test_route_b_steps(name):
    """step() four times: the list pipeline -- the concurrent kernels in MODE_STEP, the row parked in B.info (finish_search_item)."""
    _route(name, "step")


@pytest.mark.gpu
@pytest.mark.parametrize("name", FULL)
def test_route_c_rollout(name):
    """The four actions as one rollout(): k_step_solver, the agents in sequence (search_game_run, SearchGame::next)."""
    _route(name, "rollout")


@pytest.mark.gpu
@pytest.mark.parametrize("nslots", [8, 0], ids=["slots8", "slotsN"])
@pytest.mark.parametrize("pop_budget", [4, 40])
@pytest.mark.parametrize("name", FULL)
def test_route_d_async_ticks(name, pop_budget, nslots):
    """enable_async + tick: k_search_async.  With 4 pops a tick every level whose game takes more than one agent is suspended inside
    and between agents; with 8 slots most suspended searches find no slot (the overflow path); the heavy levels take the generic
    search in one piece."""
    p = pool(name)
    n = len(p["maps"])
    cnt = _route(name, "async", pop_budget=pop_budget, nslots=nslots or n)
    long_ones = sum(1 for c, t in zip(p["cls"], p["tags"]) if "heavy" not in t and max(c["it"]) > pop_budget)
    assert long_ones > 8 and cnt["suspended"] > 0, (cnt, long_ones)
    assert (cnt["overflow"] > 0) == (nslots == 8), cnt


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["stats", "step", "rollout"])
@pytest.mark.parametrize("name", GENERIC)
def test_route_e_generic_search_in_lds(name, route):
    """sok_generic = 1: every level through agent_generic with heap and table in LDS, on set_maps, steps and the rollout."""
    tuning = {"sok_generic": 1}
    if route == "stats":
        _stats_route(name, tuning)
    else:
        _route(name, route, tuning)


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["stats", "step"])
@pytest.mark.parametrize("name", ARENA)
def test_route_e_global_arena(name, route):
    """solver_power 5001: heap and table in the global arena, the generic search on lane 0; a rollout there is a sequence of steps."""
    if route == "stats":
        _stats_route(name)
    else:
        _route(name, route)


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["stats", "step", "rollout"])
@pytest.mark.parametrize("name", BIG)
def test_route_f_beyond_256_cells(name, route):
    """Levels of 17 x 17 = 289 bordered cells: k_search_big (search_big.h), against the oracle's build with wider limits."""
    if route == "stats":
        _stats_route(name)
    else:
        _route(name, route)


@pytest.mark.gpu
@pytest.mark.parametrize("name", TIERS + P1000)
def test_small_tier_of_the_rollout(name):
    """k_step_solver's two tiers at their edge: solver_power 255 and 256 (the small tier's 256-pop limit is the real cap: final),
    257 (a capped search is stopped one pop short and redone in the full region), and 1000 with searches of 250..262 pops and a
    block whose 64 environments all go to the deferred list s_big."""
    _route(name, "rollout")
