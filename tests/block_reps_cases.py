"""The cases of tests/test_gpu_block_reps.py (narrowcast, narrowmulti, turtlecast: k_update_block) and what their tapes contain, from
the CPU oracle alone -- shared by the GPU module, which steps the library through the same tapes, and test_block_reps_host.py, which
asserts the conditions without a GPU.  `PYTHONPATH=. python tests/block_reps_cases.py` prints every figure.

Terms.  The *cursor of a step* is where the cursor stood before the step (after the reset, if the step before ended an episode): the
centre of the block the step writes.  The *change* of a step is what it adds to `changes`: the info column of the step minus that of
the step before (minus 0 at the start of an episode).  A *write* is a step with a change of at least 1, a *multi-cell write* one of
at least 2, a *nine-cell write* one of exactly 9.  "seq" is random_start=False, random_tile=False: the cursor walks the cells in
row-major order from wherever the reset put it (the oracle's reset draws the cursor with or without random_start)."""
import numpy as np

import oracle_lib as ol
import parity_harness as ph

SEQ = dict(random_start=False, random_tile=False)
SEED = 8800


def _case(prob, rep, w, h, cp, E, T, seq=False, warp=None, floors=(), seed=SEED):
    calls = [dict(width=w, height=h), dict(change_percentage=cp)]
    if seq:
        calls.append(dict(SEQ))
    if warp is not None:
        calls.append(dict(warp=warp))
    return dict(prob=prob, rep=rep, calls=calls, E=E, T=T, seed=seed, floors=dict(floors))


# A: the geometry of the block write.  floors: figure of coverage() -> the least the oracle's tape must show ("corners": that many
# distinct corner cells had a write with the cursor on them -- four, or two on a map of one row or column).
A_CASES = {
    "binary-narrowmulti-3x3": _case("binary", "narrowmulti", 3, 3, 1.0, 8, 60, seq=True, floors=dict(corners=4, border=50, jump=10, done=50)),
    "binary-narrowmulti-1x1": _case("binary", "narrowmulti", 1, 1, 1.0, 8, 30, floors=dict(writes=20)),
    "binary-narrowcast-2x5": _case("binary", "narrowcast", 2, 5, 0.8, 8, 80, floors=dict(corners=4, change6=5)),
    "binary-narrowcast-1x6": _case("binary", "narrowcast", 1, 6, 0.8, 8, 80, floors=dict(corners=2, change3=1)),
    "binary-narrowcast-6x1": _case("binary", "narrowcast", 6, 1, 0.8, 8, 80, floors=dict(corners=2, change3=1)),
    "zelda-narrowmulti-33x4": _case("zelda", "narrowmulti", 33, 4, 0.4, 8, 200, seq=True, floors=dict(corners=4, word_cols=20, nine=10)),
    "zelda-narrowcast-32x16": _case("zelda", "narrowcast", 32, 16, 0.3, 6, 200, seq=True, floors=dict(corners=4, nine=1, done=1)),
    "zelda-narrowcast-16x17": _case("zelda", "narrowcast", 16, 17, 0.3, 6, 200, seq=True, floors=dict(corners=4, nine=1, done=1)),
    "zelda-turtlecast-5x4-warp": _case("zelda", "turtlecast", 5, 4, 0.8, 16, 200, warp=True, floors=dict(corners=4, nine=20, outward=20)),
    "zelda-turtlecast-5x4-nowarp": _case("zelda", "turtlecast", 5, 4, 0.8, 16, 200, warp=False, floors=dict(outward=20)),
    "binary-narrowcast-66x3": _case("binary", "narrowcast", 66, 3, 0.3, 6, 220, seq=True, floors=dict(corners=4, cols63=10, done=10)),
    "binary-narrowmulti-3x66": _case("binary", "narrowmulti", 3, 66, 0.3, 6, 220, seq=True, floors=dict(rows63=1)),
    "zelda-narrowmulti-130x3": _case("zelda", "narrowmulti", 130, 3, 0.2, 4, 400, seq=True, floors=dict(corners=4, edge_cols=20, nine=20)),
    "binary-turtlecast-65x65": _case("binary", "turtlecast", 65, 65, 0.01, 6, 200, warp=True, floors=dict(cols63=5, border_any=5, done=5)),
    "binary-narrowcast-255x2": _case("binary", "narrowcast", 255, 2, 0.02, 2, 600, seq=True, floors=dict(col254=1)),
}

# B: past done (auto_reset=False).  E 32..64, T 60..120.
BIG_OPEN = dict(probs={"empty": 0.97, "solid": 0.03}, random_probs=False)      # (the form test_gpu_block_reps.py's switch case steps with auto-reset, too)
SOKOBAN_HALF = [dict(change_percentage=0.5)]
B_CASES = {
    "binary-narrowcast-14x14": dict(prob="binary", rep="narrowcast", calls=[dict(width=14, height=14)], E=32, T=100, seed=SEED + 100),
    "zelda-narrowmulti": dict(prob="zelda", rep="narrowmulti", calls=[], E=32, T=60, seed=SEED + 101),
    "sokoban-turtlecast": dict(prob="sokoban", rep="turtlecast", calls=list(SOKOBAN_HALF), E=32, T=100, seed=SEED + 102),
    "mdungeon-narrowcast": dict(prob="mdungeon", rep="narrowcast", calls=[], E=32, T=80, seed=SEED + 103),
    # (an open mix: the oracle's statistics of a 90 x 70 map cost 50 times more on the default one, 14 s for this case)
    "binary-narrowmulti-90x70": dict(prob="binary", rep="narrowmulti", calls=[dict(width=90, height=70), dict(change_percentage=0.005), dict(BIG_OPEN)],
                                     E=32, T=60, seed=SEED + 104),
}


def _oracle(prob, rep, calls):
    o = ol.OracleEnv(prob, rep)
    for kw in calls:
        o.adjust_param(**kw)
    return o


def oracle_tape(case, auto_reset=True):
    """(acts [T, E, k], exp): the tape of a case, drawn as parity_harness.run_config draws it, and the oracle's rollouts of every
    environment (environment i seeded seed + i), each with the map and cursor it started from (map0, pos0) and its max_changes."""
    prob, rep, calls, E, T, seed = (case[k] for k in ("prob", "rep", "calls", "E", "T", "seed"))
    o = _oracle(prob, rep, calls)
    acts = ph.draw_actions(ph.action_dims(prob, rep, o.width, o.height), np.random.RandomState(seed), T, E)
    exp = []
    for i in range(E):
        o = _oracle(prob, rep, calls)
        o.seed(seed + i)
        start = o.reset()
        x = o.rollout(acts[:, i]) if auto_reset else ph.oracle_noreset(o, acts[:, i])
        x["map0"], x["pos0"], x["max_changes"] = start["map"], start["pos"].astype(np.int64), o.max_changes
        exp.append(x)
    return acts, exp


_TAPES = {}


def tape(kind, name):
    """The tape of case `name` of A or B, made once per process."""
    if (kind, name) not in _TAPES:
        _TAPES[(kind, name)] = oracle_tape({"A": A_CASES, "B": B_CASES}[kind][name], auto_reset=kind == "A")
    return _TAPES[(kind, name)]


WORD_COLS = (31, 32, 63, 64, 65, 127, 128)      # the last / first columns of a 32-bit and of the 64-bit words of a row mask
EDGE_COLS = (63, 64, 65, 127, 128)              # ... of the 64-bit words alone: what counts on a map of three words per row


def step_changes(x, auto_reset=True):
    """Per step of one oracle rollout: (change, `changes` before the step)."""
    ch = x["info"][:, -1].astype(np.int64)
    before = np.concatenate([[0], ch[:-1]])
    if auto_reset:
        before[1:][x["done"][:-1]] = 0
    return ch - before, before


def coverage(case, acts, exp):
    """What the tape of a case of A contains (see the module's docstring for the terms):
      done        episodes ended                          writes / nine   writes, nine-cell writes
      corners     distinct corner cells with a write      border          writes with the cursor on a border cell that is no corner
      border_any  writes with the cursor on the border    jump            steps that take `changes` from < max_changes - 1 to > max_changes
      word_cols   multi-cell writes with the cursor in column 31, 32, 63, 64, 65, 127 or 128 (on 33 columns: 31 / 32, the 32-bit boundary)
      edge_cols   multi-cell writes with the cursor in column 63, 64, 65, 127 or 128;  cols63: in column 63, 64 or 65
      rows63      the least number of writes with the cursor in row 63, in row 64, in row 65;  col254: writes with the cursor in column 254
      outward     turtlecast: moves with the cursor on the border, outwards (with warp they wrap, without they are stopped)
      change3 / change6   steps with a change of 3 / of 6;  hist[k]: steps with a change of k"""
    w, h = case["calls"][0]["width"], case["calls"][0]["height"]
    c = dict(done=0, writes=0, nine=0, border=0, border_any=0, jump=0, word_cols=0, edge_cols=0, cols63=0, col254=0, outward=0)
    hist = np.zeros(10, np.int64)
    rows = np.zeros(3, np.int64)
    corners = set()
    for i, x in enumerate(exp):
        d, before = step_changes(x)
        assert d.min() >= 0 and d.max() <= 9, (d.min(), d.max())
        cur = np.concatenate([x["pos0"][None], x["pos"][:-1]])
        cx, cy = cur[:, 0], cur[:, 1]
        on_x, on_y = (cx == 0) | (cx == w - 1), (cy == 0) | (cy == h - 1)
        wr = d >= 1
        hist += np.bincount(d, minlength=10)
        c["done"] += int(x["done"].sum())
        c["writes"] += int(wr.sum())
        c["nine"] += int((d == 9).sum())
        corners |= {(int(a), int(b)) for a, b in cur[wr & on_x & on_y]}
        c["border"] += int((wr & (on_x | on_y) & ~(on_x & on_y)).sum())
        c["border_any"] += int((wr & (on_x | on_y)).sum())
        c["jump"] += int(((before < x["max_changes"] - 1) & (before + d > x["max_changes"])).sum())
        c["word_cols"] += int(((d >= 2) & np.isin(cx, WORD_COLS)).sum())
        c["edge_cols"] += int(((d >= 2) & np.isin(cx, EDGE_COLS)).sum())
        c["cols63"] += int(((d >= 2) & np.isin(cx, (63, 64, 65))).sum())
        c["col254"] += int((wr & (cx == 254)).sum())
        rows += [int((wr & (cy == r)).sum()) for r in (63, 64, 65)]
        if case["rep"] == "turtlecast":
            t = acts[:, i, 0]
            c["outward"] += int((((t == 0) & (cx == 0)) | ((t == 1) & (cx == w - 1)) | ((t == 2) & (cy == 0)) | ((t == 3) & (cy == h - 1))).sum())
    c.update(corners=len(corners), rows63=int(rows.min()), change3=int(hist[3]), change6=int(hist[6]), hist=hist.tolist())
    return c


_COVER = {}


def cover_a(name):
    if name not in _COVER:
        _COVER[name] = coverage(A_CASES[name], *tape("A", name))
    return _COVER[name]


def check_case_a(name):
    """The floors of one case of A on the oracle's tape."""
    c = cover_a(name)
    short = {k: (c[k], v) for k, v in A_CASES[name]["floors"].items() if c[k] < v}
    assert not short, ("the tape of %s holds less than its case is there for (figure: (has, needs))" % name, short)


def check_histogram():
    """Over all cases of A, every change of 1..9 occurs."""
    hist = np.sum([cover_a(n)["hist"] for n in A_CASES], 0)
    assert (hist[1:] > 0).all(), hist.tolist()
    return hist.tolist()


def coverage_b(exp):
    """A case of B: environments that take at least 10 steps after their first done; the largest `changes` - max_changes at the end."""
    late = sum(1 for x in exp if x["done"].any() and len(x["done"]) - 1 - int(np.argmax(x["done"])) >= 10)
    return dict(envs=len(exp), late=late, over=max(int(x["info"][-1, -1]) - x["max_changes"] for x in exp))


def cover_b(name):
    if ("B", name) not in _COVER:
        _COVER[("B", name)] = coverage_b(tape("B", name)[1])
    return _COVER[("B", name)]


def check_case_b(name):
    c = cover_b(name)
    assert 4 * c["late"] >= c["envs"], ("under a quarter of the environments take 10 steps past their first done", name, c)


def check_sums_b():
    assert max(cover_b(n)["over"] for n in B_CASES) > 8, "no case ends more than 8 changes above max_changes"


def report(out=print):
    import time
    for name in A_CASES:
        t0 = time.time()
        c = cover_a(name)
        out("A %-28s %4.1fs %s" % (name, time.time() - t0, {k: c[k] for k in list(A_CASES[name]["floors"]) + ["writes", "done", "hist"]}))
        check_case_a(name)
    out("A change histogram 0..9: %s" % check_histogram())
    for name in B_CASES:
        t0 = time.time()
        c = cover_b(name)
        out("B %-28s %4.1fs %s" % (name, time.time() - t0, c))
        check_case_b(name)
    check_sums_b()


if __name__ == "__main__":
    report()
