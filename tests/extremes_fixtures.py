"""The extremes_<prob>_<H>x<W>.npz fixtures (tests/golden/make_golden.py gen_extremes: levels with 254 .. 257 and more tiles of one
kind at the smallest shapes that hold them) and what the library promises about them.  Test infrastructure only.

The device row of Dave and MiniDungeons has eight 32-bit slots for eleven statistics (csrc/pcgrl_algos.h, dd_pack / md_pack):
  ddave     slot 0 = player | exit << 8 | key << 16, slot 7 = col-diamonds | won << 24
  mdungeon  slot 7 = col-potions | col-treasures << 8 | col-enemies << 16 | won << 24
A row is WITHIN LIMITS when every count that shares a slot is at most 255: it must equal the reference bit for bit and leave the
status word at 0.  BEYOND the limits the count is stored saturated at 255, status bit 0 is raised (check_status(): RuntimeError) and
every column that owns a whole slot must still be exact."""
import glob
import os

import numpy as np

import oracle_lib as ol

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STAT_KEYS = {      # the order of the fixtures' columns (make_golden.py STAT_KEYS)
    "zelda": ["player", "key", "door", "enemies", "regions", "nearest-enemy", "path-length"],
    "sokoban": ["player", "crate", "target", "regions", "dist-win", "sol-length"],
    "mdungeon": ["player", "exit", "potions", "treasures", "enemies", "regions", "col-potions", "col-treasures", "col-enemies", "dist-win", "sol-length"],
    "ddave": ["player", "dist-floor", "exit", "diamonds", "key", "spikes", "regions", "num-jumps", "col-diamonds", "dist-win", "sol-length"],
}
SHARED = {"ddave": ["player", "exit", "key", "col-diamonds"], "mdungeon": ["col-potions", "col-treasures", "col-enemies"], "zelda": [], "sokoban": []}
OWN = {"ddave": ["dist-floor", "diamonds", "spikes", "regions"], "mdungeon": ["player", "exit", "potions", "treasures", "enemies", "regions"]}
ONCE_ONLY = {"ddave": ["player", "exit", "key"], "mdungeon": ["player", "exit"], "zelda": ["player", "key", "door"], "sokoban": ["player"]}
SET_A, SET_B, SET_C = [(16, 16)], [(13, 20), (8, 33)], [(4, 65)]
PACKED = ("ddave", "mdungeon")
ALL4 = ("ddave", "mdungeon", "zelda", "sokoban")
D_CASES = [("mdungeon", 3, 128), ("mdungeon", 3, 129), ("ddave", 3, 130)]      # the serpentines: (problem, h, w)


def cases(shapes, probs):
    return [(p, h, w) for (h, w) in shapes for p in probs]


def case_id(c):
    return "%s-%dx%d" % c


class Fixture:
    def __init__(self, prob, h, w):
        d = np.load(os.path.join(G, "extremes_%s_%dx%d.npz" % (prob, h, w)))
        self.prob, self.h, self.w = prob, h, w
        self.maps, self.stats, self.names, self.power = d["maps"], d["stats"].astype(np.int64), [str(x) for x in d["names"]], int(d["solver_power"])
        assert [str(k) for k in d["keys"]] == STAT_KEYS[prob] and self.maps.shape[1:] == (h, w) and len(self.maps) == len(self.stats) == len(self.names)
        self.within = within(prob, self.stats)

    def index(self, name):
        return self.names.index(name)


_CACHE = {}


def fixture(prob, h, w):
    if (prob, h, w) not in _CACHE:
        _CACHE[(prob, h, w)] = Fixture(prob, h, w)
    return _CACHE[(prob, h, w)]


def all_fixture_cases():
    out = []
    for p in sorted(glob.glob(os.path.join(G, "extremes_*.npz"))):
        _, prob, dims = os.path.basename(p)[:-4].split("_")
        h, w = (int(v) for v in dims.split("x"))
        out.append((prob, h, w))
    return out


def col(prob, stats, key):
    return np.asarray(stats)[..., STAT_KEYS[prob].index(key)]


def within(prob, stats):
    """bool per row of `stats` (STAT_KEYS order): every count that shares a slot is at most 255."""
    stats = np.asarray(stats)
    ok = np.ones(stats.shape[:-1], bool)
    for k in SHARED[prob]:
        ok &= col(prob, stats, k) <= 255
    return ok


def own_columns(prob):
    """Indices (STAT_KEYS order) of the columns that must be exact beyond the limits."""
    return [STAT_KEYS[prob].index(k) for k in OWN[prob]]


def mismatch(prob, got, want, names=None):
    """None, or a message: rows within limits must be equal in every column, the others in the columns that own a slot and saturated
    at 255 in the ones that share one.  got, want: [N, nstats] in STAT_KEYS order; `want` is the reference's."""
    got, want = np.asarray(got).astype(np.int64), np.asarray(want).astype(np.int64)
    assert got.shape == want.shape, (got.shape, want.shape)
    ok = within(prob, want)
    for i in range(len(want)):
        label = "%d%s" % (i, " (%s)" % names[i] if names is not None else "")
        if ok[i]:
            if not np.array_equal(got[i], want[i]):
                return "%s level %s within limits: got %s, the reference %s" % (prob, label, got[i].tolist(), want[i].tolist())
        else:
            own = own_columns(prob)
            if not np.array_equal(got[i, own], want[i, own]):
                return "%s level %s beyond limits, columns %s: got %s, the reference %s (rows %s / %s)" % (
                    prob, label, OWN[prob], got[i, own].tolist(), want[i, own].tolist(), got[i].tolist(), want[i].tolist())
            for k in SHARED[prob]:
                j = STAT_KEYS[prob].index(k)
                if got[i, j] != min(want[i, j], 255):
                    return "%s level %s beyond limits: %s is %d, not the saturated %d of the reference's %d" % (prob, label, k, got[i, j], min(want[i, j], 255), want[i, j])
    return None


def pack_rows(prob, stats):
    """The device rows [N, 8] int32 of `stats` (STAT_KEYS order), from the layout the header describes -- saturated counts included."""
    stats = np.asarray(stats).astype(np.int64)
    c = lambda k: col(prob, stats, k)
    s = lambda k: np.minimum(c(k), 255)
    rows = np.zeros((len(stats), 8), np.int64)
    if prob == "ddave":
        won = (c("sol-length") > 0).astype(np.int64)
        rows[:, 0] = s("player") | s("exit") << 8 | s("key") << 16
        rows[:, 1], rows[:, 2], rows[:, 3], rows[:, 4], rows[:, 5] = c("dist-floor"), c("diamonds"), c("spikes"), c("regions"), c("num-jumps")
        rows[:, 6] = np.where(won == 1, c("sol-length"), c("dist-win"))
        rows[:, 7] = s("col-diamonds") | won << 24
    elif prob == "mdungeon":
        won = (c("sol-length") > 0).astype(np.int64)
        for j, k in enumerate(STAT_KEYS[prob][:6]):
            rows[:, j] = c(k)
        rows[:, 6] = np.where(won == 1, c("sol-length"), c("dist-win"))
        rows[:, 7] = s("col-potions") | s("col-treasures") << 8 | s("col-enemies") << 16 | won << 24
    else:
        rows[:, :stats.shape[1]] = stats
    return rows.astype(np.int32)


def threshold_tape(fx, tile):
    """The scripted writes of one environment: from the level with 254 of `tile` on the first cells, wide actions [6, 3] (x, y, tile)
    that take the count to 255, 256, 257, 256, 255, 254 -- or, on a map of 256 cells, to 255, 256, 255, 256, 255, 254 -- one changed
    cell per step, and the counts themselves."""
    cells = fx.h * fx.w
    counts = [255, 256, 257, 256, 255, 254] if cells >= 257 else [255, 256, 255, 256, 255, 254]
    t = ol.TILES[fx.prob].index(tile)
    acts, n = [], 254
    for c in counts:
        cell, v = (n, t) if c > n else (n - 1, 0)
        acts.append([cell % fx.w, cell // fx.w, v])
        n = c
    return np.array(acts, np.int32), counts
