"""BatchedPcgrlEnv.paths() / pcgrl_get_paths on the GPU: the cells of the paths behind binary's path-length and zelda's path-length /
nearest-enemy, bit for bit against the legs that the reference's run_dikjstra maps define (tests/golden/paths.npz), the statistics
rows beside them, the grid-stride and max_len edges of k_get_paths, and a handle in the middle of its episodes left as it was."""
import ctypes as C
import os

import numpy as np
import pytest

import readout_harness as rh
from readout_harness import N_ENVS, make_env as _make, torch as _torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
G = os.path.join(HERE, "golden")
PASSABLE = {"binary": [[0]], "zelda": [[0, 2, 3, 5, 6, 7], [0, 2, 3, 4, 5, 6, 7], [0, 2, 5, 6, 7]]}
LEGS = {"binary": ("longest",), "zelda": ("key", "door", "enemy")}
GROUPS = ["stats_binary_%s" % s for s in ("1x1", "1x9", "8x1", "3x7", "5x5", "14x14", "16x11", "9x32", "64x64")] + \
         ["stats_zelda_%s" % s for s in ("5x5", "7x11", "11x16", "16x11")] + \
         ["rand_binary_%s" % s for s in ("5x40", "16x33", "16x32", "17x9", "17x33")] + ["rand_zelda_%s" % s for s in ("5x40", "16x33", "17x9")] + \
         ["hand_binary_64x64", "hand_binary_3x7", "hand_zelda_7x11"]


_CACHE = {}


def _group(name):
    """(problem, maps, stats, cells, length) of one group of the fixture: loaded once; the tests copy what they change."""
    if name not in _CACHE:
        fix = np.load(os.path.join(G, "paths.npz"))
        assert name in fix["groups"].tolist()
        prob = name.split("_")[1]
        if name.startswith("stats_"):
            d = np.load(os.path.join(G, name + ".npz"))
            maps, stats = d["maps"], d["stats"]
        else:
            maps, stats = fix["maps_" + name], fix["stats_" + name]
        _CACHE[name] = (prob, maps, stats, fix["cells_" + name], fix["length_" + name])
    return _CACHE[name]


def _padded(want, max_len):
    return rh.padded(want, max_len, np.int16)


def _same(a, b):
    torch = _torch()
    return all(torch.equal(x, y) for x, y in ((a.cells, b.cells), (a.length, b.length), (a.rows, b.rows)))


@pytest.mark.parametrize("name", GROUPS)
def test_fixture_paths(name):
    """cells, length and rows of every level of the group; rows are evaluate()'s; the lengths are the statistics'; every leg is a walk
    on its passable tiles."""
    torch = _torch()
    from gym_pcgrl_amd import check_path
    prob, maps, stats, want, wlen = _group(name)
    h, w = maps.shape[1:]
    env = _make(prob, h, w)
    p = env.paths(maps)
    ev = env.evaluate(maps)
    assert p.legs == LEGS[prob] and p.cells.dtype == torch.int16 and p.length.dtype == torch.int32
    assert tuple(p.cells.shape) == (maps.shape[0], len(LEGS[prob]), h * w) and tuple(p.length.shape) == (maps.shape[0], len(LEGS[prob]))
    cells, length, rows = p.cells.cpu().numpy(), p.length.cpu().numpy(), p.rows.cpu().numpy()      # one copy to the host
    assert np.array_equal(length, wlen), np.nonzero(length != wlen)
    assert np.array_equal(cells, _padded(want, h * w)), np.nonzero((cells != _padded(want, h * w)).any((1, 2)))
    ns = stats.shape[1]
    assert np.array_equal(rows[:, :ns], stats) and (rows[:, ns:] == 0).all() and torch.equal(p.rows, ev.rows)
    assert np.array_equal(p.exists.cpu().numpy(), wlen >= 0) and not p.truncated.any().item()
    if prob == "binary":
        has = length[:, 0] >= 0
        assert np.array_equal(length[has, 0], rows[has, 1]) and np.array_equal(has, (maps == 0).any((1, 2)))
    else:
        both = (rows[:, 0] == 1) & (rows[:, 4] == 1) & (rows[:, 1] == 1) & (rows[:, 2] == 1)
        assert np.array_equal(length[:, 0] >= 0, both) and (length[~both, 1] == -1).all()
        assert np.array_equal(length[both, 0] + length[both, 1], rows[both, 6])
        en = length[:, 2] >= 0
        assert np.array_equal(length[en, 2], rows[en, 5])
        assert (rows[~en & (rows[:, 0] == 1) & (rows[:, 4] == 1) & (rows[:, 3] > 0), 5] == h * w).all()
    for i, leg in zip(*np.nonzero(length >= 0)):
        r = check_path(maps[i], cells[i, leg], PASSABLE[prob][leg])
        assert r.ok and r.legal.shape == (length[i, leg] + 1,), (i, leg)
    x, y = p.xy()
    assert torch.equal(x >= 0, p.cells >= 0) and torch.equal((y * w + x)[p.cells >= 0], p.cells[p.cells >= 0]) and (y[p.cells < 0] == -1).all().item()
    assert env.check_status() == 0
    env.close()


# 16 lanes: sixteen maps a block and round; 64 lanes: four.  The last count is beyond what 8 192 blocks take in one round.
@pytest.mark.parametrize("name,count", [("stats_binary_3x7", c) for c in (1, 15, 16, 17, 8192 * 16 + 5)] +
                         [("stats_zelda_5x5", c) for c in (1, 15, 17)] + [("rand_binary_17x9", c) for c in (1, 3, 4, 5)] + [("rand_zelda_17x9", 5)])
def test_grid_stride_edges(name, count):
    torch = _torch()
    prob, maps, stats, want, wlen = _group(name)
    h, w = maps.shape[1:]
    pick = np.random.RandomState(count).permutation(maps.shape[0])
    pick = np.concatenate([pick[np.argsort(wlen[pick].max(1) < 0, kind="stable")]] * (count // len(pick) + 1))[:count]      # (a level with a leg first)
    env = _make(prob, h, w)
    m = torch.as_tensor(np.ascontiguousarray(maps[pick])).to(env.device)
    p = env.paths(m)
    chunk = 4096
    parts = [env.paths(m[i:i + chunk]) for i in range(0, count, chunk)]
    assert torch.equal(p.cells, torch.cat([q.cells for q in parts])) and torch.equal(p.length, torch.cat([q.length for q in parts]))
    assert torch.equal(p.rows, torch.cat([q.rows for q in parts]))
    k = min(count, 600)                                  # ... and against the fixture
    assert np.array_equal(p.length[:k].cpu().numpy(), wlen[pick[:k]]) and np.array_equal(p.cells[:k].cpu().numpy(), _padded(want[pick[:k]], h * w))
    assert np.array_equal(p.length[-k:].cpu().numpy(), wlen[pick[-k:]]) and np.array_equal(p.cells[-k:].cpu().numpy(), _padded(want[pick[-k:]], h * w))
    assert (p.length[0] >= 0).any().item()
    env.close()


@pytest.mark.parametrize("name", ["stats_binary_14x14", "stats_zelda_7x11", "rand_binary_17x33"])
def test_max_len_and_row_bounds(name):
    """Rows shorter than the legs: the full length, the prefix, the -1 fill, `truncated`; and through the C entry point nothing is
    written outside [count, legs, max_len] -- guard values on both sides of the outputs stay intact."""
    torch = _torch()
    prob, maps, stats, want, wlen = _group(name)
    h, w = maps.shape[1:]
    M, legs = maps.shape[0], wlen.shape[1]
    full = int(wlen.max())
    assert full >= 3
    env = _make(prob, h, w)
    dev = env.device
    m = torch.as_tensor(np.ascontiguousarray(maps)).to(dev)
    cfg = env._config()
    for max_len in (1, 2, full, full + 1, full + 2):
        p = env.paths(m, max_len=max_len)
        assert np.array_equal(p.length.cpu().numpy(), wlen) and np.array_equal(p.cells.cpu().numpy(), _padded(want, max_len)), max_len
        assert np.array_equal(p.truncated.cpu().numpy(), wlen + 1 > max_len) and p.truncated.any().item() == (max_len < full + 1)
        cl, ln, rw = rh.Guarded(torch.int16, M * legs * max_len, dev), rh.Guarded(torch.int32, M * legs, dev), rh.Guarded(torch.int32, M * 8, dev)
        need = int(env._lib.pcgrl_get_paths_bytes(C.byref(cfg), M, max_len))
        assert need >= 256
        work = torch.empty((need,), dtype=torch.uint8, device=dev)
        for rows_ptr in (rw.ptr, None):                  # (the second time no rows wanted)
            rh.guarded_call((cl, ln, rw), lambda a, b, _: env._lib.pcgrl_get_paths(env._handle, rh.ptr(m), M, max_len, a, b, rows_ptr, rh.ptr(work), need, env._stream()))
            assert torch.equal(cl.inner.view(M, legs, max_len), p.cells) and torch.equal(ln.inner.view(M, legs), p.length)
            assert torch.equal(rw.inner.view(M, 8), p.rows)
        # refusals: a workspace one byte short, max_len 0, count 0, no cells
        args = lambda **kw: (env._handle, rh.ptr(m), kw.get("count", M), kw.get("max_len", max_len), kw.get("cells", cl.ptr),
                             ln.ptr, None, rh.ptr(work), kw.get("need", need), env._stream())
        for kw in (dict(need=need - 1), dict(max_len=0), dict(count=0), dict(cells=None)):
            assert env._lib.pcgrl_get_paths(*args(**kw)) == -1, kw
    assert env.check_status() == 0
    env.close()


# ------------------------------------------------------------------ the handle is left alone
@pytest.mark.parametrize("prob,rep", [("binary", "narrow"), ("zelda", "wide")])
def test_handle_in_the_middle_of_its_episodes(prob, rep):
    torch = _torch()
    from gym_pcgrl_amd.envs import BatchedPcgrlEnv
    n = 24

    def sample(env):
        W, H, nt = env._prob._width, env._prob._height, env.get_num_tiles()
        rs = np.random.RandomState(3)
        if rep == "narrow":
            return rs.randint(0, nt + 1, size=(40, n)).astype(np.int32)
        return np.stack([rs.randint(0, W, size=(40, n)), rs.randint(0, H, size=(40, n)), rs.randint(0, nt, size=(40, n))], -1).astype(np.int32)

    def after_own(env, own):
        assert tuple(own.cells.shape) == (n, len(LEGS[prob]), env._prob._height * env._prob._width)
        ns = 2 if prob == "binary" else 7
        assert torch.equal(own.rows[:, :ns], env._bufs["stats"][:, :ns])
        assert (own.length >= 0).any().item()

    names = ("map", "old_map", "planes", "stats", "start_stats", "counters", "heatmap", "pos", "reward", "done", "rng_cursor", "rng_rep", "rng_prob", "info")
    rh.check_handle_left_alone(lambda: BatchedPcgrlEnv(prob=prob, rep=rep, num_envs=n, seed=77), sample, lambda env, *m: env.paths(*m), ("cells", "length", "rows"),
                               lambda env: [k for k in names if env._bufs.get(k) is not None], after_own, twin_too=True)


@pytest.mark.parametrize("name", ["stats_binary_5x5", "stats_zelda_7x11"])
def test_bad_tile_is_clamped_and_reported(name):
    prob, maps, stats, want, wlen = _group(name)
    h, w = maps.shape[1:]
    env = _make(prob, h, w)
    rh.check_bad_tile(env, env.paths, ("cells", "length", "rows"), maps[:40], [(i, i % h, (2 * i) % w) for i in range(5)])
    env.close()


def test_refusals_and_the_one_call_form():
    _torch()
    import gym_pcgrl_amd
    for prob, pointer in (("sokoban", "solve()"), ("mdungeon", "playthrough()"), ("ddave", "playthrough()"), ("smb", "playthrough_smb()")):
        h, w = (5, 5) if prob != "smb" else (8, 20)
        env = _make(prob, h, w)
        with pytest.raises(NotImplementedError, match=pointer.replace("(", r"\(").replace(")", r"\)")):
            env.paths(np.zeros((2, h, w), np.uint8))
        env.close()
    for prob in ("binary", "zelda"):
        env = _make(prob, 65, 64)
        with pytest.raises(NotImplementedError, match="64 x 64"):
            env.paths(np.zeros((2, 65, 64), np.uint8))
        env.close()
    env = _make("binary", 5, 5)
    with pytest.raises(RuntimeError):
        env.paths()                                               # before reset()
    with pytest.raises(ValueError):
        env.paths(np.zeros((2, 5, 6), np.uint8))
    with pytest.raises(ValueError):
        env.paths(np.zeros((2, 5, 5), np.uint8), max_len=0)
    for name in ("stats_binary_5x5", "stats_zelda_7x11"):            # the one-call form equals paths() on a handle
        prob, maps, stats, want, wlen = _group(name)
        h, w = maps.shape[1:]
        one = gym_pcgrl_amd.path_levels(prob, maps, max_len=want.shape[2])
        e2 = _make(prob, h, w)
        assert _same(one, e2.paths(maps, max_len=want.shape[2]))
        assert np.array_equal(one.cells.cpu().numpy(), want) and np.array_equal(one.length.cpu().numpy(), wlen)
        e2.close()
    env.close()
