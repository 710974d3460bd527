"""BatchedPcgrlEnv: N lockstep PcgrlEnv instances on one MI355X.

Mirrors the reference's PcgrlEnv (pcgrl_env.py) method for method -- seed / reset / step /
adjust_param / get_border_tile / get_num_tiles -- with a leading environment axis, vector-env
auto-reset (the reference leaves that to SubprocVecEnv, utils.py:60-71) and torch tensors that are
zero-copy views of the state the HIP kernels own.  All computation happens in
gym_pcgrl_amd/lib/libpcgrl_hip.so through the C ABI of include/pcgrl_hip.h; there is no CPU path.
"""
import ctypes as C
from collections import OrderedDict

import numpy as np

from .. import _lib, seeding, spaces
from .problems import PROB_IDS, PROBLEMS
from .representations import REP_IDS, REPRESENTATIONS


class InfoBatch:
    """Struct-of-tensors view of the per-step info dicts (pcgrl_env.py:144-148)."""

    def __init__(self, keys, table, max_iterations, max_changes, decode=None):
        self.keys = list(keys)
        self.table = table            # int32 [N,10]: problem info (8 slots), iterations, changes
        self.max_iterations = max_iterations
        self.max_changes = max_changes
        self._decode = decode         # Problem.decode_rows for rows that pack several values into a slot (mdungeon)

    def __getitem__(self, key):
        if key == "iterations":
            return self.table[:, 8]
        if key == "changes":
            return self.table[:, 9]
        if key == "max_iterations":
            return self.max_iterations
        if key == "max_changes":
            return self.max_changes
        if self._decode is not None:
            return self._decode(self.table, [key])[:, 0]
        return self.table[:, self.keys.index(key)]

    def to_list(self):
        t = self.table.cpu().numpy()
        vals = self._decode(self.table, self.keys).cpu().numpy() if self._decode is not None else t
        out = []
        for row, v in zip(t, vals):
            d = {k: int(v[i]) for i, k in enumerate(self.keys)}
            d["iterations"] = int(row[8])
            d["changes"] = int(row[9])
            d["max_iterations"] = self.max_iterations
            d["max_changes"] = self.max_changes
            out.append(d)
        return out


class Evaluation:
    """What BatchedPcgrlEnv.evaluate() returns: `rows` int32 [M, 8] (the packed device rows, include/pcgrl_hip.h pcgrl_layout.stats),
    `stats` (the same decoded: the columns of env.stats), and -- with a `ref` -- `reward` float64 [M] and `over` bool [M]; None without."""
    __slots__ = ("rows", "stats", "reward", "over")

    def __init__(self, rows, stats, reward=None, over=None):
        self.rows, self.stats, self.reward, self.over = rows, stats, reward, over


class _PlannerMoves:
    """What Solutions and Playthroughs share: a planner's move rows for a batch of levels."""
    __slots__ = ("moves", "length", "agent", "rows", "stats")

    def __init__(self, moves, length, agent, rows, stats):
        self.moves, self.length, self.agent, self.rows, self.stats = moves, length, agent, rows, stats

    @property
    def truncated(self):
        return self.length > self.moves.shape[1]


class Solutions(_PlannerMoves):
    """What BatchedPcgrlEnv.solve() returns: `moves` int8 [M, max_len] (0..3 = left, right, up, down; -1 beyond the solution),
    `length` int32 [M] (the full len(solution), also beyond max_len), `agent` int8 [M] (-2 the planner did not run, -1 no agent won,
    0..3 = BFS, A*(1), A*(0.5), A*(0)), `rows` / `stats` as in an Evaluation; `truncated` bool [M]: the row holds only a prefix."""
    __slots__ = ()


class Playthroughs(_PlannerMoves):
    """What BatchedPcgrlEnv.playthrough() and playthrough_smb() return: `moves` int8 [M, max_len] (mdungeon 0..3 = left, right, up,
    down; ddave 0..3 = stay, left, right, jump; smb 0..3 = stay, right, jump, right + jump; -1 beyond the play), `length` int32 [M]
    (the depth of the node the statistics come from, also beyond max_len), `agent` int8 [M] (-2 the planner did not run, -1 no agent
    won, 0..3 = A*(1), A*(0.5), A*(0), BFS; smb: -1 nobody won, 0 = A*(1), 1 = A*(0), never -2), `rows` / `stats` as in an
    Evaluation; `truncated` bool [M]: the row holds only a prefix; `won` bool [M]: an agent won."""
    __slots__ = ()

    @property
    def won(self):
        return self.agent >= 0


class Paths:
    """What BatchedPcgrlEnv.paths() returns: `cells` int16 [M, legs, max_len] (cell i of each leg as y * W + x, start -> target; -1 beyond
    the leg), `length` int32 [M, legs] (the full length in steps, also beyond max_len; -1: the leg does not exist), `rows` / `stats` as in
    an Evaluation; `legs`: the legs' names -- ("longest",) for binary, ("key", "door", "enemy") for zelda; `exists` bool [M, legs];
    `truncated` bool [M, legs]: the row holds only a prefix; xy(): the cells as (x, y)."""
    __slots__ = ("cells", "length", "rows", "stats", "legs", "width")

    def __init__(self, cells, length, rows, stats, legs, width):
        self.cells, self.length, self.rows, self.stats, self.legs, self.width = cells, length, rows, stats, legs, width

    @property
    def exists(self):
        return self.length >= 0

    @property
    def truncated(self):
        return self.length + 1 > self.cells.shape[2]

    def xy(self):
        """(x, y): two int16 tensors shaped like `cells`, -1 where the cell is -1."""
        c = self.cells
        none = c < 0
        x, y = c % self.width, c // self.width
        return x.masked_fill(none, -1), y.masked_fill(none, -1)


class Changes:
    """What BatchedPcgrlEnv.changes() returns, entry [m, k, t] being level m with cell cells[m, k] set to tile t: `rows` int32 [M, K, T, 8]
    (None with rows=False), `reward` float64 [M, K, T] (new = the entry's row, old = the level's own), `over` bool [M, K, T],
    `base_rows` int32 [M, 8] (the levels' own rows: evaluate()'s), `cells` int32 [M, K] (y * W + x), `stats`: base_rows decoded."""
    __slots__ = ("rows", "reward", "over", "base_rows", "cells", "stats")

    def __init__(self, rows, reward, over, base_rows, cells, stats):
        self.rows, self.reward, self.over, self.base_rows, self.cells, self.stats = rows, reward, over, base_rows, cells, stats


class Connectivity:
    """What BatchedPcgrlEnv.connectivity() returns, all on the device, None where not asked for: `regions` int32 [M] (calc_num_regions),
    `longest` int32 [M] (calc_longest_path), `labels` int16 [M, H, W] (calc_num_regions' color_map: -1 on impassable cells, else 1 ..
    regions in the row-major order of the regions' first cells), `dist` int16 [M, H, W] (run_dikjstra's map from the source, -1 where
    unreached), `reach` int32 [M] (calc_num_reachable_tile), `source` int32 [M] (the source cell that was used, y * W + x, -1: none)."""
    __slots__ = ("regions", "longest", "labels", "dist", "reach", "source")

    def __init__(self, regions, longest, labels, dist, reach, source):
        self.regions, self.longest, self.labels, self.dist, self.reach, self.source = regions, longest, labels, dist, reach, source


class TileStats:
    """What BatchedPcgrlEnv.tile_stats() returns, all on the device, None where not asked for: `counts` int32 [M, 32] (the cells that
    hold tile t), `floor_dist` int32 [M] (get_floor_dist), `floor_map` int16 [M, H, W] (_calc_dist_floor of every cell), `grouping`
    int32 [M] (get_type_grouping), `group_map` int8 [M, H, W] (_calc_group_value of every cell), `changes` int32 [M, 2]
    (get_changes horizontal, vertical)."""
    __slots__ = ("counts", "floor_dist", "floor_map", "grouping", "group_map", "changes")

    def __init__(self, counts, floor_dist, floor_map, grouping, group_map, changes):
        self.counts, self.floor_dist, self.floor_map, self.grouping, self.group_map, self.changes = counts, floor_dist, floor_map, grouping, group_map, changes


def expand_changes(flat, cells, first, n, ntiles):
    """The expansion rule of changes(): entries `first` .. `first + n - 1` in the order (m, k, t) -- entry (m * K + k) * T + t is level m
    with cell cells[m, k] set to tile t -- of `flat` uint8 [M, H * W] and `cells` int64 [M, K] (torch tensors on one device, the CPU
    included).  Returns (levels uint8 [n, H * W], the level m of each entry, noop bool [n]: the cell already holds the tile -- a tile
    id beyond the last counts as the last one, what the scoring clamps it to)."""
    import torch
    e = torch.arange(first, first + n, dtype=torch.int64, device=flat.device)
    t, col = e % ntiles, e // ntiles
    k, lv = col % cells.shape[1], col // cells.shape[1]
    cell = cells[lv, k]
    levels = flat[lv]                                              # (a copy: advanced indexing)
    row = torch.arange(n, device=flat.device)
    noop = levels[row, cell].clamp(max=ntiles - 1) == t
    levels[row, cell] = t.to(torch.uint8)
    return levels, lv, noop


class BatchedPcgrlEnv:
    metadata = {"render.modes": []}

    def __init__(self, prob="binary", rep="narrow", num_envs=1, device=None, seed=None, auto_reset=True, strict_actions=False, tuning=None):
        """strict_actions: check after every step() / rollout() whether an action was outside the action space and raise IndexError
        at the offending call, like the reference does (wide_rep.py:68-69 ...); costs a device synchronisation per step, so it is
        off by default -- the actions are then clamped and the status word reports it (check_status()).
        tuning: {switch: value} for the library's developer switches (include/pcgrl_hip.h pcgrl_tuning; A/B measurements, tests)."""
        import torch
        self._torch = torch
        self._lib = _lib.load()                      # fails loudly when the HIP library is absent
        self._prob = PROBLEMS[prob]()                # KeyError on unknown names, like pcgrl_env.py:28-29
        self._rep = REPRESENTATIONS[rep]()
        self.num_envs = int(num_envs)
        self.auto_reset = bool(auto_reset)
        self.strict_actions = bool(strict_actions)
        self._tuning = dict(tuning or {})
        if device is None:
            device = "cuda:0"
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("BatchedPcgrlEnv runs on an AMD GPU only (device=%r); there is no CPU fallback" % (device,))
        # pcgrl_env.py:33-34
        self._max_changes = max(int(0.2 * self._prob._width * self._prob._height), 1)
        self._max_iterations = self._max_changes * self._prob._width * self._prob._height
        self._handle = None
        self._bufs = None
        self._rng = None
        self._episode = None          # RNG tensors survive re-allocation on width/height changes
        self._needs_reset = True
        self._realloc = False
        self._alloc_dims = None
        self._probs_dirty = False
        self._obs_spec = None          # bind_observation(): (out tensor, h, w, centered, pad, onehot)
        self._async = None             # enable_async(): arena tensor + views (pending, counters)
        self._async_nslots = 0
        self._row = None               # bind_rollout_row(): (column pointers in _lib.ROW_FIELDS order, the tensors kept alive)
        self._row_applied = None       # what the handle was last told (pcgrl_bind_row): (column pointers, actions are int64)
        self._eval_work = None         # evaluate(): the workspace of pcgrl_get_stats, regrown on demand
        self._eval_scratch = None      # evaluate(), configurations without a fast form: a private scratch environment
        self._was_reset = False        # the handle has been reset since it was allocated: it carries episodes
        self._update_spaces()
        self.seed(seed)

    # ------------------------------------------------------------------ spaces / simple getters
    def _update_spaces(self):
        w, h, t = self._prob._width, self._prob._height, self.get_num_tiles()
        self.single_action_space = self._rep.get_action_space(w, h, t)
        self.single_observation_space = self._rep.get_observation_space(w, h, t)
        self.single_observation_space.spaces["heatmap"] = spaces.Box(low=0, high=self._max_changes, dtype=np.uint8, shape=(h, w))
        self.action_space = self.single_action_space
        self.observation_space = self.single_observation_space

    def get_border_tile(self):
        return self._prob.get_tile_types().index(self._prob._border_tile)

    def get_num_tiles(self):
        return len(self._prob.get_tile_types())

    # ------------------------------------------------------------------ config plumbing
    def _config(self, map_dims=None):
        """map_dims: (width, height) of the allocated maps when they are not the problem's -- adjust_param(width, height) without a
        reset(): the reference goes on stepping the old maps with the problem's new size in its formulas (pcgrl_env.py:106-115)."""
        c = _lib.Config()
        c.prob, c.rep, c.num_envs = PROB_IDS[self._prob.name], REP_IDS[self._rep.name], self.num_envs
        c.width, c.height = (int(self._prob._width), int(self._prob._height)) if map_dims is None else (int(map_dims[0]), int(map_dims[1]))
        c.prob_width, c.prob_height = int(self._prob._width), int(self._prob._height)
        # (pcgrl_env.py:33-34 computes max_iterations = max_changes * W * H with Python integers; the device field and the iteration
        #  counter it is compared with are 32-bit: beyond 2^31 - 1 -- e.g. 255 x 255 with change_percentage above 0.5 -- the limit is
        #  one no episode can reach either way, and the info dict keeps reporting the exact value from the host side)
        c.max_changes, c.max_iterations = int(self._max_changes), min(int(self._max_iterations), 2 ** 31 - 1)
        c.random_start, c.random_tile, c.warp, c.random_probs = 1, 1, 0, 0
        c.auto_reset = int(self.auto_reset)
        for k, v in list(self._prob.device_params().items()) + list(self._rep.device_params().items()):
            setattr(c, k, v)
        for i, t in enumerate(self._prob.tiles):
            c.tile_probs[i] = float(self._prob._prob[t])
        for i, k in enumerate(self._prob.reward_keys):
            c.rewards[i] = float(self._prob._rewards[k])
        return c

    def _stream(self):
        return C.c_void_p(self._torch.cuda.current_stream(self.device).cuda_stream)

    def _free(self):
        if self._handle is not None:
            self._torch.cuda.synchronize(self.device)
            self._lib.pcgrl_destroy(self._handle)
            self._handle = None
        self._bufs = None

    def _allocate(self):
        torch = self._torch
        self._free()
        cfg = self._config()
        lay = _lib.Layout()
        _lib.check(self._lib.pcgrl_query_layout(C.byref(cfg), C.byref(lay)), "pcgrl_query_layout")
        n, w, h = self.num_envs, cfg.width, cfg.height
        dev = self.device
        mask_dtype = torch.int32 if lay.mask_bytes == 4 else torch.int64
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        b = OrderedDict()
        b["map"] = z((n, h, w), torch.uint8)
        b["old_map"] = z((n, h, w), torch.uint8)
        b["heatmap"] = z((n, h, w), torch.int16 if lay.heatmap == 2 * n * h * w else torch.int32)     # 32-bit counts without auto-reset
        b["pos"] = z((n, 2), torch.uint8)
        b["planes"] = z((n, lay.group, lay.nplanes), mask_dtype) if lay.nplanes else z((2,), mask_dtype)   # smb keeps no bit planes
        b["counters"] = z((n, 2), torch.int32)
        b["stats"] = z((n, 8), torch.int32)
        b["start_stats"] = z((n, 8), torch.int32)
        b["info"] = z((n, 10), torch.int32)
        b["reward"] = z((n,), torch.float64)
        b["done"] = z((n,), torch.uint8)
        first = self._rng is None
        if first:
            self._rng = OrderedDict()
            self._rng["tile_p"] = z((n, 2), torch.float64)      # BinaryProblem._prob per environment
            self._rng["rng_rep"] = z((n, seeding.MT_N), torch.int32)
            self._rng["rng_prob"] = z((n, seeding.MT_N), torch.int32) if self._prob.name == "binary" else None
            self._rng["rng_cursor"] = z((n, 2), torch.int32)
            self._rng_seeded = False
        b.update(self._rng)
        b["scratch"] = z((int(lay.scratch),), torch.uint8)
        for name in _lib.BUFFER_NAMES:
            t = b[name]
            if t is not None:
                assert t.is_contiguous() and t.numel() * t.element_size() >= getattr(lay, name), name
        handle = C.c_void_p()
        _lib.check(self._lib.pcgrl_create(C.byref(cfg), C.byref(handle)), "pcgrl_create")
        tun = _lib.make_tuning(self._tuning)
        _lib.check(self._lib.pcgrl_set_tuning(handle, C.byref(tun)), "pcgrl_set_tuning")
        bufs = _lib.Buffers()
        for name in _lib.BUFFER_NAMES:
            setattr(bufs, name, b[name].data_ptr() if b[name] is not None else None)
        _lib.check(self._lib.pcgrl_bind(handle, C.byref(bufs), self._stream()), "pcgrl_bind")
        self._handle, self._bufs, self._layout = handle, b, lay
        self._was_reset = False
        self._alloc_dims = (w, h)
        if first or self._probs_dirty:
            _lib.check(self._lib.pcgrl_set_tile_probs(self._handle, self._stream()), "pcgrl_set_tile_probs")
            self._probs_dirty = False
        if not self._rng_seeded:
            self._upload_seeds()
        if self._episode is not None:      # rebinding after a reallocation keeps the running episodes' sums
            self._bind_episode_stats()
        self._apply_observation()
        self._row_applied = None       # (a new handle: the row binding is applied again by the next step)
        self._async = None
        if self._async_nslots:
            self._bind_async()

    def _upload_seeds(self):
        words = np.ascontiguousarray(self._seed_keys, dtype=np.uint32)      # [N, 3]: the MT19937 states are made on the device
        _lib.check(self._lib.pcgrl_seed_words(self._handle, words.ctypes.data_as(C.c_void_p), 0, self.num_envs, self._stream()), "pcgrl_seed_words")
        self._rng_seeded = True

    # ------------------------------------------------------------------ reference surface
    def seed(self, seed=None):
        """Environment i is seeded with `seed + i` (pcgrl_env.py:54-57 per environment).  `seed` may
        also be a sequence of N seeds.  Returns the list of seeds used."""
        if seed is None:
            seed = seeding.create_seed(None, max_bytes=7)
        if np.ndim(seed) == 0:
            seeds = [int(seed) + i for i in range(self.num_envs)]
        else:
            seeds = [int(s) for s in seed]
            if len(seeds) != self.num_envs:
                raise ValueError("need %d seeds, got %d" % (self.num_envs, len(seeds)))
        for s in seeds:
            if s < 0:
                raise ValueError("Seed must be a non-negative integer or omitted, not %r" % (s,))
        self._seeds = seeds
        self._seed_keys = seeding.key_words_for_seeds(seeds)
        self._rng_seeded = False
        if self._handle is not None:
            self._upload_seeds()
        return seeds

    def adjust_param(self, **kwargs):
        """pcgrl_env.py:106-115, including the ordering quirk: max_changes is recomputed only when
        change_percentage is passed, and both limits use the width/height from *before* this call."""
        import copy
        if self._async is not None and self._handle is not None and not self._needs_reset:
            self.flush()           # suspended steps are finished under the parameters they were taken with, as in lockstep
        before = (copy.deepcopy(self._prob.__dict__), copy.deepcopy(self._rep.__dict__), self._max_changes, self._max_iterations)
        if "change_percentage" in kwargs:
            percentage = min(1, max(0, kwargs.get("change_percentage")))
            self._max_changes = max(int(percentage * self._prob._width * self._prob._height), 1)
        self._max_iterations = self._max_changes * self._prob._width * self._prob._height
        self._prob._probs_touched = False
        self._prob.adjust_param(**kwargs)
        self._rep.adjust_param(**kwargs)
        self._update_spaces()
        self._drop_eval_scratch()          # (evaluate()'s scratch environment carries the parameters it was made with)
        if self._handle is not None:
            # A new width / height takes effect on the maps at the next reset() (representation.py:40-45: only reset() makes a map of
            # the new size); until then the allocated maps go on being stepped, with the problem's new size in its formulas -- what
            # the reference does.  Everything else is applied to the live handle.
            stale = (self._prob._width, self._prob._height) != self._alloc_dims
            cfg = self._config(self._alloc_dims if stale else None)
            # a value the library refuses outright (solver_power < 1 or beyond 10^6, a size beyond its limits ...) is reported here, at
            # the call that passed it -- the layout query validates a configuration without touching the handle
            lay = _lib.Layout()
            if self._lib.pcgrl_query_layout(C.byref(self._config()), C.byref(lay)) != 0:
                self._prob.__dict__, self._rep.__dict__, self._max_changes, self._max_iterations = before      # nothing of the call sticks
                self._update_spaces()
                raise ValueError("adjust_param(%s): outside what the library takes (include/pcgrl_hip.h: map side <= 255 -- the wide representation, which "
                                 "has no cursor: any size whose row masks fit a compute unit's LDS --, max_changes <= 65535, search levels of at most "
                                 "16384 bordered cells, 1 <= solver_power <= 10^6; smb: width <= 250, height 3..32, solver_power <= 16383)" %
                                 ", ".join("%s=%r" % kv for kv in kwargs.items()))
            rc = self._lib.pcgrl_configure(self._handle, C.byref(cfg))
            if rc == _lib.PCGRL_EINVAL:
                # a valid configuration the handle cannot take in place: a solver_power beyond what its search arena was sized for, or one
                # that moves the searches to the other kernel family.  The buffers are re-allocated by the next reset(), which has to
                # come first (the reference would let the new solver_power take effect in the middle of the episode) -- also where the
                # handle has not been reset yet (evaluate() binds one before the first reset()): it keeps NONE of this call's parameters
                self._realloc = True
                if not self._needs_reset:
                    self._needs_reset = True
                    self._reset_reason = "adjust_param(%s) needs another search arena" % ", ".join("%s=%r" % kv for kv in kwargs.items())
            else:
                _lib.check(rc, "pcgrl_configure")
            if rc == 0 and self._prob._probs_touched:
                _lib.check(self._lib.pcgrl_set_tile_probs(self._handle, self._stream()), "pcgrl_set_tile_probs")
                self._prob._probs_touched = False
        self._probs_dirty = self._probs_dirty or self._prob._probs_touched

    def _obs(self):
        b = self._bufs
        o = OrderedDict()
        if self._rep.has_pos:
            o["pos"] = b["pos"]
        o["map"] = b["map"]
        # pcgrl_env.py:35,137 keeps a float64 count per cell.  With auto-reset the device counts in 16 bits (a count is at most the
        # episode's changes <= max_changes): the view is int16 while a count cannot pass 32 767 (every configuration of the reference's
        # defaults) -- full operator support in torch -- and uint16 beyond (maps of more than 32 767 cells with a change_percentage to
        # match).  Without auto-reset an episode goes on past done and the counts are unbounded: int32, as the device keeps them
        hm = b["heatmap"]
        o["heatmap"] = hm if (hm.dtype == self._torch.int32 or self._max_changes <= 32767) else hm.view(self._torch.uint16)
        return o

    def reset(self):
        """Reset every environment (pcgrl_env.py:66-76).  Returns the observation dict of tensors."""
        if self._handle is None or (self._prob._width, self._prob._height) != self._alloc_dims or self._realloc:
            self._allocate()
            self._realloc = False
        _lib.check(self._lib.pcgrl_reset(self._handle, self._stream()), "pcgrl_reset")
        self._needs_reset = False
        self._was_reset = True
        self._reset_reason = None
        return self._obs()

    def _as_actions(self, actions):
        torch = self._torch
        aw = self._rep.action_width()
        if not torch.is_tensor(actions):
            actions = torch.as_tensor(np.asarray(actions), device=self.device)
        if actions.device != self.device:
            actions = actions.to(self.device)
        if actions.dtype != torch.int32:
            actions = actions.to(torch.int32)
        actions = actions.reshape(self.num_envs, aw) if aw > 1 else actions.reshape(self.num_envs)
        return actions.contiguous()

    def _pass_actions(self, actions, width=None):
        """The action tensor the library is handed: a contiguous int64 or int32 device tensor of the right size goes through as it
        is (pcgrl_row::actions_i64: the kernels read the low words of int64 values -- what .to(int32) keeps -- so a policy's argmax
        needs no conversion kernel); anything else is converted by _as_actions as ever.  Tells the handle which of the two it is."""
        torch = self._torch
        aw = self._rep.action_width() if width is None else width
        if not (torch.is_tensor(actions) and actions.device == self.device and actions.dtype in (torch.int64, torch.int32)
                and actions.numel() == self.num_envs * aw and actions.is_contiguous()):
            actions = self._as_actions(actions) if width is None else \
                torch.as_tensor(actions).to(device=self.device, dtype=torch.int32).reshape(self.num_envs * aw).contiguous()
        self._apply_row(actions.dtype == torch.int64)
        return actions

    # ---- the rest of a rollout row, written by the step itself (pcgrl_bind_row)
    _ROW_DTYPES = dict(actions_out=("int64",), reward=("float64",), done=("bool", "uint8"), start_in=("bool", "uint8"), start_out=("bool", "uint8"),
                       ep_return=("float64",), ep_length=("int32",), took=("bool", "uint8"), fresh=("bool", "uint8"))

    def bind_rollout_row(self, **columns):
        """From the next step() / step_flat() / tick() on, the step writes these columns of a rollout row itself (include/pcgrl_hip.h
        pcgrl_row; where the step is one fused kernel: no extra launch, elsewhere one small kernel behind it): actions_out int64
        [N] / [N, k] (the actions it was handed), reward float64 [N], done / start_out / took / fresh bool or uint8 [N], start_in
        (read by tick() only), ep_return float64 [N] and ep_length int32 [N] (the finished episodes' return / length, NaN / 0
        elsewhere: need enable_episode_stats()).  Contiguous tensors on this device, kept alive here; call again with other
        tensors for the next row (host work only).  The live views step() returns are written as ever."""
        torch = self._torch
        row = {}
        for name, t in columns.items():
            if name not in self._ROW_DTYPES:
                raise TypeError("bind_rollout_row(): unknown column %r (known: %s)" % (name, ", ".join(_lib.ROW_FIELDS)))
            if t is None:
                continue
            aw = self._rep.action_width()
            shapes = [(self.num_envs,)] if (name != "actions_out" or aw == 1) else [(self.num_envs, aw)]
            if name == "actions_out" and self._rep.name == "wide":
                shapes.append((self.num_envs,))          # step_flat(): the flat indices
            want = "expected a contiguous %s tensor of shape %s on %s" % (" / ".join(self._ROW_DTYPES[name]), " or ".join(str(x) for x in shapes), self.device)
            if not torch.is_tensor(t) or str(t.dtype).replace("torch.", "") not in self._ROW_DTYPES[name]:
                raise ValueError("bind_rollout_row(%s=...): wrong dtype %s: %s" % (name, getattr(t, "dtype", type(t).__name__), want))
            if tuple(t.shape) not in shapes:
                raise ValueError("bind_rollout_row(%s=...): wrong shape %s: %s" % (name, tuple(t.shape), want))
            if not t.is_contiguous():
                raise ValueError("bind_rollout_row(%s=...): not contiguous: %s" % (name, want))
            if t.device != self.device:
                raise ValueError("bind_rollout_row(%s=...): wrong device %s: %s" % (name, t.device, want))
            row[name] = t
        if ("ep_return" in row or "ep_length" in row) and self._episode is None:
            raise RuntimeError("bind_rollout_row(ep_return / ep_length): call enable_episode_stats() first")
        self._set_row(tuple(row[n].data_ptr() if n in row else None for n in _lib.ROW_FIELDS) if row else None, row)

    def _set_row(self, ptrs, keep):
        """bind_rollout_row() without the checks: `ptrs` in _lib.ROW_FIELDS order (None: column not wanted).  RolloutCollector checks
        its [T, N] columns once and walks down them with this."""
        self._row = (ptrs, keep) if ptrs is not None else None

    def unbind_rollout_row(self):
        """No row from now on; the handle is told at once, so that nothing that steps it by another way (MultiGpuPcgrlEnv's one-call
        step) finds a row, or the int64 reading of `actions`, still in place."""
        self._row = None
        self._row_rest()

    def _row_plain(self):
        """The handle takes int32 actions and writes no row: what a caller that hands it raw pointers (pcgrl_step_multi) relies on."""
        return self._row is None and self._row_applied in (None, (None, False))

    def _row_rest(self):
        """Behind every step: without a bound row the handle goes back to plain int32 actions -- the int64 reading of `actions` holds
        for the call that passed an int64 tensor, never for a later one."""
        if self._row is None and self._handle is not None and self._row_applied not in (None, (None, False)):
            self._apply_row(False)

    def _apply_row(self, i64):
        """Tell the handle the row binding in effect for the step that follows (a host call, and only when something changed)."""
        key = (self._row[0] if self._row else None, bool(i64))
        if key == self._row_applied:
            return
        if key[0] is None and not i64:
            _lib.check(self._lib.pcgrl_bind_row(self._handle, None), "pcgrl_bind_row")
        else:
            r = _lib.Row(*(key[0] or (None,) * len(_lib.ROW_FIELDS)), 1 if i64 else 0)
            _lib.check(self._lib.pcgrl_bind_row(self._handle, C.byref(r)), "pcgrl_bind_row")
        self._row_applied = key

    def _step_result(self):
        """Behind the library call of step(), step_flat() and tick(): the strict status check, then the live views they return."""
        if self.strict_actions:
            self.check_status()
        b = self._bufs
        decode = self._prob.decode_rows if self._prob.packed_rows else None
        info = InfoBatch(self._prob.info_keys, b["info"], self._max_iterations, self._max_changes, decode)
        return self._obs(), b["reward"], b["done"].view(self._torch.bool), info

    def step(self, actions):
        """pcgrl_env.py:129-150 for every environment.  actions: int [N] (narrow/turtle) or [N,3]
        (wide: x, y, tile).  Returns (obs, reward f64[N], done bool[N], InfoBatch); tensors are views
        of the live state and are overwritten by the next step."""
        if self._needs_reset:
            raise RuntimeError("reset() must be called before step()" + (": " + self._reset_reason if getattr(self, "_reset_reason", None) else ""))
        a = self._pass_actions(actions)
        self._last_actions = a   # keep the buffer alive until the launches are done
        _lib.check(self._lib.pcgrl_step(self._handle, C.c_void_p(a.data_ptr()), self._stream()), "pcgrl_step")
        self._row_rest()
        return self._step_result()

    def step_flat(self, flat, xyv):
        """ActionMap.step + step() for the wide representation in one call of the library (pcgrl_step_flat): `flat` int32 or int64 [N] device
        tensor of indices into (H, W, tiles), `xyv` int32 [N, 3] device scratch.  Same return value as step()."""
        if self._needs_reset:
            raise RuntimeError("reset() must be called before step()")
        flat = self._pass_actions(flat, width=1)
        self._last_actions = (flat, xyv)
        _lib.check(self._lib.pcgrl_step_flat(self._handle, C.c_void_p(flat.data_ptr()), C.c_void_p(xyv.data_ptr()), self._stream()), "pcgrl_step_flat")
        self._row_rest()
        return self._step_result()

    def rollout(self, actions, want_info=True, out=None):
        """`T` consecutive steps on a tape of actions: int tensor [T, N] (narrow, turtle), [T, N, 3] (wide), [T, N, 2] /
        [T, N, 9] (cast / multi).  Returns (reward f64 [T, N], done bool [T, N], info) with `info` an InfoBatch over the
        [T*N, 10] table (rows in step-major order) or None.  The environments end up exactly where T calls of step()
        would leave them; where the whole step is one kernel (binary maps of at most 16 rows) the tape is ONE launch.
        `out`: optional preallocated (reward f64 [T,N], done u8 [T,N], info i32 [T,N,10] or None) on this device."""
        if self._needs_reset:
            raise RuntimeError("reset() must be called before rollout()")
        torch = self._torch
        a = torch.as_tensor(actions, device=self.device).to(torch.int32).contiguous()
        T = int(a.shape[0])
        aw = self._rep.action_width()
        if a.numel() != T * self.num_envs * aw:
            raise ValueError("actions must have shape [T, %d%s], got %s" % (self.num_envs, "" if aw == 1 else ", %d" % aw, tuple(a.shape)))
        if out is not None:
            rew, done, info = out
            want_info = info is not None
            for ten, dt, shape in ((rew, torch.float64, (T, self.num_envs)), (done, torch.uint8, (T, self.num_envs)),
                                   (info, torch.int32, (T, self.num_envs, 10))):
                if ten is not None and (ten.dtype != dt or tuple(ten.shape) != shape or not ten.is_contiguous() or ten.device != self.device):
                    raise ValueError("rollout(out=...): expected a contiguous %s tensor of shape %s on %s" % (dt, shape, self.device))
        else:
            rew = torch.empty((T, self.num_envs), dtype=torch.float64, device=self.device)
            done = torch.empty((T, self.num_envs), dtype=torch.uint8, device=self.device)
            info = torch.empty((T, self.num_envs, 10), dtype=torch.int32, device=self.device) if want_info else None
        self._last_actions = a
        _lib.check(self._lib.pcgrl_rollout(self._handle, C.c_void_p(a.data_ptr()), T, C.c_void_p(rew.data_ptr()),
                                           C.c_void_p(done.data_ptr()), C.c_void_p(info.data_ptr()) if want_info else None,
                                           self._stream()), "pcgrl_rollout")
        if self.strict_actions:
            self.check_status()
        ib = None
        if want_info:
            decode = self._prob.decode_rows if self._prob.packed_rows else None
            ib = InfoBatch(self._prob.info_keys, info.view(T * self.num_envs, 10), self._max_iterations, self._max_changes, decode)
        return rew, done.view(torch.bool), ib

    # ---- the wrapped observation (wrappers.py:215-248), written by the step itself
    def bind_observation(self, out_h, out_w, centered, pad_value, onehot, out=None, incremental=True):
        """From now on every reset() / step() / rollout() / set_maps() leaves the image the reference's composite wrappers
        would produce -- uint8 [N, out_h, out_w, D], D = 1 or the number of tiles (one-hot); centred on the cursor and padded
        with `pad_value`, or the map from its origin -- in the returned tensor (`out`, or a new one).  Where the step is one
        fused kernel it writes the image from its on-chip copy of the state; no extra launch.  `incremental` (default): the
        tensor is the environment's to maintain -- do not write into it -- so that a step may update it in place where that
        is cheaper (a window that does not follow a cursor changes in one cell per step); after set_observation_target() the
        next step writes a full image into the new tensor."""
        torch = self._torch
        depth = self.get_num_tiles() if onehot else 1
        shape = (self.num_envs, int(out_h), int(out_w), depth)
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=self.device)
        self._check_obs_target(out, shape)
        self._obs_spec = (out, int(out_h), int(out_w), int(bool(centered)), int(pad_value), int(bool(onehot)), int(bool(incremental)))
        self._apply_observation()
        return out

    def _check_obs_target(self, out, shape):
        torch = self._torch
        if out.dtype != torch.uint8 or tuple(out.shape) != tuple(shape) or not out.is_contiguous() or out.device != self.device or out.data_ptr() % 16:
            raise ValueError("observation target: expected a contiguous, 16-byte aligned uint8 tensor of shape %s on %s" % (tuple(shape), self.device))

    def set_observation_target(self, out):
        """Redirect the bound observation to another tensor of the same shape (e.g. row t+1 of a rollout buffer)."""
        old = self._obs_spec
        if old is None:
            raise RuntimeError("call bind_observation() first")
        self._check_obs_target(out, old[0].shape)
        self._obs_spec = (out,) + old[1:]
        self._apply_observation()

    def unbind_observation(self):
        self._obs_spec = None
        if self._handle is not None:
            _lib.check(self._lib.pcgrl_bind_observation(self._handle, None, 0, 0, 0, 0, 0, 0), "pcgrl_bind_observation")

    def _apply_observation(self):
        if self._obs_spec is None or self._handle is None:
            return
        out, h, w, centered, pad, onehot, inc = self._obs_spec
        _lib.check(self._lib.pcgrl_bind_observation(self._handle, C.c_void_p(out.data_ptr()), h, w, centered, pad, onehot, inc), "pcgrl_bind_observation")

    # gym.vector-style split call
    def step_async(self, actions):
        self._pending = self.step(actions)

    def step_wait(self):
        return self._pending

    # ---- asynchronous stepping of the search problems (pcgrl_step_async, csrc/kernels_search_async.h)
    def enable_async(self, nslots=1024):
        """Prepare tick(): room for `nslots` suspended searches (about 0.46 MB each at solver_power 5000).  Returns False when
        this configuration has no asynchronous form (binary, zelda, smb; levels or solver_power beyond the compact searches) --
        tick() is then step() with nothing ever pending."""
        self._async_nslots = int(nslots)
        if self._handle is None:
            self._allocate()
        elif self._async is None:
            self._bind_async()
        return self._async is not None

    def _bind_async(self):
        torch = self._torch
        cfg = self._config(self._alloc_dims)
        need = int(self._lib.pcgrl_async_bytes(C.byref(cfg), self._async_nslots))
        if need == 0:
            self._async = None
            return
        arena = torch.empty((need,), dtype=torch.uint8, device=self.device)          # (zeroed by the call)
        rc = self._lib.pcgrl_bind_async(self._handle, C.c_void_p(arena.data_ptr()), need, self._async_nslots, self._stream())
        if rc == _lib.PCGRL_EINVAL:
            # the handle's search arena was cut for another solver_power than the one in effect (an in-place adjust_param(solver_power=
            # smaller)): no asynchronous form on THIS allocation -- tick() steps in lockstep, nothing ever pending -- and the next
            # reset() re-allocates, after which the slots fit
            self._async = None
            self._realloc = True
            return
        _lib.check(rc, "pcgrl_bind_async")
        n = self.num_envs
        off = (n + 255) // 256 * 256
        self._async = dict(arena=arena, pending=arena[:n], counters=arena[off:off + 64 + 16 * 64].view(torch.int64))

    def tick(self, actions, pop_budget=256):
        """One tick of asynchronous stepping (include/pcgrl_hip.h pcgrl_step_async): every environment whose previous step is
        complete takes its action and steps; every search gets at most `pop_budget` pops, an environment whose search is not
        finished by then stays *pending* -- it ignores the actions of the following ticks until one of them completes its step.
        Returns (obs, reward, done, info, pending): the usual live views plus pending uint8 [N] (a live view too) -- where it is
        0 the outputs are those of the environment's last taken action and it takes the next one; elsewhere (1: a search is
        suspended, 2: its search ended the episode and the next tick resets it) the environment's rows are to be ignored.  Per environment the sequence of (taken action -> outputs) is bitwise that of
        step().  step() / rollout() / adjust_param() finish what is pending first (flush()); reset() and set_maps() drop it (every map is
        replaced: what was in flight is void)."""
        if self._needs_reset:
            raise RuntimeError("reset() must be called before tick()")
        if self._async is None:
            if self._async_nslots == 0:
                self.enable_async()
            if self._async is None:            # no asynchronous form: a lockstep step, nothing pending
                o, r, d, i = self.step(actions)
                if getattr(self, "_never_pending", None) is None:
                    self._never_pending = self._torch.zeros(self.num_envs, dtype=self._torch.uint8, device=self.device)
                return o, r, d, i, self._never_pending
        a = self._pass_actions(actions)
        self._last_actions = a
        _lib.check(self._lib.pcgrl_step_async(self._handle, C.c_void_p(a.data_ptr()), int(pop_budget), self._stream()), "pcgrl_step_async")
        self._row_rest()
        return self._step_result() + (self._async["pending"],)

    def async_idle(self):
        """bool [N] device tensor (a new one, not a view): the environments that take their action at the next tick -- those with no
        step in flight.  Read from the live pending state, so it is right after anything that finished or dropped pending steps
        in between (adjust_param() / step() / rollout() flush them, reset() / set_maps() drop them)."""
        if self._async is None:
            return self._torch.ones(self.num_envs, dtype=self._torch.bool, device=self.device)
        return self._async["pending"] == 0

    def flush(self):
        """Finish every pending step (searches with an unbounded budget)."""
        if self._handle is not None:
            _lib.check(self._lib.pcgrl_async_flush(self._handle, self._stream()), "pcgrl_async_flush")

    def async_counters(self):
        """{actions taken, searches suspended, jobs finished from a slot, slot overflows, pops of the resumable searches} since
        enable_async() (synchronises)."""
        if self._async is None:
            return None
        c = self._async["counters"].cpu().numpy()
        return dict(consumed=int(c[8::8].sum()), suspended=int(c[1]), late=int(c[2]), overflow=int(c[3]), pops=int(c[4]))

    # ---- episode statistics (stable-baselines Monitor as wrapped around the reference env, utils.py:13-29)
    def enable_episode_stats(self, enable=True):
        """Keep per-environment episode return/length on the device (updated by the step kernels).  After a step,
        `episode_stats()` gives the values of the episodes that just ended (where done is set)."""
        if enable:
            if self._handle is None:
                self._allocate()
            if self._episode is None:
                torch, n, dev = self._torch, self.num_envs, self.device
                self._episode = OrderedDict(
                    ep_return=torch.zeros(n, dtype=torch.float64, device=dev), ep_length=torch.zeros(n, dtype=torch.int32, device=dev),
                    last_return=torch.zeros(n, dtype=torch.float64, device=dev), last_length=torch.zeros(n, dtype=torch.int32, device=dev))
                self._bind_episode_stats(zero=True)
        elif self._episode is not None:
            self._episode = None
            if self._handle is not None:
                _lib.check(self._lib.pcgrl_bind_episode_stats(self._handle, None, None, None, None, self._stream()), "pcgrl_bind_episode_stats")

    def _bind_episode_stats(self, zero=False):
        e = self._episode
        keep = None if zero else {k: v.clone() for k, v in e.items()}
        _lib.check(self._lib.pcgrl_bind_episode_stats(self._handle, e["ep_return"].data_ptr(), e["ep_length"].data_ptr(),
                                                     e["last_return"].data_ptr(), e["last_length"].data_ptr(), self._stream()),
                   "pcgrl_bind_episode_stats")
        if keep is not None:           # the ABI call zeroes the buffers
            for k, v in keep.items():
                e[k].copy_(v)

    def episode_stats(self):
        """-> dict of device tensors: running `ep_return`/`ep_length`, and `last_return`/`last_length` of the most
        recently finished episode of every environment (valid where the last step returned done)."""
        if self._episode is None:
            raise RuntimeError("call enable_episode_stats() first")
        return self._episode

    def set_maps(self, maps):
        """Overwrite every map (uint8 [N,H,W]) and recompute the current stats on the device."""
        if self._needs_reset:
            raise RuntimeError("reset() must be called before set_maps()")
        torch = self._torch
        m = torch.as_tensor(maps, device=self.device).to(torch.uint8).contiguous()
        assert tuple(m.shape) == tuple(self._bufs["map"].shape)
        self._last_maps = m
        _lib.check(self._lib.pcgrl_set_maps(self._handle, C.c_void_p(m.data_ptr()), self._stream()), "pcgrl_set_maps")

    # ---- Problem.get_stats / get_reward / get_episode_over on any level (pcgrl_get_stats, pcgrl_get_reward)
    def evaluate(self, maps, ref=None, chunk=65536):
        """Score `maps` -- array-like uint8 [M, H, W] on any device, M independent of num_envs -- with this environment's problem and
        the parameters in force (adjust_param applies): Problem.get_stats of every map, and with `ref` (int32 [M, 8] rows, or [8]
        for all: an earlier evaluate().rows or this environment's own stats / start-stats rows) Problem.get_reward(new=maps, old=ref)
        and Problem.get_episode_over(new=maps, start=ref).  Returns an Evaluation (rows, stats, reward, over).  A pure function: the
        running episodes, their random streams and pending asynchronous searches are not touched, nothing needs a reset() first, the
        input is not modified (a tile id >= get_num_tiles() is clamped on the way and reported by check_status()), and nothing is
        waited for.  Where the library has no one-call form (smb, maps beyond 64 x 64, the general searches) the maps go, `chunk` at a
        time, through a private scratch environment's set_maps() instead -- and so they do while an adjust_param() that the handle
        could not take in place (a larger solver_power: another search arena) waits for the next reset(): the handle still carries
        the episodes and the old parameters, the scratch environment scores -- rewards included -- with the new ones.
        The calls on one environment share a cached workspace: issue them on one stream (the current stream of the first call),
        or synchronise between calls made on different streams."""
        torch = self._torch
        self._scoring_handle()
        stale = self._realloc              # the handle keeps its episodes and, until the next reset(), the parameters before the refused change
        m = self._as_maps("evaluate", maps)
        M = int(m.shape[0])
        rows = torch.empty((M, 8), dtype=torch.int32, device=self.device)
        cfg = self._config(self._alloc_dims)
        need = 0 if stale else int(self._lib.pcgrl_get_stats_bytes(C.byref(cfg), M))
        if need:
            _lib.check(self._lib.pcgrl_get_stats(self._handle, C.c_void_p(m.data_ptr()), M, C.c_void_p(rows.data_ptr()),
                                                 *self._workspace(need), self._stream()), "pcgrl_get_stats")
        else:
            self._evaluate_by_set_maps(m, rows, int(chunk))
        reward = over = None
        if ref is not None:
            r = ref if torch.is_tensor(ref) else torch.as_tensor(np.asarray(ref))
            if r.dtype not in (torch.int32, torch.int64) or tuple(r.shape) not in ((8,), (M, 8)):
                raise ValueError("evaluate(): ref must be int32 rows of shape [%d, 8] or [8], got %s %s" % (M, r.dtype, tuple(r.shape)))
            r = r.to(device=self.device, dtype=torch.int32)
            r = (r.expand(M, 8) if r.dim() == 1 else r).contiguous()
            reward = torch.empty((M,), dtype=torch.float64, device=self.device)
            over = torch.empty((M,), dtype=torch.uint8, device=self.device)
            scorer = self._eval_scratch._handle if stale else self._handle
            _lib.check(self._lib.pcgrl_get_reward(scorer, C.c_void_p(rows.data_ptr()), C.c_void_p(r.data_ptr()), M,
                                                  C.c_void_p(reward.data_ptr()), C.c_void_p(over.data_ptr()), self._stream()), "pcgrl_get_reward")
            over = over.view(torch.bool)
        return Evaluation(rows, self._prob.decode_rows(rows), reward, over)

    # ---- what evaluate(), solve(), playthrough(), playthrough_smb() and paths() share
    def _scoring_handle(self):
        """A handle that can take the parameters in force: a new one where there is none yet, or one that was only ever bound for
        scoring and cannot take them (bound, not reset: step() and set_maps() still ask for reset())."""
        dims = (self._prob._width, self._prob._height)
        if self._handle is None or (not self._was_reset and (self._realloc or dims != self._alloc_dims)):
            self._allocate()
            self._realloc = False

    def _as_maps(self, who, maps):
        """`maps` (array-like [M, H, W] on any device) as a contiguous uint8 tensor on this environment's device."""
        torch = self._torch
        m = maps if torch.is_tensor(maps) else torch.as_tensor(np.asarray(maps))
        if m.dim() != 3:
            raise ValueError("%s(): maps must be [M, H, W], got shape %s" % (who, tuple(m.shape)))
        w, h = self._alloc_dims
        if tuple(m.shape[1:]) != (h, w) or m.shape[0] < 1:
            raise ValueError("%s(): maps of shape %s for an environment of %d rows x %d columns (at least one map)" % (who, tuple(m.shape), h, w))
        return m.to(device=self.device, dtype=torch.uint8).contiguous()

    def _workspace(self, need):
        """The cached workspace, grown to `need` bytes: the (pointer, size) pair a library call takes."""
        if self._eval_work is None or self._eval_work.numel() < need:
            self._eval_work = self._torch.empty((need,), dtype=self._torch.uint8, device=self.device)
        return C.c_void_p(self._eval_work.data_ptr()), self._eval_work.numel()

    def _readout(self, who, verb, bytes_fn, no_form_message, maps, max_len, default_len):
        """solve(), playthrough(), playthrough_smb(), paths() and connectivity() behind their problem checks, up to their outputs: the
        levels `m` ([M, H, W]: `maps`, or (None) the handle's own map buffer), `max_len` (None: `default_len(w, h)`) and the workspace
        `bytes_fn` asks for, as (m, M, max_len, work).  `no_form_message(w, h)`: the text where `bytes_fn` gives 0.  default_len None:
        the call has no rows of a length -- `bytes_fn` takes the configuration and M, max_len stays None."""
        if maps is None:
            if self._handle is None or not self._was_reset or self._needs_reset:
                raise RuntimeError("%s() without maps reads the environment's current levels: call reset() first" % who)
        self._scoring_handle()
        if self._realloc:
            raise NotImplementedError("%s(): an adjust_param() that this handle could not take in place waits for the next reset(); "
                                      "the handle still %s with the old parameters" % (who, verb))
        w, h = self._alloc_dims
        m = self._bufs["map"] if maps is None else self._as_maps(who, maps)
        M = int(m.shape[0])
        if default_len is not None:
            max_len = default_len(w, h) if max_len is None else int(max_len)
            if max_len < 1:
                raise ValueError("%s(): max_len must be at least 1, got %d" % (who, max_len))
        cfg = self._config(self._alloc_dims)
        need = int(getattr(self._lib, bytes_fn)(C.byref(cfg), M, *(() if default_len is None else (max_len,))))
        if not need:
            raise NotImplementedError(no_form_message(w, h))
        return m, M, max_len, self._workspace(need)

    def _planner_moves(self, who, fn, bytes_fn, result_cls, no_form_message, maps, max_len):
        """solve(), playthrough() and playthrough_smb() behind their problem checks: library call `fn` with the workspace `bytes_fn`
        asks for, on `maps` or (None) the handle's own map buffer.  `no_form_message(w, h, power)`: the text where `bytes_fn` gives 0."""
        torch = self._torch
        power = int(self._prob._solver_power)
        m, M, max_len, work = self._readout(who, "plans", bytes_fn, lambda w, h: no_form_message(w, h, power), maps, max_len, lambda w, h: min(power, 255))
        moves = torch.empty((M, max_len), dtype=torch.int8, device=self.device)
        length = torch.empty((M,), dtype=torch.int32, device=self.device)
        agent = torch.empty((M,), dtype=torch.int8, device=self.device)
        rows = torch.empty((M, 8), dtype=torch.int32, device=self.device)
        _lib.check(getattr(self._lib, fn)(self._handle, C.c_void_p(m.data_ptr()), M, max_len, C.c_void_p(moves.data_ptr()),
                                          C.c_void_p(length.data_ptr()), C.c_void_p(agent.data_ptr()), C.c_void_p(rows.data_ptr()),
                                          *work, self._stream()), fn)
        return result_cls(moves, length, agent, rows, self._prob.decode_rows(rows))

    # ---- SokobanProblem.get_stats(map)["solution"] on any level (pcgrl_get_solution)
    def solve(self, maps=None, max_len=None):
        """The planner's moves for `maps` -- array-like uint8 [M, H, W] as for evaluate(); None: this environment's current levels
        (after a reset(); the handle's own map buffer is read in place) -- with the parameters in force: what the reference returns
        as get_stats(map)["solution"].  `max_len`: columns of the move rows, by default min(solver_power, 255).  Returns Solutions
        (moves, length, agent, rows, stats), all on the device.  A pure function like evaluate(): episodes, random streams and
        pending asynchronous searches are not touched, a tile id >= get_num_tiles() is clamped on the way and reported by
        check_status(), nothing is waited for; the workspace is evaluate()'s (the same one-stream rule).  NotImplementedError where
        the library has no one-call form: there is no scratch-environment route for the moves."""
        if self._prob.name != "sokoban":
            raise NotImplementedError("solve(): only sokoban's get_stats returns its planner's moves (problem %r keeps at most their number%s)"
                                      % (self._prob.name, "; playthrough() returns the play behind its statistics" if self._prob.name in ("mdungeon", "ddave") else ""))
        return self._planner_moves("solve", "pcgrl_get_solution", "pcgrl_get_solution_bytes", Solutions, lambda w, h, power: (
            "solve(): no one-call form for this configuration (levels of %d x %d = %d bordered cells, solver_power %d): "
            "the traced searches are the ones that run in LDS -- at most 256 bordered cells and solver_power <= 5000"
            % (h + 2, w + 2, (h + 2) * (w + 2), power)), maps, max_len)

    # ---- the play that _run_game scores, mdungeon and ddave (pcgrl_get_playthrough)
    def playthrough(self, maps=None, max_len=None):
        """The play behind the planner's statistics for `maps` -- array-like uint8 [M, H, W] as for evaluate(); None: this
        environment's current levels (after a reset(); the handle's own map buffer is read in place) -- with the parameters in
        force: the moves of the first agent of _run_game that wins, or, when none wins, the moves that lead to the BFS agent's best
        node -- the state `col-*` / `num-jumps` / `dist-win` describe.  `max_len`: columns of the move rows, by default
        min(solver_power, 255).  Returns Playthroughs (moves, length, agent, rows, stats), all on the device.  `length` is not
        `sol-length`: with agent == -1 the row holds the BFS agent's best node's moves while stats["sol-length"] is 0.
        A pure function like evaluate(): episodes, random streams and pending asynchronous searches are not touched, a tile id >=
        get_num_tiles() is clamped on the way and reported by check_status(), nothing is waited for; the workspace is evaluate()'s
        (the same one-stream rule).  NotImplementedError for the other problems (sokoban: solve()) and where the library has no
        one-call form: there is no scratch-environment route for the moves."""
        if self._prob.name not in ("mdungeon", "ddave"):
            raise NotImplementedError("playthrough(): the plays of mdungeon and ddave only, not problem %r%s"
                                      % (self._prob.name, " (solve() returns sokoban's solution)" if self._prob.name == "sokoban" else
                                         " (playthrough_smb() returns smb's play)" if self._prob.name == "smb" else ""))
        return self._planner_moves("playthrough", "pcgrl_get_playthrough", "pcgrl_get_playthrough_bytes", Playthroughs, lambda w, h, power: (
            "playthrough(): no one-call form for this configuration (levels of %d x %d = %d bordered cells, solver_power %d): "
            "the traced searches are the ones that run in LDS -- at most 256 bordered cells and solver_power <= 5000"
            % (h + 2, w + 2, (h + 2) * (w + 2), power)), maps, max_len)

    # ---- the play that SMBProblem._run_game scores (pcgrl_get_smb_play)
    def playthrough_smb(self, maps=None, max_len=None):
        """The play behind smb's `jumps`, `jumps-dist` and `dist-win` for `maps` -- array-like uint8 [M, H, W] as for evaluate(); None:
        this environment's current levels (after a reset(); the handle's own map buffer is read in place) -- with the parameters in
        force: the moves of A*(balance 1) if it wins, else of A*(balance 0) -- to its winning node, or, when nobody wins, to its best
        node, the state `dist-win` is measured from.  Moves are 0 stay, 1 right, 2 jump, 3 right + jump.  `max_len`: columns of the move
        rows, by default min(solver_power, 255).  Returns Playthroughs (moves, length, agent, rows, stats), all on the device; agent is
        0, 1 or -1.  A pure function like evaluate(): episodes, random streams and the kept play-throughs of the step are not touched,
        a tile id >= get_num_tiles() is clamped on the way and reported by check_status(), nothing is waited for; the workspace is
        evaluate()'s (the same one-stream rule).  solver_power is smb's attribute (prob._solver_power, then adjust_param()).
        NotImplementedError for the other problems (mdungeon, ddave: playthrough(); sokoban: solve())."""
        if self._prob.name != "smb":
            raise NotImplementedError("playthrough_smb(): smb's play only, not problem %r%s"
                                      % (self._prob.name, " (solve() returns sokoban's solution)" if self._prob.name == "sokoban" else
                                         " (playthrough() returns its play)" if self._prob.name in ("mdungeon", "ddave") else ""))
        return self._planner_moves("playthrough_smb", "pcgrl_get_smb_play", "pcgrl_get_smb_play_bytes", Playthroughs, lambda w, h, power: (
            "playthrough_smb(): the library does not take this configuration (width %d, height %d, solver_power %d)" % (w, h, power)), maps, max_len)

    # ---- the paths behind path-length / nearest-enemy, binary and zelda (pcgrl_get_paths)
    PATH_LEGS = {"binary": ("longest",), "zelda": ("key", "door", "enemy")}

    def paths(self, maps=None, max_len=None):
        """The cells of the paths that the statistics measure, for `maps` -- array-like uint8 [M, H, W] as for evaluate(); None: this
        environment's current levels (after a reset(); the handle's own map buffer is read in place) -- with the parameters in force.
        binary: one leg, "longest" -- the longest shortest path `path-length` is the length of (helper.py:250-264).  zelda: three --
        "key" (player -> key) and "door" (key -> door), whose lengths add up to `path-length`, and "enemy" (player -> the nearest
        enemy, `nearest-enemy` long), zelda_prob.py:91-110.  The rule that makes each leg unique is in include/pcgrl_hip.h
        (pcgrl_get_paths).  `max_len`: columns of a leg's row, by default H * W, which holds every leg; a smaller one saves memory at
        large M (M * legs * max_len * 2 bytes) and leaves prefixes (`truncated`).  Returns Paths (cells, length, rows, stats), all on
        the device.  A pure function like evaluate(): episodes, random streams and pending asynchronous searches are not touched, a
        tile id >= get_num_tiles() is clamped on the way and reported by check_status(), nothing is waited for; the workspace is
        evaluate()'s (the same one-stream rule).  NotImplementedError for the other problems (their routes are plays: solve(),
        playthrough(), playthrough_smb()) and where the library has no one-call form (maps beyond 64 x 64): there is no
        scratch-environment route for the cells."""
        name = self._prob.name
        if name not in self.PATH_LEGS:
            raise NotImplementedError("paths(): the paths of binary and zelda only, not problem %r (%s)" % (name, {
                "sokoban": "solve() returns sokoban's solution", "smb": "playthrough_smb() returns smb's play"}.get(name, "playthrough() returns its play")))
        torch = self._torch
        m, M, max_len, work = self._readout("paths", "scores", "pcgrl_get_paths_bytes", lambda w, h: (
            "paths(): no one-call form for this configuration (maps of %d rows x %d columns): "
            "the row-bitboard kernels take maps up to 64 x 64" % (h, w)), maps, max_len, lambda w, h: h * w)
        legs = self.PATH_LEGS[name]
        cells = torch.empty((M, len(legs), max_len), dtype=torch.int16, device=self.device)
        length = torch.empty((M, len(legs)), dtype=torch.int32, device=self.device)
        rows = torch.empty((M, 8), dtype=torch.int32, device=self.device)
        _lib.check(self._lib.pcgrl_get_paths(self._handle, C.c_void_p(m.data_ptr()), M, max_len, C.c_void_p(cells.data_ptr()),
                                             C.c_void_p(length.data_ptr()), C.c_void_p(rows.data_ptr()),
                                             *work, self._stream()), "pcgrl_get_paths")
        return Paths(cells, length, rows, self._prob.decode_rows(rows), legs, self._alloc_dims[0])

    # ---- helper.py for any tile set: regions, longest path, labels, distance map, reachable tiles (pcgrl_tile_graph)
    def connectivity(self, maps=None, passable=(), source=None, reach=None, labels=False, dist=False, scalars=True):
        """gym_pcgrl/envs/helper.py (helper.py:170-296) on the device for `maps` -- array-like uint8 [M, H, W] as for evaluate(), of any
        tile values 0..31 whatever this environment's problem; None: this environment's current levels (after a reset(); the handle's
        own map buffer is read in place).  `passable`: the tiles one can walk on -- ints, or this problem's tile names, one or a list.
        Returns a Connectivity (regions, longest, labels, dist, reach, source), None where not asked for:
        `regions` / `longest` (scalars=True) calc_num_regions / calc_longest_path; `labels` (labels=True) calc_num_regions' color_map;
        `dist` (dist=True) run_dikjstra's map from the source; `reach` (`reach`: tiles like `passable`) calc_num_reachable_tile;
        `source` (with a `source`) the cell that was used.
        `source`: None; an int cell y * W + x (-1: none); a tensor / array [M] of cells; a tuple (x, y) of ints or tensors [M]; or a
        tile name, or a LIST of tiles: the first cell in row-major order that holds one of them.  Host ints are range-checked; a cell
        of a tensor outside the map counts as none and is reported by check_status() like an action outside the action space.
        A tile argument is a set, not the reference's list: the rule, and where `longest` and the label numbering deviate from a
        reference call with several passable values, is in include/pcgrl_hip.h (pcgrl_tile_graph) and gym_pcgrl_amd/helper.py.
        A pure function like evaluate(): episodes, random streams and pending asynchronous searches are not touched, a byte >= 32 is
        in no set and reported by check_status(), nothing is waited for; the workspace is evaluate()'s (the same one-stream rule).
        NotImplementedError where the library has no form: maps beyond 64 x 64, smb."""
        from ..helper import source_arg, tile_set
        torch = self._torch
        names = self._prob.get_tile_types()
        pass_set = tile_set(passable, names, "passable")
        reach_set = tile_set(reach, names, "reach")
        m, M, _, work = self._readout("connectivity", "reads levels", "pcgrl_tile_graph_bytes", lambda w, h: (
            "connectivity(): no form for this configuration (problem %r, maps of %d rows x %d columns): "
            "the row-bitboard kernel takes maps up to 64 x 64 and not smb's" % (self._prob.name, h, w)), maps, None, None)
        w, h = self._alloc_dims
        kind, src = source_arg(source, w, h, names)
        if (dist or reach is not None) and kind == "none":
            raise ValueError("connectivity(): dist and reach are measured from a source: pass source=")
        if not (scalars or labels or dist or reach is not None or kind != "none"):
            raise ValueError("connectivity(): nothing was asked for")
        cells = None
        if kind == "cells":
            c = src if torch.is_tensor(src) else torch.as_tensor(np.asarray(src))
            if c.dtype not in (torch.int32, torch.int64, torch.int16, torch.int8, torch.uint8) or c.dim() > 1 or (c.dim() == 1 and c.shape[0] != M):
                raise ValueError("connectivity(): source cells must be integers, one or [%d], got %s %s" % (M, c.dtype, tuple(c.shape)))
            cells = c.to(device=self.device, dtype=torch.int32).expand(M).contiguous()
        new = lambda want, shape, dtype: torch.empty(shape, dtype=dtype, device=self.device) if want else None
        out = Connectivity(new(scalars, (M,), torch.int32), new(scalars, (M,), torch.int32), new(labels, (M, h, w), torch.int16),
                           new(dist, (M, h, w), torch.int16), new(reach is not None, (M,), torch.int32), new(kind != "none", (M,), torch.int32))
        ptr = lambda t: t.data_ptr() if t is not None else None
        d = _lib.TileGraphDesc(ptr(m), M, pass_set, src if kind == "tiles" else 0, reach_set, ptr(cells), ptr(out.regions), ptr(out.longest),
                               ptr(out.labels), ptr(out.dist), ptr(out.reach), ptr(out.source))
        _lib.check(self._lib.pcgrl_tile_graph(self._handle, C.byref(d), *work, self._stream()), "pcgrl_tile_graph")
        return out

    # ---- the local half of helper.py for any tile set: floor distance, grouping, changes, tile counts (pcgrl_tile_local)
    def tile_stats(self, maps=None, counts=False, floor=None, floor_from=None, floor_map=False, group=None, offsets=(), group_min=0, group_max=None,
                   group_map=False, changes=False):
        """gym_pcgrl/envs/helper.py's local helpers (helper.py:37-137) on the device for `maps` -- array-like uint8 [M, H, W] as for
        evaluate(), of any tile values 0..31 whatever this environment's problem; None: this environment's current levels (after a
        reset(); the handle's own map buffer is read in place).  Tiles are ints or this problem's tile names, one or a list.
        Returns a TileStats (counts, floor_dist, floor_map, grouping, group_map, changes), None where not asked for:
        `counts` (counts=True) the cells of every tile 0..31; `floor_dist` (`floor_from` and `floor`) get_floor_dist(map, floor_from,
        floor); `floor_map` (floor_map=True, with `floor`) _calc_dist_floor of every cell; `grouping` (`group`, with `offsets` = relLocs,
        (dx, dy) each, at most 16, and group_min .. group_max, by default 0 .. len(offsets)) get_type_grouping; `group_map`
        (group_map=True, with `group`) _calc_group_value of every cell; `changes` (changes=True) get_changes horizontal, vertical.
        The reference only tests `in types`: a tile set is the reference exactly.
        A pure function like evaluate(): episodes, random streams and pending asynchronous searches are not touched, a byte >= 32 is
        in no set and reported by check_status(), nothing is waited for; the workspace is evaluate()'s (the same one-stream rule).
        There is a form for every configuration: smb and maps beyond 64 x 64 included."""
        from ..helper import offsets_arg, tile_set
        torch = self._torch
        names = self._prob.get_tile_types()
        if floor_from is not None and floor is None:
            raise ValueError("tile_stats(): floor_from needs floor: the distance is measured to the floor tiles")
        if floor_map and floor is None:
            raise ValueError("tile_stats(): floor_map needs floor")
        if group_map and group is None:
            raise ValueError("tile_stats(): group_map needs group")
        want_fd, want_gr = floor_from is not None, group is not None
        if not (counts or want_fd or floor_map or want_gr or group_map or changes):
            raise ValueError("tile_stats(): nothing was asked for")
        from_set, floor_set, group_set = tile_set(floor_from, names, "floor_from"), tile_set(floor, names, "floor"), tile_set(group, names, "group")
        offs = offsets_arg(offsets) if want_gr else []
        group_max = len(offs) if group_max is None else int(group_max)
        m, M, _, work = self._readout("tile_stats", "reads levels", "pcgrl_tile_local_bytes", lambda w, h: (
            "tile_stats(): the library does not take this configuration (problem %r, maps of %d rows x %d columns)" % (self._prob.name, h, w)), maps, None, None)
        w, h = self._alloc_dims
        new = lambda want, shape, dtype: torch.empty(shape, dtype=dtype, device=self.device) if want else None
        out = TileStats(new(counts, (M, 32), torch.int32), new(want_fd, (M,), torch.int32), new(floor_map, (M, h, w), torch.int16),
                        new(want_gr, (M,), torch.int32), new(group_map, (M, h, w), torch.int8), new(changes, (M, 2), torch.int32))
        ptr = lambda t: t.data_ptr() if t is not None else None
        clip = lambda v: max(-2 ** 31, min(2 ** 31 - 1, int(v)))
        d = _lib.TileLocalDesc(ptr(m), M, from_set, floor_set, group_set, clip(group_min), clip(group_max), len(offs))
        for k, (dx, dy) in enumerate(offs):
            d.offsets[k][0], d.offsets[k][1] = dx, dy
        d.counts_out, d.floor_dist_out, d.floor_map_out = ptr(out.counts), ptr(out.floor_dist), ptr(out.floor_map)
        d.grouping_out, d.group_map_out, d.changes_out = ptr(out.grouping), ptr(out.group_map), ptr(out.changes)
        _lib.check(self._lib.pcgrl_tile_local(self._handle, C.byref(d), *work, self._stream()), "pcgrl_tile_local")
        return out

    # ---- every one-cell change of a level: rows, reward and episode end (pcgrl_get_changes)
    def changes(self, maps=None, cells=None, start=None, rows=True, chunk=65536):
        """What would changing one cell do?  For `maps` -- array-like uint8 [M, H, W] as for evaluate(); None: this environment's current
        levels (after a reset(); the handle's own map buffer is read in place) -- and per level K cells, entry [m, k, t] is level m with
        cell k set to tile t, for each of the problem's T tiles, scored with the parameters in force:
        `rows` int32 [M, K, T, 8] (rows=False: None, and nothing that large is allocated) the statistics row of that level, `reward`
        float64 [M, K, T] Problem.get_reward(new=that row, old=the level's own row) -- what the step that makes the change would pay --
        and `over` bool [M, K, T] Problem.get_episode_over(new=that row, start).  The entry of the tile a cell already holds is the
        level's own row with reward 0.  Returns Changes (rows, reward, over, base_rows [M, 8], cells int32 [M, K], stats = base_rows
        decoded), all on the device; nothing is waited for.
        `cells`: [M, K] or [K] (the same for every level), a cell being y * W + x, repeats allowed; None: every cell in row-major
        order.  A host array is range-checked (ValueError); a device tensor is not: a cell outside the map is clamped into it and
        reported by check_status() like an action outside the action space.  "cursor" (maps=None; not the wide representation,
        which has none): K = 1, the cell under each environment's cursor, read from the `pos` buffer on the device -- reward[i, 0, a - 1]
        is what action a > 0 of a narrow environment would be paid next.
        `start`: int32 [M, 8] or [8] rows that `over` is judged against; None: the level's own row, and with maps=None the handle's
        start statistics, so that `over` is what the episode would report (max_changes / max_iterations aside).
        A pure function like evaluate(): episodes, random streams and pending asynchronous searches are not touched, a tile id >=
        get_num_tiles() is clamped on the way and reported by check_status(); the workspace is evaluate()'s (the same one-stream rule).
        Which form runs where: the library's one call (pcgrl_get_changes: every level staged once, no-op entries not computed) wherever
        evaluate() has its fast form -- binary, zelda, and the compact searches of sokoban, mdungeon and ddave, maps up to 64 x 64 --
        and M * K * T + M below 2^31.  Elsewhere (smb, larger maps, the general searches, more entries, and a handle that waits for a
        reset() after an adjust_param() it could not take in place) the changed levels are built `chunk` entries at a time with
        torch indexing on the device and scored through evaluate(..., ref=...): the same result wherever evaluate() works; a device
        cell outside the map is clamped there too but not reported."""
        torch = self._torch
        own = maps is None
        if own and (self._handle is None or not self._was_reset or self._needs_reset):
            raise RuntimeError("changes() without maps reads the environment's current levels: call reset() first")
        self._scoring_handle()
        stale = self._realloc
        w, h = self._alloc_dims
        m = self._bufs["map"] if own else self._as_maps("changes", maps)
        M, T, ncell = int(m.shape[0]), self.get_num_tiles(), h * w
        if isinstance(cells, str):
            if cells != "cursor":
                raise ValueError("changes(): cells must be an array, None or \"cursor\", got %r" % (cells,))
            if self._rep.name == "wide":
                raise ValueError("changes(cells=\"cursor\"): the wide representation has no cursor")
            if not own:
                raise ValueError("changes(cells=\"cursor\") reads the environment's own cursors: leave maps=None")
            pos = self._bufs["pos"]
            c = (pos[:, 1].to(torch.int32) * w + pos[:, 0].to(torch.int32)).view(M, 1).contiguous()
        elif cells is None:
            c = None
        else:
            on_device = torch.is_tensor(cells) and cells.is_cuda
            c = cells if torch.is_tensor(cells) else torch.as_tensor(np.asarray(cells))
            if c.dtype not in (torch.int32, torch.int64, torch.int16, torch.int8, torch.uint8) or c.dim() not in (1, 2) or c.numel() < 1 or \
                    (c.dim() == 2 and c.shape[0] != M):
                raise ValueError("changes(): cells must be integers of shape [%d, K] or [K] with K >= 1, got %s %s" % (M, c.dtype, tuple(c.shape)))
            if not on_device and (int(c.min()) < 0 or int(c.max()) >= ncell):
                raise ValueError("changes(): a cell outside [0, %d) for maps of %d rows x %d columns" % (ncell, h, w))
            c = c.to(device=self.device, dtype=torch.int32)
            c = (c.expand(M, c.shape[0]) if c.dim() == 1 else c).contiguous()
        K = ncell if c is None else int(c.shape[1])
        if start is None:
            s = self._bufs["start_stats"] if own else None
        else:
            s = start if torch.is_tensor(start) else torch.as_tensor(np.asarray(start))
            if s.dtype not in (torch.int32, torch.int64) or tuple(s.shape) not in ((8,), (M, 8)):
                raise ValueError("changes(): start must be int32 rows of shape [%d, 8] or [8], got %s %s" % (M, s.dtype, tuple(s.shape)))
            s = s.to(device=self.device, dtype=torch.int32)
            s = (s.expand(M, 8) if s.dim() == 1 else s).contiguous()
        cfg = self._config(self._alloc_dims)
        need = 0 if stale else int(self._lib.pcgrl_get_changes_bytes(C.byref(cfg), M, K))
        if not need:
            return self._changes_by_evaluate(m, c, s, bool(rows), max(1, int(chunk)))
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        out_rows = torch.empty((M, K, T, 8), dtype=torch.int32, device=self.device) if rows else None
        reward = torch.empty((M, K, T), dtype=torch.float64, device=self.device)
        over = torch.empty((M, K, T), dtype=torch.uint8, device=self.device)
        base = torch.empty((M, 8), dtype=torch.int32, device=self.device)
        _lib.check(self._lib.pcgrl_get_changes(self._handle, ptr(m), M, ptr(c), K, ptr(s), ptr(base), ptr(out_rows), ptr(reward), ptr(over),
                                               *self._workspace(need), self._stream()), "pcgrl_get_changes")
        if c is None:
            c = torch.arange(ncell, dtype=torch.int32, device=self.device).expand(M, ncell)
        return Changes(out_rows, reward, over.view(torch.bool), base, c, self._prob.decode_rows(base))

    def _changes_by_evaluate(self, m, c, s, want_rows, chunk):
        """changes() where pcgrl_get_changes_bytes is 0: the entries in their order (m, k, t), `chunk` at a time -- each chunk's levels
        are copies of their level with the one byte written by torch indexing -- through evaluate(levels, ref=the level's own row);
        the no-op entries come out as the level's own row, their reward is set to 0; `over` against other start rows: pcgrl_get_reward
        on the chunk's rows."""
        torch = self._torch
        M, T = int(m.shape[0]), self.get_num_tiles()
        w, h = self._alloc_dims
        ncell = h * w
        base = self.evaluate(m, chunk=chunk).rows
        if c is None:
            c = torch.arange(ncell, dtype=torch.int32, device=self.device).expand(M, ncell)
        K = int(c.shape[1])
        cc = c.clamp(0, ncell - 1).to(torch.int64)
        flat = m.reshape(M, ncell)
        E = M * K * T
        rows = torch.empty((E, 8), dtype=torch.int32, device=self.device) if want_rows else None
        reward = torch.empty((E,), dtype=torch.float64, device=self.device)
        over = torch.empty((E,), dtype=torch.uint8, device=self.device)
        for i in range(0, E, chunk):
            n = min(chunk, E - i)
            levels, lv, noop = expand_changes(flat, cc, i, n, T)
            ev = self.evaluate(levels.view(n, h, w), ref=base[lv], chunk=chunk)
            if want_rows:
                rows[i:i + n] = ev.rows
            reward[i:i + n] = ev.reward.masked_fill(noop, 0.0)
            if s is None:
                over[i:i + n] = ev.over
            else:
                scorer = self._eval_scratch._handle if self._realloc else self._handle
                ref = s[lv].contiguous()
                _lib.check(self._lib.pcgrl_get_reward(scorer, C.c_void_p(ev.rows.data_ptr()), C.c_void_p(ref.data_ptr()), n, None,
                                                      C.c_void_p(over[i:i + n].data_ptr()), self._stream()), "pcgrl_get_reward")
        return Changes(rows.view(M, K, T, 8) if want_rows else None, reward.view(M, K, T), over.view(torch.bool).view(M, K, T), base, c,
                       self._prob.decode_rows(base))

    def _evaluate_by_set_maps(self, m, rows, chunk):
        """evaluate() where pcgrl_get_stats_bytes is 0: a scratch environment of this problem (wide representation, the same
        adjust_param state, no auto-reset) of min(M, chunk) maps, reset once; the maps go through its set_maps() chunk by chunk and
        the rows are copied out with the library's private slots zeroed.  This environment's handle is not touched -- its status word
        included: what set_maps() clamps on this route is reported by the scratch environment's (self._eval_scratch.check_status())."""
        import copy
        torch = self._torch
        M = int(m.shape[0])
        n = max(1, min(M, chunk))
        sc = self._eval_scratch
        if sc is None or sc.num_envs != n:
            self._drop_eval_scratch()
            sc = BatchedPcgrlEnv(prob=self._prob.name, rep="wide", num_envs=n, device=self.device, seed=0, auto_reset=False, tuning=self._tuning)
            sc._prob = copy.deepcopy(self._prob)
            sc._prob._width, sc._prob._height = self._alloc_dims
            sc._update_spaces()
            sc.reset()
            self._eval_scratch = sc
        nstats = int(sc._layout.nstats)
        for i in range(0, M, n):
            part = m[i:i + n]
            k = int(part.shape[0])
            if k < n:                      # the last chunk: the handle takes exactly n maps
                part = torch.cat([part, torch.zeros((n - k,) + tuple(part.shape[1:]), dtype=torch.uint8, device=self.device)])
            sc.set_maps(part)
            rows[i:i + k] = sc._bufs["stats"][:k]
        rows[:, nstats:] = 0

    def _drop_eval_scratch(self):
        if self._eval_scratch is not None:
            self._eval_scratch.close()
            self._eval_scratch = None

    def check_status(self):
        """Raise if a kernel flagged an unsupported case (synchronises)."""
        st = C.c_int32()
        _lib.check(self._lib.pcgrl_status(self._handle, self._stream(), C.byref(st)), "pcgrl_status")
        if st.value and self.strict_actions:       # report this call's problem only once: the word is sticky otherwise
            _lib.check(self._lib.pcgrl_clear_status(self._handle, self._stream()), "pcgrl_clear_status")
        if st.value & 1:
            raise RuntimeError("a level was outside the limits of a search kernel (a Sokoban level with more crates than the search takes -- 32 in the "
                               "compact searches, 256 in the general ones -- or more than 255 tiles / collected things of one kind in a packed statistics row)")
        if st.value & 2:
            raise IndexError("an action outside the action space was passed to step()/rollout() (it was clamped into range; "
                             "the reference raises IndexError or writes the bad value)")
        if st.value & 4:
            raise ValueError("set_maps() / evaluate() was given a tile id >= get_num_tiles() (it was clamped)")
        return st.value

    def profile(self, enable=True):
        """Record HIP events around every phase of step() on the current stream."""
        _lib.check(self._lib.pcgrl_profile(self._handle, int(enable)), "pcgrl_profile")

    def profile_read(self):
        """-> ({phase: total ms}, steps) since profile(True); synchronises."""
        ms = (C.c_double * _lib.NPHASE)()
        steps = C.c_int32()
        _lib.check(self._lib.pcgrl_profile_read(self._handle, ms, C.byref(steps)), "pcgrl_profile_read")
        return dict(zip(_lib.PHASES, list(ms))), steps.value

    @property
    def stats(self):
        return self._prob.decode_rows(self._bufs["stats"])

    def state_dict(self):
        """Everything a batch of environments carries between steps (checkpoint / resume): maps, first maps,
        heatmaps, cursors, counters, current and start stats, last step outputs, binary tile probabilities, both MT19937
        rings with their cursors, and the episode statistics when they are on.  Device tensors (clones)."""
        self.flush()                       # (asynchronous ticks: a step in flight is finished first -- a checkpoint holds completed steps only)
        self._torch.cuda.synchronize(self.device)
        sd = {k: (v.clone() if v is not None else None) for k, v in self._bufs.items() if k not in ("scratch", "planes")}
        if self._episode is not None:
            sd.update({"episode_" + k: v.clone() for k, v in self._episode.items()})
        return sd

    def load_state_dict(self, sd):
        """Restore `state_dict()` of an environment batch with the same problem, representation, size and parameters.
        The derived state (row planes, cached champion components) is rebuilt from the maps on the device."""
        if self._handle is None:
            raise RuntimeError("call reset() once before load_state_dict() (buffers are allocated lazily)")
        for k, v in sd.items():
            if v is None or k.startswith("episode_"):
                continue
            dst = self._bufs[k]
            if tuple(dst.shape) != tuple(v.shape) or dst.dtype != v.dtype:
                raise ValueError("state_dict entry %r does not fit this environment: %s %s vs %s %s" % (k, tuple(v.shape), v.dtype, tuple(dst.shape), dst.dtype))
            dst.copy_(v)
        if any(k.startswith("episode_") for k in sd):
            self.enable_episode_stats()
            for k, v in self._episode.items():
                v.copy_(sd["episode_" + k])
        stats = self._bufs["stats"].clone()
        self.set_maps(self._bufs["map"].clone())       # planes + champion cache from the maps; recomputes the current stats ...
        self._torch.cuda.synchronize(self.device)
        n = len(self._prob.stat_keys)
        if not self._torch.equal(self._bufs["stats"][:, :n], stats[:, :n]):   # ... which must be the ones that were saved
            raise ValueError("state_dict is inconsistent: the saved stats are not the stats of the saved maps")

    def set_graphics(self, graphics):
        """Tile pictures for render(): None = the reference's grey fallback (the default), "drawn" = the package's own
        pictures (envs/tile_art.py), or a dict {tile name: tile_size x tile_size x 3 image} -- the reference's `_graphics`."""
        self._palette = None               # (render_batch's device copy of the pictures: built again at the next call)
        if graphics is None:
            self._graphics = None
            return
        if isinstance(graphics, str):
            if graphics != "drawn":
                raise ValueError("unknown graphics %r" % (graphics,))
            from .tile_art import make_graphics
            graphics = make_graphics(self._prob.tiles, int(self._prob._tile_size))
        missing = [t for t in self._prob.tiles if t not in graphics]
        if missing:
            raise KeyError("no picture for tiles %r" % (missing,))
        self._graphics = dict(graphics)

    def render(self, mode="rgb_array", index=0):
        """Image of environment `index` with the reference's layout (pcgrl_env.py:161-175): 16-pixel tiles, a one-tile
        border of the border tile (problem.py:142-156), a two-pixel red frame on the cursor cell for narrow/turtle
        (narrow_rep.py:128-142).  The tile pictures are the reference's *fallback* graphics -- grey level
        i*255/len(tiles), problem.py:136-140 -- its PNG assets are not part of this package.  Host side, one
        device->host map copy; returns a PIL image when PIL is importable (like the reference), else an ndarray."""
        if mode not in ("rgb_array", "human"):
            raise ValueError("unsupported render mode %r" % (mode,))
        tiles = self._prob.tiles
        ts = int(self._prob._tile_size)
        bx, by = self._prob._border_size
        m = self._bufs["map"][index].cpu().numpy()
        h, w = m.shape
        full = np.full((h + 2 * by, w + 2 * bx), tiles.index(self._prob._border_tile), dtype=np.int64)
        full[by:by + h, bx:bx + w] = m
        gfx = getattr(self, "_graphics", None)
        if gfx is None:
            grey = np.array([int(i * 255 / len(tiles)) for i in range(len(tiles))], dtype=np.uint8)
            img = np.repeat(np.repeat(grey[full], ts, axis=0), ts, axis=1)
            img = np.stack([img, img, img], -1)
        else:                                             # Problem.render with a `_graphics` dict (problem.py:128-156)
            pal = np.stack([np.asarray(gfx[t], dtype=np.uint8)[:ts, :ts, :3] for t in tiles])       # [tile, ts, ts, 3]
            img = pal[full].transpose(0, 2, 1, 3, 4).reshape(full.shape[0] * ts, full.shape[1] * ts, 3).copy()
        if self._rep.has_pos:
            x, y = [int(v) for v in self._bufs["pos"][index].cpu().numpy()]
            y0, x0 = (y + by) * ts, (x + bx) * ts
            cell = img[y0:y0 + ts, x0:x0 + ts]
            for sl in (np.s_[:2, :], np.s_[-2:, :], np.s_[:, :2], np.s_[:, -2:]):
                cell[sl] = (255, 0, 0)
        try:
            from PIL import Image
            return Image.fromarray(img, "RGB")
        except ImportError:
            return img

    def _render_palette(self):
        """The tile pictures render() draws with -- the grey fallback or the `_graphics` dict, at the problem's tile size -- as a
        device tensor uint8 [tiles, ts, ts, 3]; built once, dropped by set_graphics() and by a change of the tile size."""
        ts = int(self._prob._tile_size)
        cached = getattr(self, "_palette", None)
        if cached is not None and cached[0] == ts:
            return cached[1]
        tiles = self._prob.tiles
        gfx = getattr(self, "_graphics", None)
        if gfx is None:
            grey = np.array([int(i * 255 / len(tiles)) for i in range(len(tiles))], dtype=np.uint8)
            pal = np.broadcast_to(grey[:, None, None, None], (len(tiles), ts, ts, 3))
        else:
            pal = np.stack([np.asarray(gfx[t], dtype=np.uint8)[:ts, :ts, :3] for t in tiles])
            if pal.shape != (len(tiles), ts, ts, 3):
                raise ValueError("tile pictures of %s for a tile size of %d" % (pal.shape[1:], ts))
        dev = self._torch.as_tensor(np.ascontiguousarray(pal)).to(self.device)
        self._palette = (ts, dev)
        return dev

    def render_batch(self, indices=None, out=None, grid=None):
        """The pictures render("rgb_array", i) draws, for many environments in one kernel launch on the device (pcgrl_render): a
        uint8 device tensor [K, Hp, Wp, 3], or with `grid` one picture [rows * Hp, cols * Wp, 3] with picture k in cell
        (k // cols, k % cols) and black cells behind the last one.
        indices: None = every environment; a sequence / numpy array, checked here (IndexError outside [0, num_envs)); or an int32 /
        int64 device tensor, used as it is without a look at its values -- an entry outside the range gives a black picture.  Any
        order, repeats, more entries than environments.
        grid: None = stacked; True = stable-baselines' tile_images rule (rendering.grid_shape); or (rows, cols).
        out: a contiguous, 16-byte aligned uint8 tensor of exactly the result's shape on this device (ValueError otherwise); every
        byte of it is written.  The call reads the state as it is and does not wait for the device."""
        from .. import rendering
        torch = self._torch
        if self._handle is None or self._needs_reset:
            raise RuntimeError("reset() must be called before render_batch()")
        keep = None
        if indices is None:
            count = self.num_envs
        elif torch.is_tensor(indices) and indices.device == self.device:
            if indices.dim() != 1 or indices.dtype not in (torch.int32, torch.int64):
                raise ValueError("indices: a one-dimensional int32 or int64 tensor")
            if indices.dtype == torch.int64:       # (a value beyond 32 bits must not wrap into the range)
                indices = indices.clamp(-1, self.num_envs)
            keep = indices.to(torch.int32).contiguous()
            count = int(keep.shape[0])
        else:
            idx = np.asarray(indices.cpu() if torch.is_tensor(indices) else indices)
            if idx.ndim != 1 or (idx.size and idx.dtype.kind not in "iu"):
                raise ValueError("indices: a one-dimensional sequence of integers")
            if idx.size and (int(idx.min()) < 0 or int(idx.max()) >= self.num_envs):
                raise IndexError("render_batch: environment index outside [0, %d)" % self.num_envs)
            keep = torch.as_tensor(np.ascontiguousarray(idx, dtype=np.int32)).to(self.device)
            count = int(idx.size)
        if count < 1:
            raise ValueError("render_batch: no environment chosen")
        cells = rendering.resolve_grid(grid, count)
        ts = int(self._prob._tile_size)
        bx, by = (int(v) for v in self._prob._border_size)
        h, w = (int(v) for v in self._bufs["map"].shape[1:])
        shape = rendering.picture_shape(h, w, (bx, by), ts, count, cells)
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=self.device)
        elif (not torch.is_tensor(out) or out.dtype != torch.uint8 or tuple(out.shape) != tuple(shape) or not out.is_contiguous()
              or out.device != self.device or out.data_ptr() % 16):
            raise ValueError("render_batch: out must be a contiguous, 16-byte aligned uint8 tensor of shape %s on %s" % (tuple(shape), self.device))
        pal = self._render_palette()
        d = _lib.RenderDesc()
        d.indices, d.count = (keep.data_ptr() if keep is not None else None), count
        d.tiles, d.tile_size = pal.data_ptr(), ts
        d.border_x, d.border_y = bx, by
        d.border_tile, d.cursor = self._prob.tiles.index(self._prob._border_tile), int(bool(self._rep.has_pos))
        d.grid_rows, d.grid_cols = cells if cells is not None else (0, 0)
        d.out = out.data_ptr()
        _lib.check(self._lib.pcgrl_render(self._handle, C.byref(d), self._stream()), "pcgrl_render")
        return out

    def close(self):
        self._drop_eval_scratch()
        self._free()

    def __del__(self):
        try:
            self._drop_eval_scratch()
            self._free()
        except Exception:
            pass
