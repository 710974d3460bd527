"""gym_pcgrl_amd: MI355X-native batched PCGRL environment (the step()/reset() hot path of
amidos2006/gym-pcgrl as hand-written HIP kernels for gfx950, behind the reference's env surface).

    import gym_pcgrl_amd
    env = gym_pcgrl_amd.make("binary-narrow-v0")                       # reference-style single env
    venv = gym_pcgrl_amd.make_batched("binary-narrow-v0", num_envs=65536)  # one GPU, lockstep batch

Ids follow gym_pcgrl/__init__.py:6-12: '{prob}-{rep}-v0' for the in-scope problems
(binary, zelda, sokoban) x all six representations (narrow, narrowcast, narrowmulti, wide, turtle, turtlecast).
"""
__version__ = "0.1.0"

_ENV_IDS = {}


def _register_all():
    from .envs.problems import PROBLEMS
    from .envs.representations import REPRESENTATIONS
    for prob in PROBLEMS:
        for rep in REPRESENTATIONS:
            _ENV_IDS["%s-%s-v0" % (prob, rep)] = (prob, rep)


def registered_ids():
    if not _ENV_IDS:
        _register_all()
    return sorted(_ENV_IDS)


def register_with_gym():
    """Register every id with gym when one with the reference's four-tuple API is importable (gym_pcgrl/__init__.py:6-12 does this on
    import; so does this package, below).  Returns the ids registered by this call."""
    from . import gym_compat
    if gym_compat.find_gym() is None:
        return []
    if not _ENV_IDS:
        _register_all()
    return gym_compat.register_all(_ENV_IDS)


def register_with_gymnasium():
    """The same for the new API (gymnasium, or gym >= 0.26): the ids are registered there with the five-tuple adapter
    `gymnasium_compat.NewApiPcgrlEnv` as entry point.  Returns the ids registered by this call."""
    from . import gymnasium_compat
    if gymnasium_compat.find_gymnasium() is None:
        return []
    if not _ENV_IDS:
        _register_all()
    return gymnasium_compat.register_all(_ENV_IDS)


def _lookup(env_id):
    if not _ENV_IDS:
        _register_all()
    if env_id not in _ENV_IDS:
        raise KeyError("unknown environment id %r; available: %s" % (env_id, ", ".join(sorted(_ENV_IDS))))
    return _ENV_IDS[env_id]


def make(env_id, **kwargs):
    """gym.make(id) replacement: a single reference-style PcgrlEnv backed by the HIP kernels."""
    from .envs import PcgrlEnv
    prob, rep = _lookup(env_id)
    return PcgrlEnv(prob=prob, rep=rep, **kwargs)


def make_batched(env_id, num_envs, **kwargs):
    from .envs import BatchedPcgrlEnv
    prob, rep = _lookup(env_id)
    return BatchedPcgrlEnv(prob=prob, rep=rep, num_envs=num_envs, **kwargs)


def _on_levels(who, prob, maps, device, params, call, smb_power=None):
    """What the *_levels() functions share: the shape check, a one-environment handle of the levels' width and height with `params`
    applied (adjust_param), `call(env)`, close().  `smb_power`: where smb's solver_power -- an attribute, smb_prob.py:40-53 has no
    such key -- is set: "before" or "after" that adjust_param (then followed by one more), None: it stays in `params`."""
    import numpy as np
    from .envs import BatchedPcgrlEnv
    shape = tuple(maps.shape) if hasattr(maps, "shape") else np.asarray(maps).shape
    if len(shape) != 3:
        raise ValueError("%s(): maps must be [M, H, W], got shape %s" % (who, shape))
    env = BatchedPcgrlEnv(prob=prob, rep="wide", num_envs=1, device=device, seed=0, auto_reset=False)
    try:
        power = params.pop("solver_power", None) if smb_power and prob == "smb" else None
        if power is not None and smb_power == "before":
            env._prob._solver_power = int(power)
        env.adjust_param(width=int(shape[2]), height=int(shape[1]), **params)
        if power is not None and smb_power == "after":
            env._prob._solver_power = int(power)
            env.adjust_param()
        return call(env)
    finally:
        env.close()


def evaluate_levels(prob, maps, device=None, **params):
    """Problem.get_stats of a stack of levels in one call: `maps` array-like uint8 [M, H, W] (width and height are taken from it),
    `params` as for adjust_param (smb: solver_power is set as an attribute, smb_prob.py:40-53 has no such key).  Returns
    BatchedPcgrlEnv.evaluate()'s Evaluation (rows, stats)."""
    return _on_levels("evaluate_levels", prob, maps, device, params, lambda env: env.evaluate(maps), smb_power="after")


def solve_levels(prob, maps, device=None, max_len=None, **params):
    """SokobanProblem.get_stats(map)["solution"] of a stack of levels in one call, next to evaluate_levels(): `maps` array-like uint8
    [M, H, W], `params` as for adjust_param.  Returns BatchedPcgrlEnv.solve()'s Solutions (moves, length, agent, rows, stats)."""
    return _on_levels("solve_levels", prob, maps, device, params, lambda env: env.solve(maps, max_len=max_len))


def path_levels(prob, maps, device=None, max_len=None, **params):
    """The paths behind binary's path-length and zelda's path-length / nearest-enemy of a stack of levels in one call, next to
    solve_levels(): `maps` array-like uint8 [M, H, W], `params` as for adjust_param.  Returns BatchedPcgrlEnv.paths()'s Paths (cells,
    length, rows, stats)."""
    return _on_levels("path_levels", prob, maps, device, params, lambda env: env.paths(maps, max_len=max_len))


def change_levels(prob, maps, cells=None, device=None, start=None, rows=True, **params):
    """Every one-cell change of a stack of levels scored in one call, next to evaluate_levels() and path_levels(): `maps` array-like
    uint8 [M, H, W], `cells` [M, K] or [K] (y * W + x each; None: every cell), `params` as for adjust_param (smb: solver_power is set
    as an attribute, like evaluate_levels()).  Returns BatchedPcgrlEnv.changes()'s Changes (rows, reward, over, base_rows, cells, stats)."""
    return _on_levels("change_levels", prob, maps, device, params, lambda env: env.changes(maps, cells=cells, start=start, rows=rows), smb_power="after")


class PathCheck:
    """What check_path() returns: `legal` bool [T] per cell (in range, on a passable tile, 4-adjacent to the cell before it, not seen
    before) and `ok`: every cell is legal."""
    __slots__ = ("legal", "ok")

    def __init__(self, legal, ok):
        self.legal, self.ok = legal, ok


def check_path(level, cells, passable_tiles):
    """Is `cells` (y * W + x each; a negative entry ends the list, like the -1 padding of Paths.cells) a walk on `level` [H, W] of tile
    ids: every cell in range, on one of `passable_tiles`, 4-adjacent to the one before it, and none repeated?  Host side, numpy: for a
    drawing loop, and a check of paths() that owes nothing to a recorded result.  Returns a PathCheck (legal per cell, ok)."""
    import numpy as np
    lv = np.asarray(level)
    if lv.ndim != 2:
        raise ValueError("check_path(): level must be [H, W], got shape %s" % (lv.shape,))
    H, W = lv.shape
    ok_tiles = set(int(t) for t in np.asarray(passable_tiles).reshape(-1).tolist())
    legal, seen, prev = [], set(), None
    for c in np.asarray(cells).reshape(-1).tolist():
        if c < 0:
            break
        c = int(c)
        good = c < H * W and int(lv[c // W, c % W]) in ok_tiles and c not in seen
        if good and prev is not None:
            good = prev < H * W and abs(c // W - prev // W) + abs(c % W - prev % W) == 1
        legal.append(bool(good))
        seen.add(c)
        prev = c
    legal = np.array(legal, bool)
    return PathCheck(legal, bool(legal.all()))


class SokobanReplay:
    """What replay_sokoban() returns: `player` int [T+1, 2] and `crates` int [T+1, K, 2] -- (row, column) per frame, frame 0 the level
    as given, frame t after move t; the crates keep their row-major order of frame 0 -- `targets` int [K', 2], `legal` (every move
    moved the player) and `won` (every target is covered by a crate at the end)."""
    __slots__ = ("player", "crates", "targets", "legal", "won")

    def __init__(self, player, crates, targets, legal, won):
        self.player, self.crates, self.targets, self.legal, self.won = player, crates, targets, legal, won


def replay_sokoban(level, moves):
    """Play `moves` (0..3 = left, right, up, down; a negative entry ends the list, like the -1 padding of Solutions.moves) on one
    sokoban level [H, W] of tile ids (0 empty, 1 solid, 2 player, 3 crate, 4 target) by the game's rules: outside the level is solid;
    the player steps onto a free cell, or onto a crate's cell if the cell behind the crate is neither solid nor a crate -- the crate
    moves there; any other move changes nothing.  Host side, numpy.  Returns a SokobanReplay."""
    import numpy as np
    lv = np.asarray(level)
    if lv.ndim != 2:
        raise ValueError("replay_sokoban(): level must be [H, W], got shape %s" % (lv.shape,))
    H, W = lv.shape
    who = np.argwhere(lv == 2)
    if len(who) != 1:
        raise ValueError("replay_sokoban(): the level needs exactly one player tile, it has %d" % len(who))
    pos = (int(who[0][0]), int(who[0][1]))
    crates = [(int(r), int(c)) for r, c in np.argwhere(lv == 3)]
    targets = [(int(r), int(c)) for r, c in np.argwhere(lv == 4)]
    step = ((0, -1), (0, 1), (-1, 0), (1, 0))

    def solid(p):
        return not (0 <= p[0] < H and 0 <= p[1] < W) or lv[p] == 1

    players, frames, legal = [pos], [list(crates)], True
    for mv in np.asarray(moves).reshape(-1).tolist():
        if mv < 0:
            break
        if mv > 3:
            raise ValueError("replay_sokoban(): move %d is not one of 0..3" % mv)
        dr, dc = step[mv]
        to = (pos[0] + dr, pos[1] + dc)
        moved = False
        if not solid(to):
            if to in crates:
                behind = (to[0] + dr, to[1] + dc)
                if not solid(behind) and behind not in crates:
                    crates[crates.index(to)] = behind
                    moved = True
            else:
                moved = True
        if moved:
            pos = to
        legal = legal and moved
        players.append(pos)
        frames.append(list(crates))
    won = all(t in crates for t in targets)
    return SokobanReplay(np.array(players, np.int64).reshape(-1, 2), np.array(frames, np.int64).reshape(len(frames), len(crates), 2),
                         np.array(targets, np.int64).reshape(-1, 2), bool(legal), bool(won))


def playthrough_levels(prob, maps, device=None, max_len=None, **params):
    """The play behind the mdungeon / ddave planner statistics of a stack of levels in one call, next to solve_levels(): `maps`
    array-like uint8 [M, H, W], `params` as for adjust_param.  Returns BatchedPcgrlEnv.playthrough()'s Playthroughs (moves, length,
    agent, rows, stats)."""
    return _on_levels("playthrough_levels", prob, maps, device, params, lambda env: env.playthrough(maps, max_len=max_len))


class MdungeonReplay:
    """What replay_mdungeon() returns: `player` int [T+1, 2] -- (row, column) per frame, frame 0 the level as given, frame t after move
    t -- and per frame `health`, `potions`, `treasures`, `enemies` int [T+1] (collected / killed so far); of the last frame `won`
    (alive on the exit), `dead` (health 0) and `heuristic` (distance to the exit + 4 * (5 - health) - 4 * treasures)."""
    __slots__ = ("player", "health", "potions", "treasures", "enemies", "won", "dead", "heuristic")

    def __init__(self, player, health, potions, treasures, enemies, won, dead, heuristic):
        self.player, self.health, self.potions, self.treasures, self.enemies = player, health, potions, treasures, enemies
        self.won, self.dead, self.heuristic = won, dead, heuristic


class DdaveReplay:
    """What replay_ddave() returns: `player` int [T+1, 2] -- (row, column) per frame, frame 0 the level as given, frame t after move t --
    and per frame `jumps`, `diamonds`, `has_key`, `air` int [T+1] (jumps made, diamonds collected, 1 once the key is picked up, the air
    time left); of the last frame `won` (on the exit with the key), `dead` (on a spike) and `heuristic` (distance to the exit, or while
    the key lies there distance to the key + bordered width + bordered height; minus 5 per diamond)."""
    __slots__ = ("player", "jumps", "diamonds", "has_key", "air", "won", "dead", "heuristic")

    def __init__(self, player, jumps, diamonds, has_key, air, won, dead, heuristic):
        self.player, self.jumps, self.diamonds, self.has_key, self.air = player, jumps, diamonds, has_key, air
        self.won, self.dead, self.heuristic = won, dead, heuristic


def _replay_level(name, level, ntiles, need):
    import numpy as np
    lv = np.asarray(level)
    if lv.ndim != 2:
        raise ValueError("%s(): level must be [H, W], got shape %s" % (name, lv.shape))
    if lv.size and int(lv.max()) >= ntiles:
        raise ValueError("%s(): tile id %d is not one of 0..%d" % (name, int(lv.max()), ntiles - 1))
    where = []
    for tile, what in need:
        at = np.argwhere(lv == tile)
        if len(at) != 1:
            raise ValueError("%s(): the level needs exactly one %s tile, it has %d" % (name, what, len(at)))
        where.append((int(at[0][0]), int(at[0][1])))
    return lv, where


def _replay_moves(name, moves):
    import numpy as np
    out = []
    for mv in np.asarray(moves).reshape(-1).tolist():
        if mv < 0:
            break
        if mv > 3:
            raise ValueError("%s(): move %d is not one of 0..3" % (name, mv))
        out.append(int(mv))
    return out


def replay_mdungeon(level, moves):
    """Play `moves` (0..3 = left, right, up, down; a negative entry ends the list, like the -1 padding of Playthroughs.moves) on one
    MiniDungeons level [H, W] of tile ids (0 empty, 1 solid, 2 player, 3 exit, 4 potion, 5 treasure, 6 goblin, 7 ogre) by the game's
    rules: outside the level is solid; the player starts with health 5; a step into a solid cell changes nothing; walking onto a potion
    gives +2 health (at most 5), onto a treasure +1 treasure, onto a goblin / ogre costs 1 / 2 health (not below 0) and counts as a
    kill; the thing is gone.  Once the player is dead (health 0) or stands on the exit, nothing moves any more.  Host side, numpy.
    Returns a MdungeonReplay."""
    import numpy as np
    lv, (pos, door) = _replay_level("replay_mdungeon", level, 8, ((2, "player"), (3, "exit")))
    H, W = lv.shape
    things = {(int(r), int(c)): int(lv[r, c]) for r, c in np.argwhere(lv >= 4)}
    step = ((0, -1), (0, 1), (-1, 0), (1, 0))
    health, potions, treasures, enemies = 5, 0, 0, 0
    frames = [(pos, health, potions, treasures, enemies)]
    for mv in _replay_moves("replay_mdungeon", moves):
        to = (pos[0] + step[mv][0], pos[1] + step[mv][1])
        over = health == 0 or pos == door
        if not over and 0 <= to[0] < H and 0 <= to[1] < W and lv[to] != 1:
            pos = to
            t = things.pop(to, None)
            if t == 4:
                health, potions = min(health + 2, 5), potions + 1
            elif t == 5:
                treasures += 1
            elif t is not None:
                health, enemies = max(health - (2 if t == 7 else 1), 0), enemies + 1
        frames.append((pos, health, potions, treasures, enemies))
    col = lambda k: np.array([f[k] for f in frames], np.int64)
    heuristic = abs(pos[0] - door[0]) + abs(pos[1] - door[1]) + 4 * (5 - health) - 4 * treasures
    return MdungeonReplay(np.array([f[0] for f in frames], np.int64).reshape(-1, 2), col(1), col(2), col(3), col(4),
                          bool(health > 0 and pos == door), bool(health == 0), int(heuristic))


def replay_ddave(level, moves):
    """Play `moves` (0..3 = stay, left, right, jump; a negative entry ends the list) on one Dangerous Dave level [H, W] of tile ids
    (0 empty, 1 solid, 2 player, 3 exit, 4 diamond, 5 key, 6 spike) by the game's rules: outside the level is solid; a sideways move
    steps into a cell that is not solid; a jump starts only from the ground (a solid cell below) under a free ceiling and gives air
    time 3 and +1 jump; then, in every move, with air time above 1 it drops by one and the player rises one cell (a solid cell above
    leaves air time 1 instead), with air time 1 the player hovers (air time 0), else the player falls one cell if the cell below is
    not solid.  On the cell reached a diamond is picked up, else a spike kills, else the key is picked up.  Once the player is dead or
    stands on the exit with the key, nothing moves any more.  Host side, numpy.  Returns a DdaveReplay."""
    import numpy as np
    lv, (pos, door, key) = _replay_level("replay_ddave", level, 7, ((2, "player"), (3, "exit"), (5, "key")))
    H, W = lv.shape

    def solid(r, c):
        return not (0 <= r < H and 0 <= c < W) or lv[r, c] == 1

    left = {(int(r), int(c)) for r, c in np.argwhere(lv == 4)}
    alive, has_key, air, jumps, diamonds = True, 0, 0, 0, 0
    frames = [(pos, jumps, diamonds, has_key, air)]
    for mv in _replay_moves("replay_ddave", moves):
        if alive and not (has_key and pos == door):
            r, c = pos
            if mv == 1 and not solid(r, c - 1):
                c -= 1
            elif mv == 2 and not solid(r, c + 1):
                c += 1
            elif mv == 3 and solid(pos[0] + 1, pos[1]) and not solid(pos[0] - 1, pos[1]):
                air, jumps = 3, jumps + 1
            if air > 1:
                air -= 1
                if not solid(r - 1, c):
                    r -= 1
                else:
                    air = 1
            elif air == 1:
                air = 0
            elif not solid(r + 1, c):
                r += 1
            pos = (r, c)
            if pos in left:
                left.discard(pos)
                diamonds += 1
            elif lv[pos] == 6:
                alive = False
            elif not has_key and pos == key:
                has_key = 1
        frames.append((pos, jumps, diamonds, has_key, air))
    col = lambda k: np.array([f[k] for f in frames], np.int64)
    goal = door if has_key else key
    heuristic = abs(pos[0] - goal[0]) + abs(pos[1] - goal[1]) + (0 if has_key else W + 2 + H + 2) - 5 * diamonds
    return DdaveReplay(np.array([f[0] for f in frames], np.int64).reshape(-1, 2), col(1), col(2), col(3), col(4),
                       bool(alive and has_key and pos == door), bool(not alive), int(heuristic))


def playthrough_smb_levels(maps, device=None, max_len=None, **params):
    """The play behind smb's jumps / jumps-dist / dist-win of a stack of levels in one call, next to playthrough_levels(): `maps`
    array-like uint8 [M, H, W], `params` as for adjust_param plus solver_power (set as an attribute: smb_prob.py:40-53 has no such
    key).  Returns BatchedPcgrlEnv.playthrough_smb()'s Playthroughs (moves, length, agent, rows, stats)."""
    return _on_levels("playthrough_smb_levels", "smb", maps, device, params, lambda env: env.playthrough_smb(maps, max_len=max_len), smb_power="before")


class SmbReplay:
    """What replay_smb() returns: `player` int [T+1, 2] -- (x, y) per frame in the engine's padded grid (x = map column + 3; y = map
    row, negative above the screen), frame 0 the start, frame t after move t -- and per frame `air` (air time left) and `jumps` int
    [T+1]; `jump_cols` (the engine column of every jump, in order); of the last frame `won` (x at the pole's column), `lost` (fallen
    below the screen) and `dist_win` (columns left to the pole; SMBProblem reports 0 for a won play)."""
    __slots__ = ("player", "air", "jumps", "jump_cols", "won", "lost", "dist_win")

    def __init__(self, player, air, jumps, jump_cols, won, lost, dist_win):
        self.player, self.air, self.jumps, self.jump_cols, self.won, self.lost, self.dist_win = player, air, jumps, jump_cols, won, lost, dist_win


def replay_smb(level, moves):
    """Play `moves` (0 stay, 1 right, 2 jump, 3 right + jump; a negative entry ends the list, like the -1 padding of
    Playthroughs.moves) on one smb level [H, W] of tile ids (0 empty, 1 solid, 2 enemy, 3 brick, 4 question, 5 coin, 6 tube) by the
    game's rules.  The grid is the level with three columns added on either side, solid in the last two rows; solid, brick, question
    and tube block.  The player starts at (1, H - 3); the pole stands in column W + 4 on a block at row H - 3, and reaching that
    column wins.  Left of column 0, right of the grid and below it nothing can be entered; above the screen everything is free.  A move
    to the right steps into a free cell.  A jump starts only with a blocked cell below (which the rows above the screen and the last
    row never have) and a free cell above the cell the player has moved to: air time 5, +1 jump, the column before the move is noted.
    A move without jump cuts a running jump to air time 1.  Then, with air time above 1 it drops by one and the player rises one cell
    (a blocked cell above leaves air time 1 instead), with air time 1 the player hovers (air time 0), else the player falls one
    cell if the cell below can be entered.  Once the player has won or stands below the screen (lost) nothing moves any more.  A
    level of height 3 has no pole: the start already counts as won.  Host side, numpy.  Returns a SmbReplay."""
    import numpy as np
    lv = np.asarray(level)
    if lv.ndim != 2:
        raise ValueError("replay_smb(): level must be [H, W], got shape %s" % (lv.shape,))
    H, W = lv.shape
    if H < 3:
        raise ValueError("replay_smb(): a level has at least 3 rows, got %d" % H)
    if lv.size and int(lv.max()) > 6:
        raise ValueError("replay_smb(): tile id %d is not one of 0..6" % int(lv.max()))
    GW = W + 6
    grid = np.zeros((H, GW), bool)
    grid[H - 2:, :3] = grid[H - 2:, W + 3:] = True
    grid[H - 3, W + 4] = True
    grid[:, 3:W + 3] = np.isin(lv, (1, 3, 4, 6))
    exit_x = W + 4 if H > 3 else -1

    def free(x, y):
        return y < 0 or (0 <= x < GW and y < H and not grid[y, x])

    x, y, air, jumps, cols = 1, H - 3, 0, 0, []
    frames = [(x, y, air, jumps)]
    for mv in _replay_moves("replay_smb", moves):
        if x < exit_x and y < H:
            ground = -1 <= y < H - 1 and bool(grid[y + 1, x])
            nx = x + 1 if (mv & 1) and free(x + 1, y) else x
            if mv & 2:
                if ground and free(nx, y - 1):
                    air, jumps = 5, jumps + 1
                    cols.append(x)
            elif air > 0:
                air = 1
            ny = y
            if air > 1:
                air -= 1
                if free(nx, y - 1):
                    ny = y - 1
                else:
                    air = 1
            elif air == 1:
                air = 0
            elif free(nx, y + 1):
                ny = y + 1
            x, y = nx, ny
        frames.append((x, y, air, jumps))
    col = lambda k: np.array([f[k] for f in frames], np.int64)
    return SmbReplay(np.array([(f[0], f[1]) for f in frames], np.int64).reshape(-1, 2), col(2), col(3), np.array(cols, np.int64),
                     bool(x >= exit_x), bool(y >= H), int(exit_x - x))


from . import helper  # noqa: E402,F401  (gym_pcgrl/envs/helper.py on the device for any tile set: gym_pcgrl_amd.helper.calc_num_regions(maps, tiles), ...)

register_with_gym()      # no-op without a gym of the reference's era (none is on the MI355X image)
register_with_gymnasium()   # likewise for gymnasium / gym >= 0.26 (five-tuple adapter)
