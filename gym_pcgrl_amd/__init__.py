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


def evaluate_levels(prob, maps, device=None, **params):
    """Problem.get_stats of a stack of levels in one call: `maps` array-like uint8 [M, H, W] (width and height are taken from it),
    `params` as for adjust_param (smb: solver_power is set as an attribute, smb_prob.py:40-53 has no such key).  Returns
    BatchedPcgrlEnv.evaluate()'s Evaluation (rows, stats)."""
    import numpy as np
    from .envs import BatchedPcgrlEnv
    shape = tuple(maps.shape) if hasattr(maps, "shape") else np.asarray(maps).shape
    if len(shape) != 3:
        raise ValueError("evaluate_levels(): maps must be [M, H, W], got shape %s" % (shape,))
    env = BatchedPcgrlEnv(prob=prob, rep="wide", num_envs=1, device=device, seed=0, auto_reset=False)
    try:
        power = params.pop("solver_power", None) if prob == "smb" else None
        env.adjust_param(width=int(shape[2]), height=int(shape[1]), **params)
        if power is not None:
            env._prob._solver_power = int(power)
            env.adjust_param()
        return env.evaluate(maps)
    finally:
        env.close()


def solve_levels(prob, maps, device=None, max_len=None, **params):
    """SokobanProblem.get_stats(map)["solution"] of a stack of levels in one call, next to evaluate_levels(): `maps` array-like uint8
    [M, H, W], `params` as for adjust_param.  Returns BatchedPcgrlEnv.solve()'s Solutions (moves, length, agent, rows, stats)."""
    import numpy as np
    from .envs import BatchedPcgrlEnv
    shape = tuple(maps.shape) if hasattr(maps, "shape") else np.asarray(maps).shape
    if len(shape) != 3:
        raise ValueError("solve_levels(): maps must be [M, H, W], got shape %s" % (shape,))
    env = BatchedPcgrlEnv(prob=prob, rep="wide", num_envs=1, device=device, seed=0, auto_reset=False)
    try:
        env.adjust_param(width=int(shape[2]), height=int(shape[1]), **params)
        return env.solve(maps, max_len=max_len)
    finally:
        env.close()


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


register_with_gym()      # no-op without a gym of the reference's era (none is on the MI355X image)
register_with_gymnasium()   # likewise for gymnasium / gym >= 0.26 (five-tuple adapter)
