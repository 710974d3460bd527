"""What the GPU tests of the level read-outs -- evaluate(), solve(), playthrough(), playthrough_smb(), paths() -- share: the environment
they score with, the fixture rows cut to max_len, a raw C call into guarded outputs, and the two routines every read-out is put
through: a tile id beyond the last, and a handle in the middle of its episodes."""
import ctypes as C

import numpy as np
import pytest

N_ENVS = 3
GUARD = 64
FILL = {1: 0x5A, 2: 0x5A5A, 4: 0x5A5A5A5A}      # by element size


def torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def make_env(prob, h, w, power=None, tuning=None, rep="wide", seed=1000, num_envs=N_ENVS, auto_reset=True):
    """An environment of `h` rows x `w` columns, not reset; solver_power `power` where one is given."""
    from gym_pcgrl_amd.envs import BatchedPcgrlEnv
    env = BatchedPcgrlEnv(prob=prob, rep=rep, num_envs=num_envs, seed=seed, auto_reset=auto_reset, tuning=tuning)
    kw = dict(width=w, height=h)
    if power is not None and prob == "smb":
        env._prob._solver_power = int(power)          # smb_prob.py:40-53: an attribute, not an adjust_param key
    elif power is not None:
        kw["solver_power"] = int(power)
    env.adjust_param(**kw)
    return env


def padded(want, max_len, dtype=np.int8):
    """The fixture's rows cut or -1 padded to max_len columns (the last axis)."""
    out = np.full(want.shape[:-1] + (max_len,), -1, dtype)
    k = min(max_len, want.shape[-1])
    out[..., :k] = want[..., :k]
    return out


def ptr(t, off=0):
    return C.c_void_p(t.data_ptr() + off)


class Guarded:
    """`n` elements of an output of a raw C call between two guards of GUARD elements, all of a known value."""

    def __init__(self, dtype, n, device):
        t = torch()
        self.full = t.full((GUARD + n + GUARD,), FILL[t.empty((), dtype=dtype).element_size()], dtype=dtype, device=device)
        self.fill = int(self.full[0].item())

    @property
    def ptr(self):
        return ptr(self.full, GUARD * self.full.element_size())

    @property
    def inner(self):
        return self.full[GUARD:-GUARD]

    def intact(self):
        return (self.full[:GUARD] == self.fill).all().item() and (self.full[-GUARD:] == self.fill).all().item()


def guarded_call(outs, call):
    """`call(*pointers of outs)` -> 0, and nothing written outside the outputs: both guards of each are intact."""
    assert call(*[o.ptr for o in outs]) == 0
    torch().cuda.synchronize()
    for o in outs:
        assert o.intact()


def check_bad_tile(env, call, fields, maps, cells, values=None):
    """`call(maps)` with the tile ids `values` (200) written into `cells` [(level, y, x)]: the result is that of the levels with the
    last tile there, check_status() reports it once, and the caller's tensor still holds what it was given.  Returns that result and those levels."""
    t = torch()
    nt = env.get_num_tiles()
    bad, clamped = maps.copy(), maps.copy()
    for (i, y, x), v in zip(cells, values or [200] * len(cells)):
        assert v >= nt
        bad[i, y, x] = v
        clamped[i, y, x] = nt - 1
    ref = call(clamped)
    assert env.check_status() == 0
    given = t.as_tensor(bad).to(env.device)
    got = call(given)
    for f in fields:
        assert t.equal(getattr(got, f), getattr(ref, f)), f
    with pytest.raises(ValueError):
        env.check_status()
    assert np.array_equal(given.cpu().numpy(), bad) and (given >= nt).sum().item() == len(cells)
    return ref, clamped


def check_handle_left_alone(make, sample_actions, call, fields, buffers, after_own=None, between=None, twin_too=False):
    """Twin environments from `make()`: `call(env)` on its own levels asks for a reset(); after 20 steps of `sample_actions(env)`
    ([40, N(, k)]) the read-out on its own levels and on a clone of them gives the same `fields`, and with `between(env)` -- other
    levels -- behind it state_dict() and the buffers `buffers(env)` names are what they were; then 20 more steps against the twin,
    the read-out every fifth step.  `twin_too`: the buffers are the twin's at the end."""
    t = torch()
    env, twin = make(), make()
    with pytest.raises(RuntimeError):
        call(env)                                                 # its own levels: only after a reset()
    acts = sample_actions(env)
    for e in (env, twin):
        e.reset()
        for s in range(20):
            e.step(acts[s])
    before = env.state_dict()
    names = buffers(env)
    bufs = {k: env._bufs[k].clone() for k in names}
    own = call(env)                                               # the handle's own map buffer, read in place
    again = call(env, env._bufs["map"].clone())
    for f in fields:
        assert t.equal(getattr(own, f), getattr(again, f)), f
    if after_own is not None:
        after_own(env, own)
    if between is not None:
        between(env)                                              # ... and other levels in between
    t.cuda.synchronize()
    after = env.state_dict()
    assert before.keys() == after.keys()
    for k in before:
        assert (before[k] is None and after[k] is None) or t.equal(before[k], after[k]), k
    for k, v in bufs.items():
        assert t.equal(env._bufs[k], v), k
    for s in range(20, 40):                                       # the episodes go on as if nothing had happened
        x, y = env.step(acts[s]), twin.step(acts[s])
        if s % 5 == 0:
            call(env)
        assert t.equal(x[0]["map"], y[0]["map"]) and t.equal(x[1], y[1]) and t.equal(x[2], y[2]), s
    if twin_too:
        for k in names:
            assert t.equal(env._bufs[k], twin._bufs[k]), k
    assert env.check_status() == 0
    for e in (env, twin):
        e.close()
