"""pcgrl_bind_row (the step kernels write the rollout row): what can be checked without a GPU -- the entry point and its struct in
the header, the library and the ctypes mirror; the collector's choice between the two loops; the argument checks."""
import ctypes as C
import re

import numpy as np
import pytest

from host_kit import header, prototype, struct_fields

_C_TYPES = {"int64_t*": C.c_void_p, "double*": C.c_void_p, "uint8_t*": C.c_void_p, "const uint8_t*": C.c_void_p, "int32_t*": C.c_void_p,
            "int32_t": C.c_int32}


def test_entry_point_is_declared_exported_and_mirrored():
    from gym_pcgrl_amd import _lib
    assert re.search(prototype("int", "pcgrl_bind_row", ["pcgrl_env*", "const pcgrl_row*"]), header())
    assert "pcgrl_bind_row" in _lib.EXPORTS
    L = _lib.load()                      # (load() itself insists on every name of EXPORTS)
    assert hasattr(L, "pcgrl_bind_row")
    assert L.pcgrl_abi_version() == _lib.ABI_VERSION == 15         # an addition within the version: found by its symbol
    fields = struct_fields("pcgrl_row", _C_TYPES)
    assert [n for n, _ in fields] == list(_lib.ROW_FIELDS) + ["actions_i64"]
    assert [n for n, _ in _lib.Row._fields_] == [n for n, _ in fields]

    class FromHeader(C.Structure):
        _fields_ = fields
    assert C.sizeof(_lib.Row) == C.sizeof(FromHeader) == 9 * C.sizeof(C.c_void_p) + 8          # nine pointers, an int32, padding
    for n, _ in fields:
        assert getattr(_lib.Row, n).offset == getattr(FromHeader, n).offset, n
    assert L.pcgrl_bind_row(None, None) == _lib.PCGRL_ESTATE       # no handle: refused, nothing touched


class _FakeWrapper:
    """An image wrapper on CPU tensors without bind_rollout_row(): step t gives reward t and fills the image with t + 1."""

    def __init__(self, torch, n, shape):
        self.torch, self.t = torch, 0
        self._obs = torch.zeros((n,) + shape, dtype=torch.uint8)
        self.pcgrl_env = type("E", (), {"_torch": torch, "device": torch.device("cpu")})()

    def set_observation_target(self, out):
        self._obs = out

    def reset(self):
        self._obs.fill_(1)
        return self._obs

    def step(self, actions):
        self.t += 1
        self._obs.fill_(self.t + 1)
        n = self._obs.shape[0]
        return self._obs, self.torch.full((n,), float(self.t), dtype=self.torch.float64), self.torch.zeros(n, dtype=self.torch.bool), None


def _fake_vec(torch, n, shape):
    from gym_pcgrl_amd import spaces
    w = _FakeWrapper(torch, n, shape)
    vec = type("V", (), {})()
    vec.env, vec.num_envs, vec.monitor = w, n, False
    vec.action_space = spaces.Discrete(3)
    vec.observation_space = spaces.Box(low=0, high=255, shape=shape, dtype=np.uint8)
    vec.reset = w.reset
    return vec


def test_collector_without_the_binding_falls_back_or_raises():
    import torch
    from gym_pcgrl_amd.rollout import DoubleBufferedCollector, RolloutCollector
    n, shape, T = 4, (4, 4, 1), 5
    for kr in (None, False):
        col = RolloutCollector(_fake_vec(torch, n, shape), T, kernel_rows=kr)
        assert col.kernel_rows is False
        for r in range(2):
            b = col.collect(lambda obs: torch.full((n,), 2, dtype=torch.int64))
            assert b.rewards[:, 0].tolist() == [float(T * r + t + 1) for t in range(T)]
            assert bool((b.actions == 2).all()) and not bool(b.dones.any())
            assert b.episode_starts[0].tolist() == [r == 0] * n and not bool(b.episode_starts[1:].any())
            assert int(b.last_obs.max()) == T * (r + 1) + 1
    assert RolloutCollector(_fake_vec(torch, n, shape), T).kernel_rows is False          # the default is None
    with pytest.raises(ValueError):
        RolloutCollector(_fake_vec(torch, n, shape), T, kernel_rows=True)
    assert "kernel_rows" in DoubleBufferedCollector.__init__.__code__.co_varnames
    buf = RolloutCollector(_fake_vec(torch, n, shape), T).buffer
    assert tuple(buf.ep_returns.shape) == tuple(buf.ep_lengths.shape) == (T, n)
    assert buf.ep_returns.dtype == torch.float64 and buf.ep_lengths.dtype == torch.int32


def test_bind_rollout_row_checks_its_arguments():
    import torch
    from gym_pcgrl_amd.envs import BatchedPcgrlEnv
    n = 6
    env = BatchedPcgrlEnv(prob="binary", rep="narrow", num_envs=n, seed=1, device="cuda:0")      # (nothing is allocated before reset())
    z = lambda shape, dt: torch.zeros(shape, dtype=dt)
    # every check has a message of its own and the device is looked at last, so that each case fails for the reason it is listed
    # under (all tensors here are host tensors: a case whose check were missing would get "wrong device" instead)
    bad = [("wrong dtype", dict(reward=z((n,), torch.float32))),
           ("wrong dtype", dict(actions_out=z((n,), torch.int32))),
           ("wrong dtype", dict(done=z((n,), torch.int32))),
           ("wrong dtype", dict(ep_length=z((n,), torch.int64))),
           ("wrong dtype", dict(took=np.zeros(n, np.uint8))),
           ("wrong shape", dict(reward=z((n + 1,), torch.float64))),
           ("wrong shape", dict(actions_out=z((n, 2), torch.int64))),
           ("wrong shape", dict(took=z((n, 1), torch.bool))),
           ("not contiguous", dict(reward=z((n, 2), torch.float64)[:, 0])),
           ("not contiguous", dict(fresh=z((2 * n,), torch.bool)[::2])),
           ("wrong device", dict(reward=z((n,), torch.float64)))]       # right in everything else
    for why, cols in bad:
        with pytest.raises(ValueError, match=why):
            env.bind_rollout_row(**cols)
        assert env._row is None
    with pytest.raises(TypeError):
        env.bind_rollout_row(rewards=z((n,), torch.float64))
    assert env._row is None
    env.bind_rollout_row(reward=None)       # nothing wanted: nothing bound
    env.unbind_rollout_row()
    assert env._row is None
