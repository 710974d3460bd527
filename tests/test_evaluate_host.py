"""pcgrl_get_stats_bytes / pcgrl_get_stats / pcgrl_get_reward (Problem.get_stats, get_reward and get_episode_over on any level): what
can be checked without a GPU -- the declarations with their reference citations, the exports and the ctypes mirror, the refusals
without a handle, which configurations have the one-call form, and how large its workspace is."""
import ctypes as C
import re

import pytest

from host_kit import config as _config, header, plain_header, prototype

NAMES = ("pcgrl_get_stats_bytes", "pcgrl_get_stats", "pcgrl_get_reward")


def _bytes(cfg, count):
    from gym_pcgrl_amd import _lib
    return int(_lib.load().pcgrl_get_stats_bytes(C.byref(cfg), count))


def test_declared_with_citations_exported_and_mirrored():
    from gym_pcgrl_amd import _lib
    hdr, plain = header(), plain_header()
    assert re.search(prototype("size_t", "pcgrl_get_stats_bytes", ["const pcgrl_config*", "int32_t"]), plain)
    assert re.search(prototype("int", "pcgrl_get_stats", ["pcgrl_env*", "const uint8_t*", "int32_t", "int32_t*", "void*", "size_t", "void*"]), plain)
    assert re.search(prototype("int", "pcgrl_get_reward", ["pcgrl_env*", "const int32_t*", "const int32_t*", "int32_t", "double*", "uint8_t*", "void*"]), plain)
    # each entry point's comment names the reference method it replaces
    for cited in ("binary_prob.py:81-92", "zelda_prob.py:80-122", "sokoban_prob.py:85-145", "mdungeon_prob.py", "ddave_prob.py",
                  "Problem.get_stats", "Problem.get_reward", "Problem.get_episode_over"):
        assert cited in hdr, cited
    assert "Still 15: + pcgrl_get_stats_bytes / pcgrl_get_stats / pcgrl_get_reward" in hdr           # the version comment, in the style of the others
    L = _lib.load()
    for name in NAMES:
        assert name in _lib.EXPORTS, name
        assert hasattr(L, name), name
    assert L.pcgrl_get_stats_bytes.argtypes == [C.POINTER(_lib.Config), C.c_int32] and L.pcgrl_get_stats_bytes.restype == C.c_size_t
    assert L.pcgrl_get_stats.argtypes == [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    assert L.pcgrl_get_reward.argtypes == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]


def test_abi_version_stays_15():
    from gym_pcgrl_amd import _lib
    assert _lib.load().pcgrl_abi_version() == _lib.ABI_VERSION == 15


def test_null_handle_is_refused():
    from gym_pcgrl_amd import _lib
    L = _lib.load()
    assert L.pcgrl_get_stats(None, None, 1, None, None, 0, None) == _lib.PCGRL_ESTATE
    assert L.pcgrl_get_reward(None, None, None, 1, None, None, None) == _lib.PCGRL_ESTATE
    # an unbound handle: refused the same way, before any argument is looked at
    cfg = _config("binary", 14, 14)
    h = C.c_void_p()
    assert L.pcgrl_create(C.byref(cfg), C.byref(h)) == 0
    try:
        assert L.pcgrl_get_stats(h, None, 1, None, None, 0, None) == _lib.PCGRL_ESTATE
        assert L.pcgrl_get_reward(h, None, None, 1, None, None, None) == _lib.PCGRL_ESTATE
    finally:
        L.pcgrl_destroy(h)


@pytest.mark.parametrize("prob,h,w,power", [("binary", 14, 14, None), ("zelda", 11, 16, None), ("binary", 64, 64, None), ("sokoban", 5, 5, 5000),
                                            ("mdungeon", 7, 11, 5000), ("ddave", 7, 11, 5000)])
def test_fast_form_reports_a_workspace(prob, h, w, power):
    cfg = _config(prob, h, w, power)
    for count in (1, 5, 279, 65536):
        b = _bytes(cfg, count)
        assert b >= 256 and b % 256 == 0, (count, b)
    cfg.num_envs = 12345                     # num_envs is ignored
    assert _bytes(cfg, 279) == _bytes(_config(prob, h, w, power), 279)


@pytest.mark.parametrize("prob,h,w,power", [("binary", 65, 130, None), ("sokoban", 16, 24, 2500), ("sokoban", 8, 8, 20000),
                                            ("smb", 4, 9, 200), ("smb", 14, 114, 10000), ("smb", 8, 24, 400), ("smb", 14, 40, 2500)])
def test_no_fast_form_reports_zero(prob, h, w, power):
    cfg = _config(prob, h, w, power)
    from gym_pcgrl_amd import _lib
    lay = _lib.Layout()
    assert _lib.load().pcgrl_query_layout(C.byref(cfg), C.byref(lay)) == 0        # a configuration the library takes ...
    assert _bytes(cfg, 1) == 0 and _bytes(cfg, 4096) == 0                          # ... without the one-call form


def test_count_below_one_reports_zero():
    from gym_pcgrl_amd import _lib
    cfg = _config("binary", 14, 14)
    assert _bytes(cfg, 0) == 0 and _bytes(cfg, -3) == 0
    assert int(_lib.load().pcgrl_get_stats_bytes(None, 4)) == 0


def _layout_sum(cfg):
    from gym_pcgrl_amd import _lib
    lay = _lib.Layout()
    assert _lib.load().pcgrl_query_layout(C.byref(cfg), C.byref(lay)) == 0
    return sum(int(getattr(lay, n)) for n in _lib.BUFFER_NAMES)


def test_workspace_is_smaller_than_a_scratch_handle():
    n = 65536
    for prob, h, w, power in (("binary", 14, 14, None), ("sokoban", 5, 5, 5000)):
        work = _bytes(_config(prob, h, w, power), n)
        state = _layout_sum(_config(prob, h, w, power, num_envs=n))
        assert 0 < work < state, (prob, work, state)
    # without a search there is nothing per map in the workspace
    for prob, h, w in (("binary", 14, 14), ("zelda", 11, 16)):
        cfg = _config(prob, h, w)
        assert _bytes(cfg, 1) == _bytes(cfg, 65536) == _bytes(cfg, 1 << 24)
