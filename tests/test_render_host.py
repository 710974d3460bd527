"""pcgrl_render (level pictures drawn on the device): what can be checked without a GPU -- the entry point and its struct in the
header, the library and the ctypes mirror; the grid-shape rule; the kernel's scratch use read from the compiler's assembly."""
import ctypes as C
import re

import pytest

from host_kit import header, kernel_resources, prototype, struct_fields

_C_TYPES = {"const int32_t*": C.c_void_p, "const uint8_t*": C.c_void_p, "uint8_t*": C.c_void_p, "int32_t": C.c_int32}


def test_entry_point_is_declared_exported_and_mirrored():
    from gym_pcgrl_amd import _lib
    hdr = header()
    assert re.search(prototype("int", "pcgrl_render", ["pcgrl_env*", "const pcgrl_render_desc*", "void*"]), hdr)
    for cited in ("pcgrl_env.py:161-175", "problem.py:134-156", "narrow_rep.py:128-142", "turtle_rep.py:142"):
        assert cited in hdr, cited
    assert "pcgrl_render" in _lib.EXPORTS
    L = _lib.load()                      # (load() itself insists on every name of EXPORTS)
    assert hasattr(L, "pcgrl_render")
    fields = struct_fields("pcgrl_render_desc", _C_TYPES)
    assert [n for n, _ in fields] == ["indices", "count", "tiles", "tile_size", "border_x", "border_y", "border_tile", "cursor",
                                      "grid_rows", "grid_cols", "out"]
    assert [n for n, _ in _lib.RenderDesc._fields_] == [n for n, _ in fields]

    class FromHeader(C.Structure):
        _fields_ = fields
    assert C.sizeof(_lib.RenderDesc) == C.sizeof(FromHeader)
    for n, t in fields:
        mirrored = getattr(_lib.RenderDesc, n)
        assert mirrored.offset == getattr(FromHeader, n).offset and mirrored.size == C.sizeof(t), n
    assert L.pcgrl_render.argtypes == [C.c_void_p, C.POINTER(_lib.RenderDesc), C.c_void_p]
    assert L.pcgrl_render(None, None, None) == _lib.PCGRL_ESTATE       # no handle: refused, nothing touched


def test_abi_version_stays_15():
    from gym_pcgrl_amd import _lib
    assert _lib.load().pcgrl_abi_version() == _lib.ABI_VERSION == 15       # an addition within the version: found by its symbol


def test_grid_shape_rule():
    from gym_pcgrl_amd.rendering import grid_shape, picture_shape, resolve_grid
    want = {1: (1, 1), 2: (2, 1), 3: (2, 2), 4: (2, 2), 5: (3, 2), 16: (4, 4), 17: (5, 4)}      # ceil(sqrt(K)), ceil(K / rows)
    for k, shape in want.items():
        assert grid_shape(k) == shape, k
        assert shape[0] * shape[1] >= k
    for k in range(1, 300):              # the rule, in floating point as stable-baselines' tile_images computes it
        rows = int(__import__("math").ceil(k ** 0.5))
        assert grid_shape(k) == (rows, -(-k // rows)), k
    with pytest.raises(ValueError):
        grid_shape(0)
    assert resolve_grid(None, 5) is None and resolve_grid(True, 5) == (3, 2) and resolve_grid((1, 5), 5) == (1, 5)
    for bad in ((2, 2), (0, 5), (5, 0)):
        with pytest.raises(ValueError):
            resolve_grid(bad, 5)
    assert picture_shape(14, 14, (1, 1), 16, 5) == (5, 256, 256, 3)
    assert picture_shape(14, 114, (3, 0), 16, 2) == (2, 224, 1920, 3)
    assert picture_shape(14, 14, (1, 1), 16, 5, (3, 2)) == (768, 512, 3)


def test_render_kernel_uses_no_scratch():
    """The core part of csrc/pcgrl_abi.hip compiled to gfx950 assembly: both forms of k_render report no private segment."""
    seen = {name: scratch for name, (_, _, scratch) in kernel_resources(0).items() if name.startswith("void k_render<")}
    assert len(seen) == 2, sorted(seen)
    assert all(v == 0 for v in seen.values()), seen
