"""Batched level pictures drawn on the device (pcgrl_render, BatchedPcgrlEnv.render_batch, BatchedVecEnv.get_images / render).

The yardstick is the host render("rgb_array", index) this package already had (tests/test_host_cpu.py pins its layout to the
reference's); one small case is also held against a picture built pixel by pixel in this file.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
RED = (255, 0, 0)


def _torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _make(prob, rep, n, seed=3, **adjust):
    from gym_pcgrl_amd.envs import BatchedPcgrlEnv
    env = BatchedPcgrlEnv(prob=prob, rep=rep, num_envs=n, seed=seed, device="cuda:0")
    if adjust:
        env.adjust_param(**adjust)
    env.reset()
    return env


def _host(env, idx):
    return np.stack([np.asarray(env.render("rgb_array", index=int(i))) for i in idx])


def _prefilled(torch, shape):
    return torch.full(shape, 0xAB, dtype=torch.uint8, device="cuda:0")


def _pixel_by_pixel(m, pos, ts, border, border_id, ntiles):
    """The picture of one map with the grey palette, one pixel at a time: nothing shared with render() but the rules."""
    H, W = m.shape
    bx, by = border
    img = np.zeros(((H + 2 * by) * ts, (W + 2 * bx) * ts, 3), np.uint8)
    for Y in range(img.shape[0]):
        for X in range(img.shape[1]):
            ty, tx = Y // ts - by, X // ts - bx
            t = int(m[ty, tx]) if (0 <= ty < H and 0 <= tx < W) else border_id
            img[Y, X] = t * 255 // ntiles
            if pos is not None and (tx, ty) == tuple(pos):
                py, px = Y % ts, X % ts
                if py < 2 or py >= ts - 2 or px < 2 or px >= ts - 2:
                    img[Y, X] = RED
    return img


def test_cursor_on_every_edge_and_every_byte_written():
    torch = _torch()
    env = _make("binary", "narrow", 5)
    W = H = 14
    cursors = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (5, 7)]
    env._bufs["pos"].copy_(torch.tensor(cursors, dtype=torch.uint8))
    out = _prefilled(torch, (5, 256, 256, 3))
    got = env.render_batch(out=out)
    assert got is out
    got = got.cpu().numpy()
    assert np.array_equal(got, _host(env, range(5)))
    m = env._bufs["map"].cpu().numpy()
    for i in (1, 4):
        assert np.array_equal(got[i], _pixel_by_pixel(m[i], cursors[i], 16, (1, 1), 1, 2)), i
    # the frame really is where the cursors were put: the top-left pixel of each cursor cell, inside the one-tile border
    for i, (x, y) in enumerate(cursors):
        assert tuple(got[i, (y + 1) * 16, (x + 1) * 16]) == RED
    env.close()


@pytest.mark.parametrize("graphics", ["drawn", "random"])
def test_no_cursor_many_tiles_non_square(graphics):
    torch = _torch()
    env = _make("zelda", "wide", 3, width=11, height=16)
    rs = np.random.RandomState(5)
    if graphics == "drawn":
        env.set_graphics("drawn")
    else:      # (values below 255: no picture holds a red pixel)
        env.set_graphics({t: rs.randint(0, 255, size=(16, 16, 3)).astype(np.uint8) for t in env._prob.tiles})
    got = env.render_batch(out=_prefilled(torch, (3, 18 * 16, 13 * 16, 3))).cpu().numpy()
    assert np.array_equal(got, _host(env, range(3)))
    pal = np.stack([np.asarray(env._graphics[t], np.uint8)[:16, :16, :3] for t in env._prob.tiles])
    if graphics == "random":
        assert not (pal == np.array(RED, np.uint8)).all(-1).any()
    if not (pal == np.array(RED, np.uint8)).all(-1).any():          # no cursor: no red pixel the palette does not have
        assert not (got == np.array(RED, np.uint8)).all(-1).any()
    # set_graphics drops the cached palette: back to grey, then nothing of the pictures is left
    env.set_graphics(None)
    grey = env.render_batch().cpu().numpy()
    assert np.array_equal(grey, _host(env, range(3))) and not np.array_equal(grey, got)
    env.close()


def test_smb_border_three_by_zero():
    torch = _torch()
    env = _make("smb", "narrow", 2)
    got = env.render_batch(out=_prefilled(torch, (2, 14 * 16, 120 * 16, 3))).cpu().numpy()
    assert np.array_equal(got, _host(env, range(2)))
    env.close()


@pytest.mark.parametrize("ts,dict_graphics", [(5, False), (32, True), (48, False), (7, True)])
def test_other_tile_sizes(ts, dict_graphics):
    """5 and 7: nothing is aligned (the byte path); 32 and 48: 16-byte pieces with six / nine pieces a tile row."""
    torch = _torch()
    env = _make("binary", "turtle", 2, width=6, height=3)
    env._prob._tile_size = 16
    first = env.render_batch().cpu().numpy()                 # (a palette for 16-pixel tiles is cached now)
    assert first.shape == (2, 5 * 16, 8 * 16, 3)
    env._prob._tile_size = ts
    if dict_graphics:
        rs = np.random.RandomState(ts)
        env.set_graphics({t: rs.randint(0, 256, size=(ts, ts, 3)).astype(np.uint8) for t in env._prob.tiles})
    got = env.render_batch(out=_prefilled(torch, (2, 5 * ts, 8 * ts, 3))).cpu().numpy()
    assert np.array_equal(got, _host(env, range(2)))
    grid = env.render_batch(grid=(1, 2), out=_prefilled(torch, (5 * ts, 16 * ts, 3))).cpu().numpy()
    assert np.array_equal(grid, np.concatenate([got[0], got[1]], axis=1))
    env.close()


def test_sixty_four_pixel_tiles_palette_beyond_64k():
    """zelda's eight tiles at 64 pixels: a 98 KB palette in the block's local memory."""
    torch = _torch()
    env = _make("zelda", "narrow", 2)
    env._prob._tile_size = 64
    rs = np.random.RandomState(64)
    env.set_graphics({t: rs.randint(0, 256, size=(64, 64, 3)).astype(np.uint8) for t in env._prob.tiles})
    got = env.render_batch(out=_prefilled(torch, (2, 9 * 64, 13 * 64, 3))).cpu().numpy()
    assert np.array_equal(got, _host(env, range(2)))
    env.close()


@pytest.mark.parametrize("ts", [1, 2])
def test_tiny_tiles_clip_the_cursor_frame(ts):
    torch = _torch()
    env = _make("binary", "narrow", 4, width=3, height=3)
    env._prob._tile_size = ts
    env._bufs["pos"].copy_(torch.tensor([(0, 0), (2, 2), (1, 1), (2, 0)], dtype=torch.uint8))
    got = env.render_batch(out=_prefilled(torch, (4, 5 * ts, 5 * ts, 3))).cpu().numpy()
    assert np.array_equal(got, _host(env, range(4)))
    assert (got[2, ts * 2:ts * 3, ts * 2:ts * 3] == np.array(RED, np.uint8)).all()      # the whole cursor cell is frame
    env.close()


def test_indices_order_repeats_and_out_of_range():
    torch = _torch()
    N = 5
    env = _make("binary", "narrow", N)
    host = _host(env, range(N))
    for dtype in (torch.int32, torch.int64):
        idx = torch.tensor([4, 0, 0, 2, N, -1], dtype=dtype, device="cuda:0")
        got = env.render_batch(idx, out=_prefilled(torch, (6, 256, 256, 3))).cpu().numpy()
        assert np.array_equal(got[:4], host[[4, 0, 0, 2]])
        assert not got[4:].any()
    assert np.array_equal(env.render_batch([3, 3, 1]).cpu().numpy(), host[[3, 3, 1]])
    assert np.array_equal(env.render_batch(np.array([2, 4])).cpu().numpy(), host[[2, 4]])
    for bad in ([4, 0, N], [0, -1], np.array([N])):
        with pytest.raises(IndexError):
            env.render_batch(bad)
    env.close()


def test_grid_layouts():
    torch = _torch()
    env = _make("binary", "narrow", 5)
    stacked = env.render_batch().cpu().numpy()
    assert np.array_equal(stacked, _host(env, range(5)))
    sheet = env.render_batch(grid=True, out=_prefilled(torch, (3 * 256, 2 * 256, 3))).cpu().numpy()
    for k in range(6):
        cell = sheet[(k // 2) * 256:(k // 2 + 1) * 256, (k % 2) * 256:(k % 2 + 1) * 256]
        assert np.array_equal(cell, stacked[k]) if k < 5 else not cell.any(), k
    row = env.render_batch(grid=(1, 5), out=_prefilled(torch, (256, 5 * 256, 3))).cpu().numpy()
    assert np.array_equal(row, np.concatenate(list(stacked), axis=1))
    col = env.render_batch(grid=(5, 1), out=_prefilled(torch, (5 * 256, 256, 3))).cpu().numpy()
    assert np.array_equal(col, np.concatenate(list(stacked), axis=0))
    with pytest.raises(ValueError):
        env.render_batch(grid=(2, 2))
    env.close()


def test_offsets_beyond_four_gigabytes():
    """540 pictures of a 100 x 100 map are 4.31 GB: picture 268 lies across byte 2^31, picture 537 across byte 2^32."""
    torch = _torch()
    if torch.cuda.mem_get_info(0)[0] < 6 * 2 ** 30:
        pytest.skip("needs 6 GB of free device memory")
    env = _make("binary", "narrow", 3, width=100, height=100)
    per = 1632 * 1632 * 3
    assert per == 7990272 and 268 * per < 2 ** 31 < 269 * per and 537 * per < 2 ** 32 < 538 * per
    idx = (torch.arange(540, device="cuda:0") % 3).to(torch.int32)
    out = env.render_batch(idx)
    assert tuple(out.shape) == (540, 1632, 1632, 3)
    host = _host(env, range(3))
    for k in (0, 268, 537, 539):
        assert np.array_equal(out[k].cpu().numpy(), host[k % 3]), k
    del out
    env.close()


def test_live_state_across_auto_resets():
    torch = _torch()
    N = 64
    env = _make("binary", "narrow", N, change_percentage=0.03)       # (five changes end an episode)
    rs = np.random.RandomState(8)
    dones = 0
    for _ in range(30):
        _, _, done, _ = env.step(torch.as_tensor(rs.randint(0, 3, size=N).astype(np.int32), device="cuda:0"))
        dones += int(done.sum())
    assert dones > 0
    assert np.array_equal(env.render_batch().cpu().numpy(), _host(env, range(N)))
    env.close()


def test_vec_env_get_images_and_render():
    _torch()
    from gym_pcgrl_amd.utils import make_vec_envs
    venv = make_vec_envs("binary-narrow-v0", "narrow", n_cpu=20, seed=5, device="cuda:0", render=True)
    venv.reset()
    env = venv.env.pcgrl_env
    host = _host(env, range(20))
    assert np.array_equal(venv.get_images().cpu().numpy(), host)
    assert np.array_equal(venv.get_images([7, 19]).cpu().numpy(), host[[7, 19]])
    sheet = venv.render().cpu().numpy()                           # the first 16 on a 4 x 4 sheet
    assert sheet.shape == (4 * 256, 4 * 256, 3)
    for k in range(16):
        assert np.array_equal(sheet[(k // 4) * 256:(k // 4 + 1) * 256, (k % 4) * 256:(k % 4 + 1) * 256], host[k]), k
    assert np.array_equal(venv.render("human", indices=[1, 2]).cpu().numpy(), np.concatenate([host[1], host[2]], axis=0))
    venv.close()


def test_rejected_arguments():
    torch = _torch()
    from gym_pcgrl_amd import _lib
    env = _make("binary", "narrow", 2)
    shape, nbytes = (2, 256, 256, 3), 2 * 256 * 256 * 3
    flat = torch.zeros(nbytes + 16, dtype=torch.uint8, device="cuda:0")
    bad = [torch.zeros((2, 256, 256, 4), dtype=torch.uint8, device="cuda:0"),              # wrong shape
           torch.zeros(shape, dtype=torch.int8, device="cuda:0"),                           # wrong dtype
           torch.zeros((2, 256, 256, 6), dtype=torch.uint8, device="cuda:0")[..., ::2],     # not contiguous
           flat[1:1 + nbytes].view(shape),                                                  # off by one byte
           torch.zeros(shape, dtype=torch.uint8)]                                           # wrong device
    for out in bad:
        with pytest.raises(ValueError):
            env.render_batch(out=out)
    assert not flat.any()
    # the library's own checks, through ctypes
    L, pal, out = env._lib, env._render_palette(), torch.zeros(shape, dtype=torch.uint8, device="cuda:0")

    def desc(**kw):
        d = _lib.RenderDesc(None, 2, pal.data_ptr(), 16, 1, 1, 1, 1, 0, 0, out.data_ptr())
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    assert L.pcgrl_render(env._handle, C.byref(desc()), env._stream()) == _lib.PCGRL_OK
    for kw in (dict(tiles=None), dict(out=None), dict(count=0), dict(tile_size=0), dict(tile_size=65), dict(border_tile=2), dict(border_tile=-1),
               dict(grid_rows=1, grid_cols=1), dict(grid_rows=2, grid_cols=0), dict(out=out.data_ptr() + 1)):
        assert L.pcgrl_render(env._handle, C.byref(desc(**kw)), env._stream()) == _lib.PCGRL_EINVAL, kw
    assert L.pcgrl_render(env._handle, None, env._stream()) == _lib.PCGRL_EINVAL
    env.close()
    wide = _make("binary", "wide", 2)
    assert L.pcgrl_render(wide._handle, C.byref(desc()), wide._stream()) == _lib.PCGRL_EINVAL         # a cursor frame without a cursor
    assert L.pcgrl_render(wide._handle, C.byref(desc(cursor=0)), wide._stream()) == _lib.PCGRL_OK
    wide.close()
    # before the first reset: a bound handle, no state to draw
    from gym_pcgrl_amd.envs import BatchedPcgrlEnv
    fresh = BatchedPcgrlEnv(prob="binary", rep="narrow", num_envs=2, seed=1, device="cuda:0")
    with pytest.raises(RuntimeError):
        fresh.render_batch()
    fresh._allocate()
    assert L.pcgrl_render(fresh._handle, C.byref(desc()), fresh._stream()) == _lib.PCGRL_ESTATE
    fresh.close()
    torch.cuda.synchronize()
