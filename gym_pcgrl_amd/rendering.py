"""Layout rules of the batched level pictures (BatchedPcgrlEnv.render_batch, include/pcgrl_hip.h pcgrl_render): pure functions,
no device needed."""
import math


def grid_shape(count):
    """(rows, cols) of the contact sheet of `count` pictures -- stable-baselines' tile_images rule, which the reference's
    VecEnv.render goes through: rows = ceil(sqrt(count)), cols = ceil(count / rows)."""
    count = int(count)
    if count < 1:
        raise ValueError("a grid of %d pictures" % count)
    rows = math.isqrt(count - 1) + 1          # ceil(sqrt(count)) in integers
    return rows, -(-count // rows)


def resolve_grid(grid, count):
    """render_batch's `grid` argument -> (rows, cols), or None for stacked pictures.  True: grid_shape(count); a pair: as given,
    ValueError when it has fewer cells than pictures."""
    if grid is None or grid is False:
        return None
    if grid is True:
        return grid_shape(count)
    rows, cols = (int(v) for v in grid)
    if rows < 1 or cols < 1 or rows * cols < count:
        raise ValueError("grid %r has fewer cells than the %d pictures" % (tuple(grid), count))
    return rows, cols


def picture_shape(height, width, border, tile_size, count, grid=None):
    """Shape of render_batch's result: map of height x width cells, border = (border_x, border_y) cells, grid = None or (rows, cols)."""
    bx, by = border
    hp, wp = (int(height) + 2 * int(by)) * int(tile_size), (int(width) + 2 * int(bx)) * int(tile_size)
    return (int(count), hp, wp, 3) if grid is None else (grid[0] * hp, grid[1] * wp, 3)
