"""The wrapped observation (gym_pcgrl_amd/csrc/kernels_obs.h) for the tests that need no GPU and the ones that do: the rule every
image follows (expected_image), the route an image takes through the library (lean_mode, routine, route) and the table of cases --
windows, map widths, pad values -- at which the hand-made arithmetic of the routines can go wrong (CASES).  No GPU, no library."""
import collections

import numpy as np

# ------------------------------------------------------------------ the rule


def expected_image(m, pos, oh, ow, centered, pad, depth):
    """The image of the reference's composite wrappers -- Cropped (pad with the border tile, window of the given size at the cursor),
    OneHotEncoding, ToImage -- for every environment at once: m uint8 [N, H, W], pos [N, 2] = (x, y) -> uint8 [N, oh, ow, depth].
    The same contract as _expected_image of tests/test_gpu_parity.py, which restates wrappers.py with np.pad environment by
    environment; tests/test_obs_host.py holds this form against that one on every case of the table.  Here: index grids clipped
    into the map plus a mask of the cells outside it."""
    m = np.asarray(m)
    n, H, W = m.shape
    if centered:
        pos = np.asarray(pos).astype(np.int64)
        oy, ox = pos[:, 1] - oh // 2, pos[:, 0] - ow // 2
    else:
        oy = ox = np.zeros(n, np.int64)
    y = oy[:, None] + np.arange(oh)[None, :]                      # [N, oh]
    x = ox[:, None] + np.arange(ow)[None, :]                      # [N, ow]
    outside = ((y < 0) | (y >= H))[:, :, None] | ((x < 0) | (x >= W))[:, None, :]
    img = m[np.arange(n)[:, None, None], np.clip(y, 0, H - 1)[:, :, None], np.clip(x, 0, W - 1)[:, None, :]]
    img = np.where(outside, np.uint8(pad), img).astype(np.uint8)
    if depth == 1:
        return img[..., None]
    return (img[..., None] == np.arange(depth, dtype=np.uint8)).astype(np.uint8)      # (a pad value >= depth: no plane set, as np.eye cannot say)


# ------------------------------------------------------------------ the routes
OBS_EPB = 64             # kernels_obs.h: environments per block of k_obs
NTILES = dict(binary=2, zelda=8, sokoban=5, mdungeon=8, ddave=7, smb=7)       # pcgrl_abi.hip ntiles_of
FUSED_REPS = ("narrow", "wide", "turtle")                                      # PCGRL_REP_NARROW .. PCGRL_REP_TURTLE


def prob_planes(prob, W, H):
    """(problem, row bit planes an environment keeps): pcgrl_abi.hip fill_params -- none for smb and for maps beyond 64 x 64, one for
    binary, three for the others."""
    return prob, (0 if (prob == "smb" or W > 64 or H > 64) else (1 if prob == "binary" else 3))


def lean_mode(nplanes, word32, W, oh, ow, depth, pad):
    """kernels_obs.h obs_lean_mode, on numbers or numpy arrays: 0 the general routine, 1 rows (binary tile ids), 2 one-hot over eight
    tiles.  tests/test_obs_host.py pins it against the C function over the whole grid."""
    cells = oh * ow
    ok = ((cells * depth) % 16 == 0) & (cells <= 4096)
    rows = (nplanes == 1) & (depth == 1) & (ow >= 16) & (ow <= 32) & (W <= np.where(word32, 32, 64)) & (pad <= 1)
    hot8 = (nplanes == 3) & word32 & (depth == 8) & (ow <= 64) & (pad <= 7)
    return np.where(ok & rows, 1, np.where(ok & hot8, 2, 0))


def is_huge(oh, ow, depth):
    """pcgrl_abi.hip obs_is_huge: a block's stretch of k_obs would pass 2^22 bytes."""
    return OBS_EPB * oh * ow * depth >= (1 << 24) // 4


def routine(prob_planes, word_bits, W, oh, ow, depth, pad):
    """The routine of kernels_obs.h a (non-huge) image is made by: "general", "rows" or "hot8"."""
    return ("general", "rows", "hot8")[int(lean_mode(prob_planes[1], word_bits == 32, W, oh, ow, depth, pad))]


def route(prob_planes, word_bits, W, H, rep, oh, ow, depth, pad, stepping):
    """The kernel that writes an image, and for the fused step kernel the routine it writes it with: "huge", "k_obs0" .. "k_obs3",
    "fused_rows32", "fused_rows64", "fused_hot8", "fused_delta".  prob_planes: prob_planes(); word_bits: 32 for maps of at most 32
    columns, else 64 (fill_params: mask_bytes); stepping: None -- pcgrl_observe, pcgrl_reset, pcgrl_set_maps: always the stand-alone
    kernels --, "step" -- a bound image behind pcgrl_step / pcgrl_rollout --, "incremental" -- the same, bound with incremental = 1
    and the target holding the previous state's image.
    Which configurations step with the fused kernel: pcgrl_abi.hip step_one asks fused_step_applies(h) -- binary or zelda, 16-lane
    groups (at most 16 rows), no map beyond 64 x 64, a representation up to PCGRL_REP_TURTLE, auto_reset with inline resets (the
    defaults) --, and step_impl launches k_obs behind the step unless ObsSpec::fused, which obs_spec sets from obs_lean_mode.  Inside
    k_step (kernels_step.h) the wide representation with three planes writes one piece where ObsSpec::delta is set (step_impl:
    incremental, not held, the target in sync)."""
    prob, nplanes = prob_planes
    if stepping is not None:
        mode = int(lean_mode(nplanes, word_bits == 32, W, oh, ow, depth, pad))
        fused_step = prob in ("binary", "zelda") and H <= 16 and W <= 64 and rep in FUSED_REPS
        if fused_step and mode == 1:
            return "fused_rows%d" % word_bits
        if fused_step and mode == 2:
            return "fused_delta" if (rep == "wide" and stepping == "incremental") else "fused_hot8"
    # launch_obs
    if is_huge(oh, ow, depth):
        return "huge"
    if nplanes == 1 and depth == 1:
        return "k_obs1" if word_bits == 32 else "k_obs2"
    if nplanes == 3 and word_bits == 32 and depth == 8:
        return "k_obs3"
    return "k_obs0"


ROUTES = ("huge", "k_obs0", "k_obs1", "k_obs2", "k_obs3", "fused_rows32", "fused_rows64", "fused_hot8", "fused_delta")

# ------------------------------------------------------------------ the table
# family: which list of the issue the case belongs to; rep: the representation the device tests take for it; stepping / route / routine
# as route() and routine() say (worked out below, asserted by tests/test_obs_host.py to cover every route).
Case = collections.namedtuple("Case", "family prob rep H W oh ow centered onehot pad stepping route routine")


def _case(family, prob, rep, H, W, oh, ow, centered, onehot, pad, stepping):
    pp = prob_planes(prob, W, H)
    bits = 32 if W <= 32 else 64
    depth = NTILES[prob] if onehot else 1
    r = route(pp, bits, W, H, rep, oh, ow, depth, pad, stepping)
    return Case(family, prob, rep, H, W, oh, ow, centered, onehot, pad, stepping, r, "huge" if r == "huge" else routine(pp, bits, W, oh, ow, depth, pad))


def depth_of(c):
    return NTILES[c.prob] if c.onehot else 1


ROWS_WINDOWS = ((1, 16), (1, 32), (16, 16), (16, 17), (16, 31), (32, 32), (128, 32))
ROWS_FALL = ((16, 15), (16, 33))                      # beside the 16 <= ow <= 32 rule: the general routine, the same image
# (H, W): every width of the issue with a fused height (3, 16) and one for k_obs (17, 64)
ROWS_MAPS = ((3, 5), (16, 16), (3, 31), (16, 32), (16, 33), (3, 48), (16, 63), (3, 64),
             (17, 5), (64, 16), (17, 31), (64, 32), (17, 33), (64, 48), (17, 63), (64, 64))
HOT8_WINDOWS = ((2, 1), (1, 2), (8, 12), (6, 8), (8, 9), (63, 64), (64, 64), (7, 11))
HOT8_PADS = (0, 1, 3, 4, 7)
HOT8_MAPS = (("zelda", 4, 3), ("zelda", 7, 11), ("zelda", 16, 32), ("mdungeon", 7, 11), ("mdungeon", 5, 32))
GENERAL_WINDOWS = ((1, 1), (3, 1), (5, 1), (1, 3), (3, 5))
DELTA_WINDOWS = ((7, 11, (7, 11)), (7, 11, (8, 12)), (7, 11, (6, 8)), (7, 11, (8, 9)), (16, 11, (16, 11)))      # (H, W, window)


def _build():
    cases = []
    # binary rows: bound to a turtle that steps where the map has at most 16 rows (the fused kernel), observed elsewhere (k_obs)
    for H, W in ROWS_MAPS:
        stepping = "step" if H <= 16 else None
        for oh, ow in ROWS_WINDOWS:
            for centered in (1, 0):
                for pad in (0, 1):
                    cases.append(_case("rows", "binary", "turtle", H, W, oh, ow, centered, 0, pad, stepping))
        for oh, ow in ROWS_FALL:
            cases.append(_case("rows_fall", "binary", "turtle", H, W, oh, ow, 1, 0, 1, stepping))
        cases.append(_case("rows_fall", "binary", "turtle", H, W, 16, 16, 1, 0, 2, stepping))          # a pad value the rows routine does not hold
    # one-hot over eight tiles: zelda (fused) and mdungeon (k_obs<3>)
    for prob, H, W in HOT8_MAPS:
        stepping = "step" if prob == "zelda" else None
        for oh, ow in HOT8_WINDOWS:
            for centered in (1, 0):
                for pad in (HOT8_PADS if oh * ow <= 100 else (0, 4, 7)):
                    cases.append(_case("hot8", prob, "turtle", H, W, oh, ow, centered, 1, pad, stepping))
    # the general routine: one-column and other tiny windows, tile ids and one-hot, plane sources and byte maps.  On the device a batch
    # of H * W environments: 3 x 5 = 15 environments of (3, 5) x 5 = 75 bytes is 1125 bytes, no multiple of 16, one partial block
    for prob, H, W in (("binary", 3, 5), ("binary", 17, 33), ("zelda", 7, 11), ("sokoban", 5, 5), ("smb", 6, 12)):
        for oh, ow in GENERAL_WINDOWS:
            for onehot in (0, 1):
                for centered in (1, 0):
                    cases.append(_case("general", prob, "narrow", H, W, oh, ow, centered, onehot, 1 if prob == "binary" else 3, None))
    # k_obs against k_obs_huge: 65 536 bytes an image is the first size of the 64-bit stream, 65 535 the last of k_obs
    cases.append(_case("huge", "binary", "narrow", 20, 30, 256, 256, 1, 0, 1, None))
    cases.append(_case("huge", "binary", "narrow", 20, 30, 255, 257, 1, 0, 1, None))
    # the wide representation's map image, updated in place -- and written whole beside it.  (The 7 x 11 map itself, one-hot, is 616
    # bytes: no multiple of 16, so it has no lean routine and k_obs<3> writes it behind the step, whole, with the general routine.)
    for H, W, (oh, ow) in DELTA_WINDOWS:
        for stepping in ("incremental", "step"):
            cases.append(_case("delta", "zelda", "wide", H, W, oh, ow, 0, 1, 1, stepping))
    return tuple(cases)


CASES = _build()


def case_id(c):
    return "%s-%s-%s-%dx%d-w%dx%d-c%d-h%d-p%d-%s-%s" % (c.family, c.prob, c.rep, c.H, c.W, c.oh, c.ow, c.centered, c.onehot, c.pad, c.stepping or "observe", c.route)


def windows(cases):
    """The distinct windows of some cases, in the table's order (a window may stand in the table under several steppings)."""
    out = {}
    for c in cases:
        out.setdefault((c.oh, c.ow, c.centered, c.onehot, c.pad), c)
    return list(out.values())


# (problem, H, W, huge windows?): a handle each in the device test of pcgrl_observe
OBSERVE_SHAPES = sorted({(c.prob, c.H, c.W, c.route == "huge") for c in CASES})
# the map shapes whose turtle (and narrow) steps write images with the fused kernel's routines
FUSED_SHAPES = sorted({(c.prob, c.H, c.W) for c in CASES if c.route in ("fused_rows32", "fused_rows64", "fused_hot8") and c.rep == "turtle"})
NARROW_ENVS, NARROW_STEPS = 70, 30


def narrow_plan(prob, H, W):
    """(windows, seed, tape [steps x windows, NARROW_ENVS]) of the device test of the narrow representation for one map shape
    (tests/test_gpu_obs_windows.py); tests/test_obs_host.py walks the same tape on the oracle to see that its cursors reach the four
    corners of the map."""
    cases = windows(c for c in CASES if (c.prob, c.H, c.W) == (prob, H, W) and c.rep == "turtle" and c.stepping == "step")
    tape = np.random.RandomState(900 + H * 64 + W).randint(0, NTILES[prob], size=(NARROW_STEPS * len(cases), NARROW_ENVS)).astype(np.int32)
    return cases, 700 + H * 64 + W, tape


# ------------------------------------------------------------------ inputs
def seeded_maps(n, H, W, ntiles, seed):
    """n random maps, then -- appended -- five all-0 and five all-max-tile maps: uint8 [n + 10, H, W]."""
    rs = np.random.RandomState(seed)
    m = rs.randint(0, ntiles, size=(n + 10, H, W)).astype(np.uint8)
    m[n:n + 5] = 0
    m[n + 5:] = ntiles - 1
    return m


def every_cursor(H, W, extra=10):
    """[H * W + extra, 2] = (x, y): environment i on cell i, the extra ones on the four corners and the middle, twice."""
    cells = np.arange(H * W)
    pos = np.stack([cells % W, cells // W], -1)
    five = np.array([[0, 0], [W - 1, 0], [0, H - 1], [W - 1, H - 1], [W // 2, H // 2]])
    return np.concatenate([pos] + [five] * (extra // 5)).astype(np.uint8)
