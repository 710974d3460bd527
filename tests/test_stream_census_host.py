"""The census of tests/test_gpu_stream_edges.py, without a GPU: which of the MT19937 draw paths' rarely taken branches every case
of tests/stream_model.py reaches, counted by the numpy stream model and the oracle alone.

A floor, not a measurement: on every route a case is run on, every event class that applies occurs at least 3 times, in at least 2
environments, within the steps (and the reset() calls behind them) the GPU test runs.  A class that cannot occur on a case, or that
the largest case allowed (512 environments x 60 steps) would not reach, is listed with its reason (stream_model.applicable) and not
left out silently.  While the traces are made the model's ring cursor and cursor position are asserted against the oracle's at every
step (stream_model.trace_steps / trace_resets).  `pytest -s` prints the table: per (case, route) the count of every class and the
listed exclusions; `python tests/stream_model.py` prints it too."""
import numpy as np
import pytest

import stream_model as sm


@pytest.mark.parametrize("name", [c.name for c in sm.CASES])
def test_every_class_of_the_route_meets_the_floor(name):
    case = sm.CASE[name]
    assert case.E <= sm.MAX_ENVS and case.T <= sm.MAX_STEPS
    bad = []
    for route in sm.routes_of(case):
        rows, missing = sm.check_floor(case, route)
        print(sm.format_table(case, route, rows))
        for cls, n, ne, why in rows:
            assert why is None or isinstance(why, str) and why, (name, route, cls)
            if why is not None and why.startswith("cannot occur"):
                assert n == 0, ("a class listed as impossible occurred", name, route, cls, n)
        bad += [(route,) + m for m in missing]
    assert not bad, "%s: classes below the floor of %d occurrences in %d environments: %s" % (name, sm.FLOOR_COUNT, sm.FLOOR_ENVS, bad)


def test_the_model_is_numpys_stream():
    """StreamModel against plain numpy calls on the golden generator states (tests/golden/rng.npz: written from the reference's
    RandomState): words counted per draw, the cursor, and the lazy-ring image after a partial and after several whole laps."""
    import os
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rng.npz"))
    for si, seed in enumerate(d["seeds"][:3]):
        m = sm.StreamModel(int(seed), 9, 5, "narrow")
        assert np.array_equal(m.ring_image(), d["mt_key"][si])
        rs = np.random.RandomState()
        rs.set_state(("MT19937", d["mt_key"][si], 624))
        for k in range(40):
            c0, nmap, draw = m.reset()
            rs.random_sample((5, 9))
            x, y = rs.randint(9), rs.randint(5)
            assert draw[3:] == (x, y) and nmap == 90 and draw[0] == (c0 + 90) % 624
            assert m.cursor == rs.get_state()[2] % 624
            c, kx, ky, x2, y2 = m.step()
            assert (x2, y2) == (rs.randint(9), rs.randint(5)) and kx >= 1 and ky >= 1
            assert m.cursor == rs.get_state()[2] % 624 == (c + kx + ky) % 624
            # the lazy ring: the slots below the cursor are numpy's current block, the others the block before
            img, key = m.ring_image(), np.asarray(rs.get_state()[1], dtype=np.uint32)
            cur = m.cursor
            assert np.array_equal(img[:cur], key[:cur])
            if cur:
                prev = sm.StreamModel(int(seed), 9, 5, "narrow")
                prev.words = m.words - cur
                assert np.array_equal(img[cur:], prev.ring_image()[cur:])
        assert m.words > 3 * 624


def test_case_table_routes_and_thresholds():
    """The shapes the table promises: the partial-staging threshold on both sides, with and without a draw cache; the word counts of
    the block reset's rounds; every route present."""
    c = sm.CASE
    assert sm.is_partial(c["zelda-turtle-12x9"]) and not sm.is_partial(c["zelda-turtle-11x10"])
    assert sm.need_words(c["zelda-turtle-12x9"]) + 2 == 226
    assert sm.is_partial(c["binary-narrow-17x6"]) and not sm.is_partial(c["binary-narrow-13x8"])
    assert sm.need_words(c["binary-narrow-17x6"]) + 2 == 223
    assert sm.is_partial(c["binary-narrow-65x1"]) and sm.is_partial(c["binary-narrow-17x3"]) and sm.is_partial(c["sokoban-narrow-5x5"])
    assert [2 * c[n].w * c[n].h % 454 for n in ("binary-narrow-12x19", "binary-narrow-17x20", "binary-narrow-11x31", "binary-narrow-6x19")] == [2, 226, 228, 228]
    assert {x.route for x in sm.CASES} == {"fused", "block", "big", "solver", "smb"}
    for x in sm.CASES:
        assert x.route != "fused" or (x.h <= 16 and x.w <= 64 and x.prob in ("binary", "zelda"))
        assert x.route != "block" or (x.h > 16 and x.prob == "binary" and x.w <= 64 and x.h <= 64)
        assert x.route != "big" or x.w > 64 or x.h > 64
