"""A given-up champion update resumes instead of restarting (pcgrl_algos.h: binary_touch with a memo, rlp_resume), on the CPU
lane-group simulator (tests/hostsim/sim_touch_resume.cpp): random walks of single-cell flips routed the way the step kernels route
them -- incremental, touch, resume on a give-up, the plain computation only for want of a champion -- with regions and path of EVERY
step against the oracle, and the carried state (champion rows, the bound on the other components) checked by brute force inside the
simulator after every step.  CPU only."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_lib as ol
from hostsim_build import build_so
from oracle_lib import _p

HERE = os.path.dirname(os.path.abspath(__file__))
INVARIANT = {1: "the champion is not one whole component", 2: "the champion's double sweep is not the path",
             3: "no champion, but the path is not the tiny components'", 4: "ub2 is below another component's double-sweep value",
             5: "ub2 is unknown or above the path", 6: "the parent's route gives other statistics"}


@pytest.fixture(scope="module")
def sim():
    L = build_so("sim_touch_resume.cpp", ["-ffp-contract=off"])
    L.sim_touch_resume.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.sim_touch_resume.restype = C.c_long
    L.sim_set_spurious.argtypes = [C.c_int]
    return L


def _walk(sim, rs, h, w, dens, T, tot):
    m = (rs.random_sample((h, w)) < dens).astype(np.uint8)
    flips = rs.randint(0, h * w, size=T).astype(np.int32)
    out = np.zeros((T + 1, 2), np.int32)
    counts = np.zeros(8, np.int64)
    sim.sim_set_spurious(int(rs.randint(0, 30)))
    try:
        rc = sim.sim_touch_resume(_p(m), h, w, _p(flips), T, _p(out), _p(counts))
    finally:
        sim.sim_set_spurious(0)
    assert rc == 0, ((h, w), dens, "step %d: %s" % (rc // 8 - 1, INVARIANT[rc % 8]))
    cur = m.copy()
    assert np.array_equal(out[0], ol.get_stats("binary", cur))
    for t in range(T):
        cur.flat[flips[t]] ^= 1
        assert np.array_equal(out[t + 1], ol.get_stats("binary", cur)), ((h, w), dens, t, out[t + 1], ol.get_stats("binary", cur))
    tot += counts
    return counts


def test_touch_resume_walks(sim):
    rs = np.random.RandomState(29)
    tot = np.zeros(8, np.int64)
    steps = 0
    for (h, w) in ((14, 14), (16, 11), (5, 5), (9, 32), (3, 7), (16, 40), (1, 9)):
        for dens in (0.3, 0.5, 0.65):
            for rep in range(2):
                _walk(sim, rs, h, w, dens, 120, tot)
                steps += 120
    # the flagship's shape: as long as it takes for 200 resumed give-ups, removals and additions among them (the parent gives up on
    # about 7 % of the touches there: some 10 000 steps)
    while tot[2] < 200 or tot[3] == 0 or tot[4] == 0:
        assert steps < 60000, tot
        _walk(sim, rs, 14, 14, 0.5, 1000, tot)
        steps += 1000
    inc, touch, resumed, rem, add, plain, p_touch, p_giveup = (int(v) for v in tot)
    print("steps %d: incremental %d, touches %d, resumed %d (removals %d, additions %d), plain %d" % (steps, inc, touch, resumed, rem, add, plain))
    print("give-up rate with the resume's bound %.2f %% (%d / %d); the parent's on the same walks %.2f %% (%d / %d)"
          % (100.0 * resumed / touch, resumed, touch, 100.0 * p_giveup / p_touch, p_giveup, p_touch))
    assert inc > steps // 3                        # the incremental route is the common one
    assert touch > steps // 4 and resumed * 5 < touch, tot
