"""The tapes of test_gpu_block_reps.py hold what they are there for -- asserted on the CPU oracle alone, without a GPU (the host
twin of that module; the cases, the terms and the figures are in block_reps_cases.py).  A tape of 3 x 3 writes proves nothing about
corners, clipped borders, the words a row mask is made of or the step that jumps past max_changes unless it contains them.
`PYTHONPATH=. python tests/test_block_reps_host.py` prints every figure."""
import numpy as np
import pytest

import block_reps_cases as bc


@pytest.mark.parametrize("name", list(bc.A_CASES))
def test_geometry_tape_holds_what_its_case_needs(name):
    """A: the floors of the case (block_reps_cases.A_CASES) on the oracle's rollouts: corners, borders, word-edge columns, nine-cell
    writes, the jump past max_changes, episodes ended, moves outwards at the border."""
    bc.check_case_a(name)


def test_every_change_count_occurs():
    """A: over all cases a step changes 1, 2, ... 9 cells at least once each."""
    bc.check_histogram()


def test_corner_counting_knows_its_maps():
    """The coverage function itself on two tapes written by hand (3 x 2 narrowcast): a block at a corner counts for that corner
    only, a write in the middle of a border for `border`, and a step that changes nothing is no write."""
    case = dict(rep="narrowcast", calls=[dict(width=3, height=2)])
    acts = np.zeros((3, 1, 2), np.int32)

    def x(pos0, pos, changes, done=(False, False, False)):
        info = np.zeros((3, 3), np.int64)
        info[:, -1] = changes
        return dict(pos0=np.array(pos0), pos=np.array(pos), info=info, done=np.array(done), max_changes=4)
    c = bc.coverage(case, acts, [x((0, 0), [(1, 0), (2, 1), (0, 0)], [4, 4, 6])])
    assert (c["corners"], c["border"], c["writes"], c["jump"], c["hist"][4], c["hist"][2], c["hist"][0]) == (2, 0, 2, 0, 1, 1, 1)
    # changes 2 -> 6 with max_changes 4: from < 3 to > 4 in one step; the episode ends, the next step starts from 0
    c = bc.coverage(case, acts, [x((1, 0), [(1, 1), (0, 1), (0, 0)], [2, 6, 1], done=(False, True, False))])
    assert (c["corners"], c["border"], c["writes"], c["jump"], c["done"]) == (1, 2, 3, 1, 1)


@pytest.mark.parametrize("name", list(bc.B_CASES))
def test_past_done_tape_spends_its_steps_past_done(name):
    """B: at least a quarter of the environments take 10 or more steps after their first done (the oracle stepped without reset)."""
    bc.check_case_b(name)


def test_past_done_tapes_run_beyond_max_changes():
    """B: in at least one case `changes` ends more than 8 above max_changes."""
    bc.check_sums_b()


if __name__ == "__main__":
    bc.report()
