"""A given-up champion update resumes from what binary_touch found (csrc/pcgrl_algos.h rlp_resume; pcgrl_tuning touch_resume) --
every step of the binary problem against the oracle with the switch on and off: the three single-cell representations on the
flagship's 14 x 14 map, as single steps and as one pcgrl_rollout tape, every block size of the fused step kernel, the two-launch
pipeline and 64-bit row masks (16 x 40) -- both of which keep the restart whatever the switch says (k_stats is handed no touch; the
64-bit step kernels have no registers to spare), so these cases pin that the switch is harmless there -- and a 5 x 5 map whose
champion comes and goes.
The oracle's side of a configuration is made once and shared by the runs that use it."""
import numpy as np
import pytest

import parity_harness as ph

SEED0 = 9100
_TAPES = {}


def _tape(rep, calls, E, T):
    key = (rep, repr(calls), E, T)
    if key not in _TAPES:
        _TAPES[key] = ph.oracle_tape("binary", rep, list(calls), E, T, SEED0, np.random.RandomState(31))
    return _TAPES[key]


def _run(rep, calls, E, T, use_rollout, tuning):
    msg = ph.run_config("binary", rep, list(calls), E, T, SEED0, None, use_rollout, tuning=tuning, tape=_tape(rep, calls, E, T))
    assert msg is None, (msg, tuning)


FLAGSHIP = ((), 512, 300)


@pytest.mark.gpu
@pytest.mark.parametrize("resume", [1, 0])
@pytest.mark.parametrize("use_rollout", [False, True], ids=["steps", "rollout"])
@pytest.mark.parametrize("rep", ["narrow", "wide", "turtle"])
def test_flagship_map_every_step(rep, use_rollout, resume):
    _run(rep, *FLAGSHIP, use_rollout, dict(touch_resume=resume))


@pytest.mark.gpu
@pytest.mark.parametrize("resume", [1, 0])
@pytest.mark.parametrize("epb", [64, 128, 256])
def test_block_sizes(epb, resume):
    _run("narrow", *FLAGSHIP, False, dict(touch_resume=resume, step_epb=epb))


@pytest.mark.gpu
@pytest.mark.parametrize("resume", [1, 0])
@pytest.mark.parametrize("rep", ["narrow", "wide"])
def test_two_launch_pipeline(rep, resume):
    _run(rep, *FLAGSHIP, False, dict(touch_resume=resume, no_fused=1))


@pytest.mark.gpu
@pytest.mark.parametrize("resume", [1, 0])
@pytest.mark.parametrize("use_rollout", [False, True], ids=["steps", "rollout"])
def test_64_bit_row_masks(use_rollout, resume):
    _run("wide", (dict(width=40, height=16), dict(change_percentage=0.5)), 96, 200, use_rollout, dict(touch_resume=resume))


@pytest.mark.gpu
@pytest.mark.parametrize("resume", [1, 0])
@pytest.mark.parametrize("use_rollout", [False, True], ids=["steps", "rollout"])
def test_tiny_map(use_rollout, resume):
    _run("narrow", (dict(width=5, height=5), dict(change_percentage=1.0)), 256, 300, use_rollout, dict(touch_resume=resume))
