"""The helix's ring rows on the CPU: tools/pencil_emu.py replays the kernel's
first-lap role (wave 0 builds the y = 0 face records of its steps before t_sw
from its own H values and fetches the ring only from t_sw on; only the rows of
steps [t_sw, lag) are filled before the first step) with the ring AND the LDS
record slots starting as garbage, as a workspace that an earlier launch used.
A row read before this unit wrote it would spoil the score. The shapes are
those of tests/test_helix_ring_rows.py scaled to the emulator's speed: the
same lap counts, P above the position count and rounded up to a multiple of
4, M = 1 and 2, TWO mode."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

# (la, lb, lc): what the shape exercises
SHAPES = [
    (128, 24, 128),  # several laps
    (128, 8, 128),   # one lap: every row wave 0 reads is a face row
    (100, 3, 125),   # one lap, fewer rows than waves, P = 128 > LA
    (128, 9, 128),   # the second lap is a single row
    (150, 17, 100),  # P = 150 > the 128 positions
    (130, 9, 129),   # M = 2, P = 256
    (261, 9, 129),   # M = 2, P = 264: LA rounded up to a multiple of 4
    (90, 20, 100),   # M = 1, P = 128
    (60, 12, 60),    # short in every dimension (TWO mode, P = 64: test_garbage_ring_two_triples)
]


def _score(orc, t, sop):
    return orc.score(*t, orc.default_params(s3_mode=sop, score_bits=0))


@pytest.mark.parametrize("sop", [0, 1])
@pytest.mark.parametrize("la,lb,lc", SHAPES)
def test_garbage_ring_vspace(orc, la, lb, lc, sop):
    import pencil_emu
    rng = np.random.default_rng(la * 1000 + lb * 10 + lc + sop)
    t = tuple(rng.integers(0, 4, n) for n in (la, lb, lc))
    got = pencil_emu.emulate([t], sop=bool(sop), vs=True, shifted=False, garbage_seed=5, ring_garbage_seed=6)
    assert got == [_score(orc, t, sop)]


@pytest.mark.parametrize("vs", [False, True])
def test_garbage_ring_other_forms(orc, vs):
    """The message form (which fills every row) and the writer-shifted V-space
    form over a garbage ring."""
    import pencil_emu
    rng = np.random.default_rng(8)
    t = tuple(rng.integers(0, 4, n) for n in (140, 17, 100))
    got = pencil_emu.emulate([t], vs=vs, shifted=vs, garbage_seed=5, ring_garbage_seed=6)
    assert got == [_score(orc, t, 0)]


@pytest.mark.parametrize("sop", [0, 1])
def test_garbage_ring_two_triples(orc, sop):
    """TWO mode: two triples of different lengths in the halves of one wave."""
    import pencil_emu
    rng = np.random.default_rng(9 + sop)
    t1 = tuple(rng.integers(0, 4, n) for n in (60, 12, 60))
    t2 = tuple(rng.integers(0, 4, n) for n in (41, 9, 33))
    got = pencil_emu.emulate([t1, t2], sop=bool(sop), vs=True, shifted=False, garbage_seed=5, ring_garbage_seed=6)
    assert got == [_score(orc, t1, sop), _score(orc, t2, sop)]


def test_garbage_ring_is_seen_when_a_row_is_missing(orc, monkeypatch):
    """The check has teeth: with the first four rows wave 0 fetches left
    unfilled (the emulator's FILL_FROM hook), the garbage reaches a real cell."""
    import pencil_emu
    rng = np.random.default_rng(10)
    t = tuple(rng.integers(0, 4, n) for n in (128, 8, 128))
    ref = [_score(orc, t, 0)]
    assert pencil_emu.emulate([t], vs=True, shifted=False, ring_garbage_seed=6) == ref
    monkeypatch.setattr(pencil_emu, "FILL_FROM", 4)
    assert pencil_emu.emulate([t], vs=True, shifted=False, ring_garbage_seed=6) != ref
