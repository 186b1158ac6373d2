"""The helix's row-above z-shift by read address (the RP forms of
csrc/pencil_kernel.hip) on the CPU: tools/pencil_emu.py with read_prev=True
takes {Iyz, best} of the row above from the record of position k-1 -- register
i-1 of the lane, register M-1 of lane-1, lane 63 for lane 0 -- and fixes only
lane 0's register 0 ({z = 0 face, lane 63's low half}); no write changes. The
ring and the LDS slots start as garbage, so a shifted read that picked up a
row or a slot nobody wrote would spoil the score.

This checks the data rule only -- which record's halves a lane and register
takes, the lane-0 wrap, the garbage start: the emulator has no LDS addresses,
so the kernel's address arithmetic (the lane - 1 base, the record offsets, wave
0's slot base) is guarded by the GPU cases of tests/test_helix_prev_reads.py.

The shapes are tests/test_helix_prev_reads.py's, scaled to the emulator's
speed: a real cell in the half that crosses from lane 63 to lane 0 (LC = 129
is the smallest), the lap wrap at every phase of the four-step group with a
third lap (so wave 0 reads shifted from the prefetched ring rows), and LB = 1,
8 (no second lap) and 9 (the first row that comes through the ring)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

SHAPES = [
    (20, 9, 129), (20, 9, 130), (20, 9, 255), (20, 9, 256),  # positions 128.. : the lane 63 -> lane 0 half
    (253, 17, 256), (254, 17, 256), (255, 17, 256), (256, 17, 256), (257, 17, 256),  # the wrap at every phase
    (40, 1, 130), (40, 8, 130), (40, 9, 130),  # one row, one full lap, the first ring row
    (90, 17, 100),  # M = 1: register 0 is the only register
]


def _score(orc, t, sop, **kw):
    return orc.score(*t, orc.default_params(s3_mode=sop, score_bits=0, **kw))


@pytest.mark.parametrize("la,lb,lc", SHAPES)
def test_prev_reads_match_oracle(orc, la, lb, lc):
    import pencil_emu
    sop = (la + lb + lc) & 1  # both s3 modes over the list
    rng = np.random.default_rng(la * 1000 + lb * 10 + lc)
    t = tuple(rng.integers(0, 4, n) for n in (la, lb, lc))
    got = pencil_emu.emulate([t], sop=bool(sop), vs=True, shifted=False, read_prev=True, garbage_seed=5,
                             ring_garbage_seed=6)
    assert got == [_score(orc, t, sop)]


def test_prev_reads_lam2(orc):
    """lam = 2: the faces step by 2 (the kernel reads its table at stride 2)."""
    import pencil_emu
    rng = np.random.default_rng(12)
    t = tuple(rng.integers(0, 4, n) for n in (50, 11, 140))
    got = pencil_emu.emulate([t], vs=True, shifted=False, read_prev=True, garbage_seed=5, ring_garbage_seed=6,
                             match=2, mismatch=-2, go=3, ge=2)
    assert got == [_score(orc, t, 0, match=2, mismatch=-2, gap_open=3, gap_extend=2)]


def test_prev_reads_two_triples(orc):
    """TWO mode: lane 0 takes the face in both halves."""
    import pencil_emu
    rng = np.random.default_rng(13)
    t1 = tuple(rng.integers(0, 4, n) for n in (60, 12, 60))
    t2 = tuple(rng.integers(0, 4, n) for n in (41, 9, 33))
    got = pencil_emu.emulate([t1, t2], vs=True, shifted=False, read_prev=True, garbage_seed=5, ring_garbage_seed=6)
    assert got == [_score(orc, t1, 0), _score(orc, t2, 0)]
