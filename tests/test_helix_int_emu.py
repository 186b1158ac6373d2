"""The helix schedule on integer bit patterns, replayed on the CPU
(tools/pencil_emu.py int_bits=True, the kernel's cell_messages_vi): every
register the 32-bit word of two 16-bit patterns bias + 8 V, the cell's constant
adds done on the word, LDS and ring started as garbage. Against the C oracle,
with both event counters at zero: no half of a started position leaves
[0x0400, 0x7BFF], and no add or subtract carries out of a low half beside a
started high half (position k + 128 of the same register).

Shapes (LA, LB, LC):
  * (5, 9, 129): the most x and z padding (P = 256, one real cell in the high
    halves) and a partial second lap;
  * (256, 8, 256), (256, 9, 256): one lap exactly, and one row more;
  * (253..257, 17, 256): the lap wrap at every phase of the four-step group;
each with a random triple; (5, 9, 129), (256, 9, 256) and (257, 17, 256) also
with the all-match triple (the top of the range) and the all-distinct one (the
bottom).
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import pencil_emu  # noqa: E402

SHAPES = [(5, 9, 129), (256, 8, 256), (256, 9, 256)] + [(la, 17, 256) for la in (253, 254, 255, 256, 257)]
EXTREMES = [(5, 9, 129), (256, 9, 256), (257, 17, 256)]


def _triples(dims, seed):
    rng = np.random.default_rng(seed)
    return {"random": tuple(rng.integers(0, 4, d).astype(np.uint8) for d in dims),
            "all-match": tuple(np.full(d, 3, np.uint8) for d in dims),
            "all-distinct": tuple(np.full(d, v, np.uint8) for d, v in zip(dims, (0, 1, 2)))}


@pytest.mark.parametrize("dims", SHAPES, ids=lambda d: "x".join(map(str, d)))
def test_int_bits_schedule(orc, dims):
    p = orc.default_params(score_bits=0)
    for kind, (a, b, c) in _triples(dims, 7 * dims[0] + dims[1]).items():
        if kind != "random" and dims not in EXTREMES:
            continue
        ev = {}
        got = pencil_emu.emulate([(a, b, c)], vs=True, read_prev=True, int_bits=True, garbage_seed=11,
                                 ring_garbage_seed=12, events=ev)
        print(dims, kind, got, ev)
        assert got == [orc.score(a, b, c, p)], (dims, kind)
        assert ev == {"window": 0, "carry": 0}, (dims, kind, ev)


def test_sop_and_lam2(orc):
    """The sum-of-pairs s3 (K is added as a packed word) and lam = 2."""
    dims = (5, 9, 129)
    for kw, okw in ((dict(sop=True), dict(s3_mode=1)),
                    (dict(match=0, mismatch=-2, go=3, ge=2), dict(match=0, mismatch=-2, gap_open=3, gap_extend=2))):
        p = orc.default_params(score_bits=0, **okw)
        for kind, (a, b, c) in _triples(dims, 3).items():
            ev = {}
            got = pencil_emu.emulate([(a, b, c)], vs=True, read_prev=True, int_bits=True, garbage_seed=5,
                                     ring_garbage_seed=6, events=ev, **kw)
            assert got == [orc.score(a, b, c, p)], (kw, kind)
            assert ev == {"window": 0, "carry": 0}, (kw, kind, ev)


def test_counters_fire_on_a_low_bias():
    """A bias placed far too low (-400: every V below 50 is negative as a
    pattern): halves leave the window and low halves borrow from started high
    halves; both counters must say so."""
    dims = (5, 9, 129)
    a, b, c = _triples(dims, 1)["all-distinct"]
    ev = {}
    pencil_emu.emulate([(a, b, c)], vs=True, read_prev=True, int_bits=True, garbage_seed=1, ring_garbage_seed=2,
                       bias=-400, events=ev)
    assert ev["window"] > 0 and ev["carry"] > 0, ev


def test_bias_rule():
    """The 512 x 256^3 batch's shape is admitted with the RTL constants, and the
    interval the rule leaves fits the window."""
    bias = pencil_emu.vi_bias(256, 256, 256)
    assert pencil_emu.VI_LO < bias < pencil_emu.VI_HI
    assert pencil_emu.vi_bias(5, 9, 129, match=-5, mismatch=-6, go=7, ge=6) == 0  # f16v admits it, the window does not
