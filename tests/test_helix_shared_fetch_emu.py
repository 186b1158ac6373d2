"""The helix's shared ring fetch on the CPU (csrc/pencil_kernel.hip, the RP
forms): tools/pencil_emu.py `shared_fetch` replays which middle wave
issues each of wave 0's ring rows, at which step of the four-step group, into
which slot of wave 0's LDS copy, and when the issuer's counted wait and the
step barrier make the row readable. A slot in flight holds garbage, the ring
and the LDS record slots start as garbage, so a row read early, fetched over
an unread one, or fetched before the last wave wrote it spoils the score; the
emulator also counts the two timing violations themselves.

Shapes (P is the lap period, t_sw wave 0's first fetching step):
  * (256, 9, 256): the second lap is one row, the first fetched rows follow
    t_sw directly;
  * (256, 24, 256): three laps, the ring wraps;
  * (257, 17, 200): P = 260, t_sw = 4 (mod 8): the slots' two groups swap;
  * (253, 17, 256): padding columns, the lap wrap inside a group.
Both cells (the integer patterns and the float V-space cell), and the schedule
shifted by one barrier interval either way, which must trip the counters."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

SHAPES = [(256, 9, 256), (256, 24, 256), (257, 17, 200), (253, 17, 256)]


def _triple(la, lb, lc):
    rng = np.random.default_rng(la * 1000 + lb * 10 + lc)
    return tuple(rng.integers(0, 4, n) for n in (la, lb, lc))


@pytest.fixture(scope="module")
def refs(orc):
    """The oracle's score of each shape's triple, computed once."""
    return {s: orc.score(*_triple(*s), orc.default_params(score_bits=0)) for s in SHAPES}


def _emulate(shape, int_bits, shift=0):
    import pencil_emu
    ev = {}
    got = pencil_emu.emulate([_triple(*shape)], vs=True, read_prev=True, int_bits=int_bits, garbage_seed=5,
                             ring_garbage_seed=6, shared_fetch=True, fetch_shift=shift, events=ev)
    return got, ev


@pytest.mark.parametrize("int_bits", [True, False], ids=["int", "float"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_shared_fetch_schedule(refs, shape, int_bits):
    got, ev = _emulate(shape, int_bits)
    assert (ev["fetch_in_flight"], ev["fetch_unread"]) == (0, 0), ev
    assert got == [refs[shape]]
    if int_bits:
        assert (ev["window"], ev["carry"]) == (0, 0), ev


def test_shifted_schedules_are_caught(refs):
    """One barrier interval early: the fetch lands on a slot wave 0 reads in the
    same interval. One late: the row is still in flight when wave 0 reads it."""
    shape = (256, 9, 256)
    got, ev = _emulate(shape, True, shift=1)
    assert ev["fetch_unread"] > 0, ev
    assert got != [refs[shape]]
    got, ev = _emulate(shape, True, shift=-1)
    assert ev["fetch_in_flight"] > 0 and ev["fetch_unread"] == 0, ev
    assert got != [refs[shape]]
