"""CPU replay of the end search of tsa_align_batch_ends (TSA_END_FACE,
TSA_END_ANY) on top of the resident and the tiled replay (tools/align_emu.py,
tools/align_tiled_emu.py), which hand it every cell in schedule order.

TEST/DESIGN INFRASTRUCTURE (tests/test_align_ends.py checks it against the
oracle on the prefixes the end cell names, move for move). It models what
csrc/align_step.h adds to the two kernels:

  * the key of a cell, one totally ordered 64-bit integer
        [63:48] MAX7 + 32768
        [47:3]  ~pos, pos = ((x-1)*lb + (y-1))*lc + (z-1), 45 bits
        [2:0]   7 - the lowest state that reaches the MAX7
    formed as the kernel forms it: the max over the 7 states of
    8 * state value + (7 - index), split again into MAX7 and state;
  * the candidates: every real cell under "any"; x == la or y == lb or
    z == lc under "face";
  * the running best of a thread: position number p of the plane (of a tile)
    belongs to thread p % nt, and a thread folds its cells in the order the
    schedule reaches them -- in the tiled kernel across all tiles;
  * the reduction: a max over the lanes of each wave of 64, then over the
    waves, and the decoding of the winner into the end record
    {x1, y1, z1, state, score};
  * the walk from the end record through the pointer words (walk_from).

A plain max is the whole rule, so neither the thread count nor the order of
the cells may change the result: `nt` and `shuffle` are there to show it.
"""
from __future__ import annotations

import random

import align_emu
import align_tiled_emu

END_CORNER, END_FACE, END_ANY = 0, 1, 2
END_MODES = {"corner": END_CORNER, "face": END_FACE, "any": END_ANY}
POS_BITS = 45
POS_MASK = (1 << POS_BITS) - 1


def key_fits(la, lb, lc):
    """align_end_key_fits of csrc/align_kernel.h."""
    return la * lb * lc <= 1 << POS_BITS


def cell_key(states, x, y, z, lb, lc):
    m = max(8 * int(v) + (7 - s) for s, v in enumerate(states))
    pos = ((x - 1) * lb + (y - 1)) * lc + (z - 1)
    assert 0 <= pos <= POS_MASK and 0 <= (m >> 3) + 32768 < 1 << 16
    return (((m >> 3) + 32768) << 48) | ((~pos & POS_MASK) << 3) | (m & 7)


def decode(key, lb, lc):
    """The end record (x1, y1, z1, state, score) of a key."""
    pos = ~(key >> 3) & POS_MASK
    row = pos // lc
    return row // lb + 1, row % lb + 1, pos % lc + 1, 7 - (key & 7), (key >> 48) - 32768


def candidate(mode, x, y, z, la, lb, lc):
    return mode == END_ANY or x == la or y == lb or z == lc


def threads_resident(lb, lc):
    """The workgroup align_launch_resident gives a plane of lb * lc positions."""
    pos = lb * lc
    k = 1 if pos <= 1024 else 2 if pos <= 2048 else 4
    return (-(-pos // k) + 63) // 64 * 64


def threads_tiled(ty, tz):
    pos = ty * tz
    k = -(-pos // 1024)
    return (-(-pos // k) + 63) // 64 * 64


def reduce_keys(best, nt):
    """The workgroup's key: a max over each wave, then over the waves."""
    waves = [max(best.get(t, 0) for t in range(w, w + 64)) for w in range(0, nt, 64)]
    return max(waves)


def end_record(a, b, c, mode, match=1, mismatch=-1, go=2, ge=1, sop=False, bits=12, tile=None, nt=None,
               shuffle=None):
    """((x1, y1, z1, state, score), ptr) by the resident schedule, or by the
    tiled one under tile = (TYmax, TZmax). shuffle: a seed; the cells are then
    folded in a shuffled order instead of the schedule's."""
    la, lb, lc = len(a), len(b), len(c)
    assert mode in (END_FACE, END_ANY) and key_fits(la, lb, lc)
    if nt is None:
        nt = threads_resident(lb, lc) if tile is None else threads_tiled(*align_tiled_emu.tile_geom(lb, lc, *tile)[:2])
    cells = []

    def on_cell(x, y, z, states, p):
        if candidate(mode, x, y, z, la, lb, lc):
            cells.append((p % nt, cell_key(states, x, y, z, lb, lc)))

    if tile is None:
        _, _, ptr = align_emu.emulate(a, b, c, match, mismatch, go, ge, sop, bits, on_cell=on_cell)
    else:
        _, _, ptr = align_tiled_emu.emulate(a, b, c, match, mismatch, go, ge, sop, bits, tile, on_cell=on_cell)
    if shuffle is not None:
        random.Random(shuffle).shuffle(cells)
    best = {}
    for t, k in cells:                       # the running best of thread t
        best[t] = max(best.get(t, 0), k)
    return decode(reduce_keys(best, nt), lb, lc), ptr


def align(a, b, c, mode, match=1, mismatch=-1, go=2, ge=1, sop=False, bits=12, tile=None, nt=None, shuffle=None):
    """(score, start, moves, end) as tsa_align_batch_ends returns them."""
    la, lb, lc = len(a), len(b), len(c)
    if mode == END_CORNER:
        if tile is None:
            s, st, mv = align_emu.align(a, b, c, match, mismatch, go, ge, sop, bits)
        else:
            s, st, mv = align_tiled_emu.align(a, b, c, match, mismatch, go, ge, sop, bits, tile)
        return s, st, mv, (la, lb, lc)
    (x1, y1, z1, state, score), ptr = end_record(a, b, c, mode, match, mismatch, go, ge, sop, bits, tile, nt, shuffle)
    start, moves = align_emu.walk_from(ptr, state, x1, y1, z1)
    return score, start, moves, (x1, y1, z1)
