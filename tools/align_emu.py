"""CPU replay of the resident traceback kernel (csrc/align_kernel.hip): the
schedule tsa_align_batch runs for a triple whose (y,z) planes fit LDS.

TEST/DESIGN INFRASTRUCTURE (tests/test_align_batch.py checks it against the
oracle's traceback move for move). It models what the kernel's correctness
rests on, not its arithmetic speed:

  * two (y,z) buffers of 7-state cells, zero-initialised, with a zero row
    y = 0 and a zero column z = 0 for those faces;
  * the publication rule: at step q position (y,z) is at x = q-y-z and writes
    its states into buf[q&1] only while 1 <= x <= la, so a position that has
    not started reads as the x = 0 face and one past x = la leaves a stale
    entry no real cell reads;
  * the reads of buf[(q-1)&1] while 0 <= x <= la -- own, N1 = (y-1,z),
    W1 = (y,z-1), NW1 = (y-1,z-1) -- and the predecessor table
        Ix <- own  Iy <- N1  Iz <- W1  Ixy <- last step's N1
        Iyz <- last step's NW1  Ixz <- last step's W1  M <- NW1 of two steps back
  * the register history: the step that reads N1, W1, NW1 evaluates at once
    what the later cells take from them -- Ixy, Ixz, Iyz of cell x+1 (symbol
    a_{x+1}) and M of cell x+2 (a_{x+2}) -- and keeps those 5 (state, argmax)
    pairs instead of the 4 cells; M of x = 1 (the corner of the zero faces) is
    evaluated at x = 0;
  * the pointer word (3 bits per target state = lowest source state that won
    its literal MAX7, src/PE_1cyc.v:1-32,164-218) and the walk back from
    (la,lb,lc), lowest state index first at the final MAX7
    (src/TriAlign_1cyc.v:141-142).

All positions of a step read before any writes (the kernel's buffers alternate
and one barrier per step orders them); here the step's writes go to the other
buffer, so program order gives the same.
"""
from __future__ import annotations

import numpy as np

from literal_emu import penalties

DX = (1, 1, 0, 0, 1, 0, 1)   # predecessor offsets per state (MOVE_CONSUMES)
DY = (1, 0, 1, 0, 1, 1, 0)
DZ = (1, 0, 0, 1, 0, 1, 1)
ZERO = (0,) * 7


def _wrap(v, bits):
    if bits == 0:
        return v
    m = 1 << bits
    return ((v + (m >> 1)) % m) - (m >> 1)


class Cell:
    """The literal cell of one triple under one parameter set: the score
    constants, MAX7 and the step of one position, shared by the resident and the
    tiled replay (csrc/align_step.h is what the two kernels share)."""

    def __init__(self, a, b, c, match=1, mismatch=-1, go=2, ge=1, sop=False, bits=12):
        self.a, self.b, self.c = (np.asarray(s, np.int64) & 3 for s in (a, b, c))
        self.la, self.lb, self.lc = len(self.a), len(self.b), len(self.c)
        self.pen, self.sop = penalties(go, ge), sop
        self.w = w = lambda v: _wrap(int(v), bits)
        self.mt, self.mm = w(match), w(mismatch)
        self.s3 = w(3 * match), w(2 * (match + mismatch)), w(3 * mismatch)

    def max7(self, T, pred, add):
        best, arg = None, 0
        for s in range(7):
            v = self.w(pred[s] - int(self.pen[T][s]) + add)
            if best is None or v > best:
                best, arg = v, s
        return best, arg

    def adds(self, x, y, z):
        """(sab, sbc, sac, s3) of cell (x, y, z); x clamped into A as the kernel's lookup."""
        ax, by, cz = int(self.a[min(max(x, 1), self.la) - 1]), int(self.b[y - 1]), int(self.c[z - 1])
        sab = self.mt if ax == by else self.mm
        sbc = self.mt if by == cz else self.mm
        sac = self.mt if ax == cz else self.mm
        if self.sop:
            s3 = self.w(sab + sbc + sac)
        else:
            s3 = (self.s3[0] if by == cz else self.s3[1]) if ax == by else self.s3[2]
        return sab, sbc, sac, s3

    @staticmethod
    def history():
        return dict(XY=(0, 0), YZ=(0, 0), XZ=(0, 0), M3=(0, 0), M2=(0, 0))

    def step(self, h, x, own, n1, w1, nw1, y, z):
        """One step of the position at global (y, z), 0 <= x <= la, on its four
        reads: updates its history h and returns (cell, pointer word), None
        at x = 0, where there is no cell."""
        out = None
        if x == 0:
            h["M3"] = self.max7(0, ZERO, self.adds(1, y, z)[3])
        else:
            res = [h["M3"], self.max7(1, own, 0), self.max7(2, n1, 0), self.max7(3, w1, 0), h["XY"], h["YZ"], h["XZ"]]
            out = tuple(v for v, _ in res), sum(g << (3 * T) for T, (_, g) in enumerate(res))
            h["M3"] = h["M2"]
        sab, sbc, sac, _ = self.adds(x + 1, y, z)
        h["XY"], h["XZ"], h["YZ"] = self.max7(4, n1, sab), self.max7(6, w1, sac), self.max7(5, nw1, sbc)
        h["M2"] = self.max7(0, nw1, self.adds(x + 2, y, z)[3])
        return out


def emulate(a, b, c, match=1, mismatch=-1, go=2, ge=1, sop=False, bits=12, on_cell=None):
    """(score, final7, ptr) by the resident schedule; ptr maps a cell
    (x, y, z) to its pointer word. on_cell(x, y, z, states, p) is called for
    every cell as the schedule computes it, p the number of its position in the
    plane (tools/align_ends_emu.py folds the end keys there)."""
    K = Cell(a, b, c, match, mismatch, go, ge, sop, bits)
    la, lb, lc = K.la, K.lb, K.lc
    buf = [[[ZERO] * (lc + 1) for _ in range(lb + 1)] for _ in range(2)]
    hist = {(y, z): K.history() for y in range(1, lb + 1) for z in range(1, lc + 1)}
    ptr, fin = {}, None
    for q in range(2, la + lb + lc + 1):
        rd, wr = buf[(q - 1) & 1], buf[q & 1]
        for (y, z), h in hist.items():
            x = q - y - z
            if x < 0 or x > la:
                continue
            out = K.step(h, x, rd[y][z], rd[y - 1][z], rd[y][z - 1], rd[y - 1][z - 1], y, z)
            if out:
                wr[y][z], ptr[(x, y, z)] = out
                if on_cell:
                    on_cell(x, y, z, out[0], (y - 1) * lc + (z - 1))
                if (x, y, z) == (la, lb, lc):
                    fin = wr[y][z]
    return max(fin), fin, ptr


def walk(ptr, fin, la, lb, lc):
    """((x0, y0, z0), moves in forward order): tb_walk on the pointer words."""
    T = 0
    for s in range(1, 7):
        if fin[s] > fin[T]:
            T = s
    return walk_from(ptr, T, la, lb, lc)


def walk_from(ptr, T, x, y, z):
    """((x0, y0, z0), moves in forward order) from cell (x, y, z) in state T:
    walk_back of csrc/plane_kernel.hip, at most x + y + z moves."""
    bound, moves = x + y + z, []
    while True:
        moves.append(T)
        px, py, pz = x - DX[T], y - DY[T], z - DZ[T]
        if px == 0 or py == 0 or pz == 0 or len(moves) >= bound:
            x, y, z = px, py, pz
            break
        T = (ptr[(x, y, z)] >> (3 * T)) & 7
        x, y, z = px, py, pz
    return (x, y, z), np.asarray(moves[::-1], np.uint8)


def align(a, b, c, match=1, mismatch=-1, go=2, ge=1, sop=False, bits=12):
    """(score, start, moves), as oracle.align and tsa_align_batch return them."""
    score, fin, ptr = emulate(a, b, c, match, mismatch, go, ge, sop, bits)
    start, moves = walk(ptr, fin, len(a), len(b), len(c))
    return score, start, moves
