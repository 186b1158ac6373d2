"""CPU replay of the grid path with a free end, tsa_align_batch_grid_ends
(TSA_END_FACE, TSA_END_ANY; the END forms of csrc/align_grid_kernel.hip): the
schedule of tools/align_grid_emu.py with the key of tools/align_ends_emu.py.

TEST/DESIGN INFRASTRUCTURE (tests/test_align_grid_ends.py checks it against the
oracle on the prefixes the end cell names, move for move):

  * the forward pass: launch d = 0 .. nty+ntz-2 sweeps every tile with
    ty + tz = d, the last tile (nty-1,ntz-1) included -- it stores no face --
    against a snapshot of the kept faces, which start POISON; every candidate
    cell folds its key into the running best of its thread (position p of the
    tile belongs to thread p % nt), and after the sweep the workgroup's max
    goes into the tile's own slot ty*ntz + tz. The slots start POISON_KEY (what
    another call left there): a tile that were not swept would win every max;
  * the end record: the max over the slots, decoded into {x1, y1, z1, state,
    score}; a key that names no cell of the cube is an error (n_moves = 0 on
    the device), never a path;
  * the backward launches j = 0, 1, ..: launch 0 too reads the walker record,
    {x1, y1, z1, state}: the record's tile swept again from its two faces, only
    the cells with x <= the record's x, pointer words into a tile cube cleared
    before every sweep. The sweep gives neither a score nor final states: when
    the end lies in the last tile with x1 = la the swept range holds
    (la,lb,lc), and what the corner would write there is not the end's;
  * the segment walks and the early end of tools/align_grid_emu.py (`swept`
    lists the tiles swept backward, in order).
"""
from __future__ import annotations

import copy

import numpy as np

from align_emu import DX, DY, DZ, Cell
from align_ends_emu import END_ANY, END_CORNER, END_FACE, END_MODES, candidate, cell_key, decode, key_fits, \
    reduce_keys, threads_tiled
from align_grid_emu import _sweep
from align_grid_emu import emulate as _emulate_corner
from align_tiled_emu import POISON, tile_geom

POISON_KEY = (1 << 64) - 1     # a slot no tile of this call has written


def emulate(a, b, c, mode, match=1, mismatch=-1, go=2, ge=1, sop=False, bits=12, tile=(64, 48), nt=None):
    """(score, start, moves, end, swept): the whole schedule; swept = the tiles
    (ty, tz) the backward launches swept, in order."""
    K = Cell(a, b, c, match, mismatch, go, ge, sop, bits)
    la, lb, lc = K.la, K.lb, K.lc
    if mode == END_CORNER:
        s, st, mv, swept = _emulate_corner(a, b, c, match, mismatch, go, ge, sop, bits, tile)
        return s, st, mv, (la, lb, lc), swept
    assert mode in (END_FACE, END_ANY) and key_fits(la, lb, lc)
    geom = tile_geom(lb, lc, *tile)
    TY, TZ, nty, ntz = geom
    if nt is None:
        nt = threads_tiled(TY, TZ)
    yface = [[[POISON] * (lc + 1) for _ in range(la + 1)] for _ in range(nty - 1)]   # [ty][x][global z]
    zface = [[[POISON] * (lb + 1) for _ in range(la + 1)] for _ in range(ntz - 1)]   # [tz][x][global y]
    slots = [POISON_KEY] * (nty * ntz)
    for d in range(nty + ntz - 1):                               # the forward launches: one more than the corner's
        yold, zold = copy.deepcopy(yface), copy.deepcopy(zface)  # what the launches before left
        for ty in range(max(0, d - (ntz - 1)), min(nty - 1, d) + 1):
            tz = d - ty
            best = {}                                            # the running best of each thread of this workgroup

            def on_cell(x, y, z, states, p):
                if candidate(mode, x, y, z, la, lb, lc):
                    best[p % nt] = max(best.get(p % nt, 0), cell_key(states, x, y, z, lb, lc))

            _sweep(K, geom, ty, tz, la, yold[ty - 1] if ty else None, zold[tz - 1] if tz else None,
                   yface[ty] if ty + 1 < nty else None, zface[tz] if tz + 1 < ntz else None, None, on_cell)
            slots[ty * ntz + tz] = reduce_keys(best, nt)         # every tile writes its slot, candidates or not
    x, y, z, T, score = decode(max(slots), lb, lc)               # the end record
    assert 1 <= x <= la and 1 <= y <= lb and 1 <= z <= lc and 0 <= T < 7, "a slot was not written"
    end = (x, y, z)
    rec = dict(x=x, y=y, z=z, T=T, done=False)                   # the walker record
    moves, swept, ptr = [], [], {}
    for j in range(nty + ntz - 1):
        if rec["done"]:
            break                                                # the early end: no other tile is swept
        x, y, z, T = rec["x"], rec["y"], rec["z"], rec["T"]
        ty, tz = (y - 1) // TY, (z - 1) // TZ
        ptr.clear()                                              # launch j overwrites the tile cube
        _sweep(K, geom, ty, tz, x, yface[ty - 1] if ty else None, zface[tz - 1] if tz else None, None, None, ptr)
        swept.append((ty, tz))
        y0, z0 = ty * TY, tz * TZ
        while True:
            moves.append(T)
            px, py, pz = x - DX[T], y - DY[T], z - DZ[T]
            if px == 0 or py == 0 or pz == 0 or len(moves) >= la + lb + lc:
                x, y, z = px, py, pz
                rec["done"] = True
                break
            T = (ptr[(x, y - y0, z - z0)] >> (3 * T)) & 7
            x, y, z = px, py, pz
            if y <= y0 or z <= z0:
                break
        rec.update(x=x, y=y, z=z, T=T)
    assert rec["done"]
    return score, (rec["x"], rec["y"], rec["z"]), np.asarray(moves[::-1], np.uint8), end, swept


def align(a, b, c, mode, match=1, mismatch=-1, go=2, ge=1, sop=False, bits=12, tile=(64, 48), nt=None):
    """(score, start, moves, end), as tsa_align_batch_grid_ends returns them;
    mode: END_MODES' values; tile = (TYmax, TZmax), the caps of the tile edges."""
    return emulate(a, b, c, mode, match, mismatch, go, ge, sop, bits, tile, nt)[:4]
