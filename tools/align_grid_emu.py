"""CPU replay of the grid path of tsa_align_batch (csrc/align_grid_kernel.hip
and tb_walk_grid of csrc/plane_kernel.hip): the schedule of align_mode=grid,
tsa_align_batch_grid's, for a triple whose (y,z) plane does not fit one
workgroup.

TEST/DESIGN INFRASTRUCTURE (tests/test_align_grid.py checks it against the
oracle's traceback move for move). The tiles are the tiled schedule's
(tools/align_tiled_emu.py), but every tile is swept on its own, from faces that
are all kept:

  * the kept faces: y face ty = the last row of tile row ty, [nty-1][x][global
    z], and z face tz = the last column of tile column tz, [ntz-1][x][global
    y]; nothing alternates by parity. They are POISON before the forward pass;
  * the forward pass: launch d = 0 .. nty+ntz-3 sweeps the tiles with
    ty + tz = d without pointer words, all of them from the faces as launch
    d-1 left them (the tiles of one launch may run in any order: here they
    run against a snapshot, so a read of a face of the same launch shows);
    tile (nty-1,ntz-1) is not swept, a tile stores its y face unless
    ty = nty-1 and its z face unless tz = ntz-1;
  * the backward launches j = 0, 1, ..: the tile that holds the walker
    record's cell ((lb,lc) at j = 0) swept again from its two faces, only the
    cells with x <= the record's x, its pointer words into a tile cube keyed
    (x, y - y0, z - z0); the cube is cleared before every sweep, so a word of
    another tile, or of a cell beyond the trim, can never be followed;
  * the segment walk after each launch: from the walker record {x, y, z, T,
    done} while y > y0 and z > z0; a predecessor on a zero face ends the path,
    one in another tile -- beyond the y seam, the z seam or the corner --
    saves the record;
  * the early end: once the record is done, no further tile is swept (`swept`
    lists the tiles that were, in order).

A read of a cell that was never stored shows as a wrong move or score.
"""
from __future__ import annotations

import copy

import numpy as np

from align_emu import DX, DY, DZ, ZERO, Cell
from align_tiled_emu import POISON, tile_geom


def _sweep(K, geom, ty, tz, xm, yrd, zrd, ywr, zwr, ptr, on_cell=None):
    """Tile (ty, tz) up to x = xm: reads the y face yrd and the z face zrd
    (None: zero), stores its last row into ywr and its last column into zwr
    (None: not kept), pointer words into ptr (None: the forward form) keyed
    (x, local y, local z). Returns the cell (xm, lb, lc) if the tile holds it.
    on_cell(x, y, z, states, p) is called for every cell as the sweep computes
    it, (y, z) global and p the number of its position in the tile
    (tools/align_grid_ends_emu.py folds the end keys there)."""
    la, lb, lc = K.la, K.lb, K.lc
    TY, TZ, _, _ = geom
    y0, z0 = ty * TY, tz * TZ
    tyl, tzl = min(TY, lb - y0), min(TZ, lc - z0)
    buf = [[[ZERO] * (TZ + 1) for _ in range(TY + 1)] for _ in range(2)]
    hist = {(y, z): K.history() for y in range(1, tyl + 1) for z in range(1, tzl + 1)}
    fin = None
    qmax = xm + tyl + tzl + (1 if ywr is not None or zwr is not None else 0)
    for q in range(1, qmax + 1):
        rd, wr = buf[(q - 1) & 1], buf[q & 1]
        new = {}
        for (y, z), h in hist.items():
            x = q - y - z
            if x < 0 or x > xm:
                continue
            out = K.step(h, x, rd[y][z], rd[y - 1][z], rd[y][z - 1], rd[y - 1][z - 1], y0 + y, z0 + z)
            if out:
                new[(y, z)] = out[0]
                if on_cell:
                    on_cell(x, y0 + y, z0 + z, out[0], (y - 1) * tzl + (z - 1))
                if ptr is not None:
                    ptr[(x, y, z)] = out[1]
                    if (x, y0 + y, z0 + z) == (xm, lb, lc):
                        fin = out[0]
        for f in range(tzl + tyl + 1):                           # the face threads
            row = f <= tzl
            y, z = (0, f) if row else (f - tzl, 0)
            x = q - y - z
            src = (yrd if (f or zrd is not None) else None) if row else zrd
            if src is not None and 1 <= x <= xm:
                new[(y, z)] = src[x][z0 + z] if row else src[x][y0 + y]
            sy, sz = (tyl, z) if row else (y, tzl)
            sx = q - 1 - sy - sz
            dst = ywr if row else zwr
            if f and dst is not None and 1 <= sx <= xm:
                if row:
                    dst[sx][z0 + sz] = rd[sy][sz]
                else:
                    dst[sx][y0 + sy] = rd[sy][sz]
        for (y, z), cell in new.items():
            wr[y][z] = cell
    return fin


def emulate(a, b, c, match=1, mismatch=-1, go=2, ge=1, sop=False, bits=12, tile=(64, 48)):
    """(score, start, moves, swept): the whole schedule; swept = the tiles
    (ty, tz) the backward launches swept, in order."""
    K = Cell(a, b, c, match, mismatch, go, ge, sop, bits)
    la, lb, lc = K.la, K.lb, K.lc
    geom = tile_geom(lb, lc, *tile)
    TY, TZ, nty, ntz = geom
    yface = [[[POISON] * (lc + 1) for _ in range(la + 1)] for _ in range(nty - 1)]   # [ty][x][global z]
    zface = [[[POISON] * (lb + 1) for _ in range(la + 1)] for _ in range(ntz - 1)]   # [tz][x][global y]
    for d in range(nty + ntz - 2):                               # the forward launches
        yold, zold = copy.deepcopy(yface), copy.deepcopy(zface)  # what the launches before left
        for ty in range(max(0, d - (ntz - 1)), min(nty - 1, d) + 1):
            tz = d - ty
            if (ty, tz) == (nty - 1, ntz - 1):
                continue
            _sweep(K, geom, ty, tz, la, yold[ty - 1] if ty else None, zold[tz - 1] if tz else None,
                   yface[ty] if ty + 1 < nty else None, zface[tz] if tz + 1 < ntz else None, None)
    rec = None                                                   # the walker record
    score, moves, swept = None, [], []
    ptr = {}
    for j in range(nty + ntz - 1):
        if rec is not None and rec["done"]:
            break                                                # the early end: no other tile is swept
        x, y, z = (la, lb, lc) if j == 0 else (rec["x"], rec["y"], rec["z"])
        ty, tz = (y - 1) // TY, (z - 1) // TZ
        ptr.clear()                                              # launch j overwrites the tile cube
        fin = _sweep(K, geom, ty, tz, x, yface[ty - 1] if ty else None, zface[tz - 1] if tz else None, None, None, ptr)
        swept.append((ty, tz))
        if j == 0:
            assert (ty, tz) == (nty - 1, ntz - 1)
            score = max(fin)
            T = 0
            for k in range(1, 7):
                if fin[k] > fin[T]:
                    T = k
            rec = dict(x=la, y=lb, z=lc, T=T, done=False)
        T = rec["T"]
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
    return score, (rec["x"], rec["y"], rec["z"]), np.asarray(moves[::-1], np.uint8), swept


def align(a, b, c, match=1, mismatch=-1, go=2, ge=1, sop=False, bits=12, tile=(64, 48)):
    """(score, start, moves), as oracle.align and tsa_align_batch_grid return
    them; tile = (TYmax, TZmax), the caps of the tile edges (align_tile)."""
    return emulate(a, b, c, match, mismatch, go, ge, sop, bits, tile)[:3]
