"""CPU replay of the strip path of tsa_align_batch (csrc/align_strip_kernel.hip
and tb_walk_strip of csrc/plane_kernel.hip): the schedule of align_mode=strip,
tsa_align_batch_lowmem's, for a triple whose (y,z) plane does not fit one
workgroup.

TEST/DESIGN INFRASTRUCTURE (tests/test_align_strip.py checks it against the
oracle's traceback move for move). A strip is one tile row of the tiled
schedule (tools/align_tiled_emu.py): TY rows of y, all of z, all of x, swept
tile by tile along z through the two z faces. On top of that it has

  * the forward pass: strips 0 .. nty-2 without pointer words, the last local
    row of strip s stored into a y face of its own, [nty-1][x][global z];
  * the strip launches j = 0, 1, ..: strip s = nty-1-j swept again from y face
    s-1 (the zero face when s = 0), its pointer words into a strip cube that
    holds this strip alone, keyed (x, y - s*TY, z); the cube is poisoned before
    every sweep, so a word of another strip can never be followed;
  * the segment walk after each launch: from the walker record {x, y, z, T, n,
    done} (from (la,lb,lc) and the final states at j = 0) while y > s*TY; a
    predecessor on a zero face ends the path, one in the strip below saves
    the record;
  * the early end: once the record is done, no further strip is swept
    (`swept` lists the strips that were).

The y faces start as POISON and so does whatever the tiled replay poisons, so
a read of a cell that was never stored shows as a wrong move or score.
"""
from __future__ import annotations

import numpy as np

from align_emu import DX, DY, DZ, ZERO, Cell
from align_tiled_emu import POISON, tile_geom


def _sweep(K, geom, s, yrd, ywr, ptr):
    """Strip s of the tiled schedule: reads the y face yrd (None: zero), stores
    its last row into ywr (None: not kept), pointer words into ptr (None: the
    forward form) keyed (x, local y, z). Returns the cell (la,lb,lc) if the
    strip holds it."""
    la, lb, lc = K.la, K.lb, K.lc
    TY, TZ, nty, ntz = geom
    y0 = s * TY
    tyl = min(TY, lb - y0)
    buf = [[[POISON] * (TZ + 1) for _ in range(TY + 1)] for _ in range(2)]
    zface = [[[POISON] * (TY + 1) for _ in range(la + 1)] for _ in range(2)]   # [parity][x][local y]
    fin = None
    for tz in range(ntz):
        z0 = tz * TZ
        tzl = min(TZ, lc - z0)
        for p in range(2):
            for y in range(TY + 1):
                buf[p][y] = [ZERO] * (TZ + 1)
        hist = {(y, z): K.history() for y in range(1, tyl + 1) for z in range(1, tzl + 1)}
        zrd = zface[(tz - 1) & 1] if tz else None
        zwr = zface[tz & 1] if tz + 1 < ntz else None
        if zwr is not None:
            for x in range(la + 1):
                zwr[x] = [POISON] * (TY + 1)
        qmax = la + tyl + tzl + (1 if ywr is not None or zwr is not None else 0)
        for q in range(1, qmax + 1):
            rd, wr = buf[(q - 1) & 1], buf[q & 1]
            new = {}
            for (y, z), h in hist.items():
                x = q - y - z
                if x < 0 or x > la:
                    continue
                out = K.step(h, x, rd[y][z], rd[y - 1][z], rd[y][z - 1], rd[y - 1][z - 1], y0 + y, z0 + z)
                if out:
                    new[(y, z)] = out[0]
                    if ptr is not None:
                        ptr[(x, y, z0 + z)] = out[1]
                        if (x, y0 + y, z0 + z) == (la, lb, lc):
                            fin = out[0]
            for f in range(tzl + tyl + 1):                       # the face threads
                row = f <= tzl
                y, z = (0, f) if row else (f - tzl, 0)
                x = q - y - z
                src = (yrd if (f or zrd is not None) else None) if row else zrd
                if src is not None and 1 <= x <= la:
                    new[(y, z)] = src[x][z0 + z] if row else src[x][y]
                sy, sz = (tyl, z) if row else (y, tzl)
                sx = q - 1 - sy - sz
                dst = ywr if row else zwr
                if f and dst is not None and 1 <= sx <= la:
                    if row:
                        dst[sx][z0 + sz] = rd[sy][sz]
                    else:
                        dst[sx][sy] = rd[sy][sz]
            for (y, z), cell in new.items():
                wr[y][z] = cell
    return fin


def emulate(a, b, c, match=1, mismatch=-1, go=2, ge=1, sop=False, bits=12, tile=(64, 48)):
    """(score, start, moves, swept): the whole schedule; swept = the strips the
    strip launches swept, last first."""
    K = Cell(a, b, c, match, mismatch, go, ge, sop, bits)
    la, lb, lc = K.la, K.lb, K.lc
    geom = tile_geom(lb, lc, *tile)
    TY, nty = geom[0], geom[2]
    kept = [[[POISON] * (lc + 1) for _ in range(la + 1)] for _ in range(nty - 1)]   # [strip][x][global z]
    for s in range(nty - 1):                                     # the forward launch
        _sweep(K, geom, s, kept[s - 1] if s else None, kept[s], None)
    rec = None                                                   # the walker record
    score, moves, swept = None, [], []
    ptr = {}
    for j in range(nty):
        s = nty - 1 - j
        if rec is not None and rec["done"]:
            break                                                # the early end: the strips above are not swept
        ptr.clear()                                              # launch j overwrites the strip cube
        fin = _sweep(K, geom, s, kept[s - 1] if s else None, None, ptr)
        swept.append(s)
        if j == 0:
            score = max(fin)
            T = 0
            for k in range(1, 7):
                if fin[k] > fin[T]:
                    T = k
            rec = dict(x=la, y=lb, z=lc, T=T, done=False)
        x, y, z, T = rec["x"], rec["y"], rec["z"], rec["T"]
        ylo = s * TY
        assert ylo < y <= ylo + TY
        while True:
            moves.append(T)
            px, py, pz = x - DX[T], y - DY[T], z - DZ[T]
            if px == 0 or py == 0 or pz == 0 or len(moves) >= la + lb + lc:
                x, y, z = px, py, pz
                rec["done"] = True
                break
            T = (ptr[(x, y - ylo, z)] >> (3 * T)) & 7
            x, y, z = px, py, pz
            if y <= ylo:
                break
        rec.update(x=x, y=y, z=z, T=T)
    assert rec["done"]
    return score, (rec["x"], rec["y"], rec["z"]), np.asarray(moves[::-1], np.uint8), swept


def align(a, b, c, match=1, mismatch=-1, go=2, ge=1, sop=False, bits=12, tile=(64, 48)):
    """(score, start, moves), as oracle.align and tsa_align_batch_lowmem return
    them; tile = (TYmax, TZmax), the caps of the tile edges (align_tile)."""
    return emulate(a, b, c, match, mismatch, go, ge, sop, bits, tile)[:3]
