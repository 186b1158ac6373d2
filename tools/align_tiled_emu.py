"""CPU replay of the tiled resident traceback kernel
(csrc/align_tiled_kernel.hip): the schedule tsa_align_batch runs under
align_mode=tiled for a triple whose (y,z) plane does not fit one workgroup.

TEST/DESIGN INFRASTRUCTURE (tests/test_align_tiled.py checks it against the
oracle's traceback move for move). On top of what tools/align_emu.py models
for one tile -- two zeroed buffers, publication only while 1 <= x <= la, the
reads own / N1 / W1 / NW1 of buf[(q-1)&1], the 5-state register history, the
pointer word and the walk -- it has what chains the tiles:

  * the tile grid: nty = ceil(lb/TYmax) tiles of TY = ceil(lb/nty) rows,
    likewise along z, swept ty outer and tz inner by one workgroup;
  * both buffers zeroed and the history reset at the start of every tile;
  * face positions: in a tile that is not in the first tile row (column),
    local (0,z) at x = q-z ((y,0) at x = q-y; the corner (0,0) at x = q, when
    the tile is in neither) publishes into buf[q&1], while 1 <= x <= la, the
    cell the neighbouring tile stored for that (x, global y, global z); steps
    start at q = 1, where the corner publishes x = 1;
  * face stores: the threads of the last local row copy what a position
    published one step ago (buf[(q-1)&1], x = q-1-y-z) into the y face
    [x][global z], those of the last local column into the z face
    [x][local y]; a tile with a face to write runs one step more for it;
  * the y face double-buffered by the parity of ty, the z face by that of tz;
  * only the tile that holds (lb,lc) gives the final states.

What the kernel never writes must never be read: the face arrays start as
POISON, the part of a face a tile is about to store is poisoned again first,
and the buffers are left poisoned at the end of every tile (the next tile's
zeroing has to clear them). A read of a cell that was never stored then shows
as a wrong move or score.
"""
from __future__ import annotations

from align_emu import ZERO, Cell, walk

POISON = tuple(12345 - 1111 * s for s in range(7))


def tile_geom(lb, lc, tymax, tzmax):
    """(TY, TZ, nty, ntz): align_tile_geom of csrc/align_kernel.h."""
    nty, ntz = -(-lb // tymax), -(-lc // tzmax)
    return -(-lb // nty), -(-lc // ntz), nty, ntz


def emulate(a, b, c, match=1, mismatch=-1, go=2, ge=1, sop=False, bits=12, tile=(64, 48), on_cell=None):
    """(score, final7, ptr) by the tiled schedule; ptr maps a cell (x, y, z)
    in global coordinates to its pointer word. on_cell(x, y, z, states, p) is
    called for every cell as the schedule computes it, p the number of its
    position in its tile (tools/align_ends_emu.py folds the end keys there)."""
    K = Cell(a, b, c, match, mismatch, go, ge, sop, bits)
    la, lb, lc = K.la, K.lb, K.lc
    TY, TZ, nty, ntz = tile_geom(lb, lc, *tile)
    buf = [[[POISON] * (TZ + 1) for _ in range(TY + 1)] for _ in range(2)]
    yface = [[[POISON] * (lc + 1) for _ in range(la + 1)] for _ in range(2)]   # [parity][x][global z]
    zface = [[[POISON] * (TY + 1) for _ in range(la + 1)] for _ in range(2)]   # [parity][x][local y]
    ptr, fin = {}, None
    for ty in range(nty):
        for tz in range(ntz):
            y0, z0 = ty * TY, tz * TZ
            tyl, tzl = min(TY, lb - y0), min(TZ, lc - z0)
            for p in range(2):                                   # zeroed again, whatever the last tile left
                for y in range(TY + 1):
                    buf[p][y] = [ZERO] * (TZ + 1)
            hist = {(y, z): K.history() for y in range(1, tyl + 1) for z in range(1, tzl + 1)}
            yrd = yface[(ty - 1) & 1] if ty else None
            zrd = zface[(tz - 1) & 1] if tz else None
            ywr = yface[ty & 1] if ty + 1 < nty else None
            zwr = zface[tz & 1] if tz + 1 < ntz else None
            if ywr is not None:                                  # what this tile does not store is never read
                for x in range(la + 1):
                    ywr[x][z0 + 1:z0 + tzl + 1] = [POISON] * tzl
            if zwr is not None:
                for x in range(la + 1):
                    zwr[x] = [POISON] * (TY + 1)
            qmax = la + tyl + tzl + (1 if ywr is not None or zwr is not None else 0)
            for q in range(1, qmax + 1):
                rd, wr = buf[(q - 1) & 1], buf[q & 1]
                new = {}                                         # this step's writes, made after all its reads
                for (y, z), h in hist.items():
                    x = q - y - z
                    if x < 0 or x > la:
                        continue
                    out = K.step(h, x, rd[y][z], rd[y - 1][z], rd[y][z - 1], rd[y - 1][z - 1], y0 + y, z0 + z)
                    if out:
                        new[(y, z)], ptr[(x, y0 + y, z0 + z)] = out
                        if on_cell:
                            on_cell(x, y0 + y, z0 + z, out[0], (y - 1) * tzl + (z - 1))
                        if (x, y0 + y, z0 + z) == (la, lb, lc):
                            fin = new[(y, z)]
                for f in range(tzl + tyl + 1):                   # the face threads
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
            for p in range(2):                                   # stale contents the next tile must not see
                for y in range(TY + 1):
                    buf[p][y] = [POISON] * (TZ + 1)
    return max(fin), fin, ptr


def align(a, b, c, match=1, mismatch=-1, go=2, ge=1, sop=False, bits=12, tile=(64, 48)):
    """(score, start, moves), as oracle.align and tsa_align_batch return them;
    tile = (TYmax, TZmax), the caps of the tile edges (align_tile)."""
    score, fin, ptr = emulate(a, b, c, match, mismatch, go, ge, sop, bits, tile)
    start, moves = walk(ptr, fin, len(a), len(b), len(c))
    return score, start, moves
