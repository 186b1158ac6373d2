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

import numpy as np

from align_emu import _wrap, walk
from literal_emu import penalties

POISON = tuple(12345 - 1111 * s for s in range(7))


def tile_geom(lb, lc, tymax, tzmax):
    """(TY, TZ, nty, ntz): align_tile_geom of csrc/align_kernel.h."""
    nty, ntz = -(-lb // tymax), -(-lc // tzmax)
    return -(-lb // nty), -(-lc // ntz), nty, ntz


def emulate(a, b, c, match=1, mismatch=-1, go=2, ge=1, sop=False, bits=12, tile=(64, 48)):
    """(score, final7, ptr) by the tiled schedule; ptr maps a cell (x, y, z)
    in global coordinates to its pointer word."""
    a, b, c = (np.asarray(s, np.int64) & 3 for s in (a, b, c))
    la, lb, lc = len(a), len(b), len(c)
    TY, TZ, nty, ntz = tile_geom(lb, lc, *tile)
    Pen = penalties(go, ge)
    w = lambda v: _wrap(int(v), bits)
    mt, mm = w(match), w(mismatch)
    s3_eq, s3_ab, s3_ne = w(3 * match), w(2 * (match + mismatch)), w(3 * mismatch)
    zero = (0,) * 7
    buf = [[[POISON] * (TZ + 1) for _ in range(TY + 1)] for _ in range(2)]
    yface = [[[POISON] * (lc + 1) for _ in range(la + 1)] for _ in range(2)]   # [parity][x][global z]
    zface = [[[POISON] * (TY + 1) for _ in range(la + 1)] for _ in range(2)]   # [parity][x][local y]
    ptr, fin = {}, None

    def max7(T, pred, add):
        best, arg = None, 0
        for s in range(7):
            v = w(pred[s] - int(Pen[T][s]) + add)
            if best is None or v > best:
                best, arg = v, s
        return best, arg

    def adds(x, gy, gz):
        """(sab, sbc, sac, s3) of cell (x, gy, gz); x clamped into A as the kernel's lookup."""
        ax, by, cz = int(a[min(max(x, 1), la) - 1]), int(b[gy - 1]), int(c[gz - 1])
        sab = mt if ax == by else mm
        sbc = mt if by == cz else mm
        sac = mt if ax == cz else mm
        if sop:
            s3 = w(sab + sbc + sac)
        else:
            s3 = (s3_eq if by == cz else s3_ab) if ax == by else s3_ne
        return sab, sbc, sac, s3

    for ty in range(nty):
        for tz in range(ntz):
            y0, z0 = ty * TY, tz * TZ
            tyl, tzl = min(TY, lb - y0), min(TZ, lc - z0)
            for p in range(2):                                   # zeroed again, whatever the last tile left
                for y in range(TY + 1):
                    buf[p][y] = [zero] * (TZ + 1)
            hist = {(y, z): dict(XY=(0, 0), YZ=(0, 0), XZ=(0, 0), M3=(0, 0), M2=(0, 0))
                    for y in range(1, tyl + 1) for z in range(1, tzl + 1)}
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
                    gy, gz = y0 + y, z0 + z
                    own, n1, w1, nw1 = rd[y][z], rd[y - 1][z], rd[y][z - 1], rd[y - 1][z - 1]
                    if x == 0:
                        h["M3"] = max7(0, zero, adds(1, gy, gz)[3])
                    else:
                        res = [h["M3"], max7(1, own, 0), max7(2, n1, 0), max7(3, w1, 0), h["XY"], h["YZ"], h["XZ"]]
                        new[(y, z)] = tuple(v for v, _ in res)
                        ptr[(x, gy, gz)] = sum(g << (3 * T) for T, (_, g) in enumerate(res))
                        if (x, gy, gz) == (la, lb, lc):
                            fin = new[(y, z)]
                        h["M3"] = h["M2"]
                    sab, sbc, sac, _ = adds(x + 1, gy, gz)
                    h["XY"], h["XZ"], h["YZ"] = max7(4, n1, sab), max7(6, w1, sac), max7(5, nw1, sbc)
                    h["M2"] = max7(0, nw1, adds(x + 2, gy, gz)[3])
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
