"""Inputs whose optimal alignment runs through the whole cube, and the geometry
of a reference path over the tile grid of the tiled traceback kernel
(tests/test_align_paths.py). A plain module, no fixtures: the recipes take a
numpy Generator, the geometry takes a path as oracle.align returns it.

A path is (start, moves): start = (x0, y0, z0) on a zero face, move k leads to
the cell the path visits next (tsa.MOVE_CONSUMES). A cell (x, y, z) with
y, z >= 1 belongs to tile ((y-1) // TY, (z-1) // TZ) of the (y, z) plane; the
start itself is no cell and belongs to none."""
import re

import numpy as np

# which of x, y, z a move consumes: MOVES / MOVE_CONSUMES of the package
CONSUMES = ((1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1))


def _sub(rng, seq, rate):
    """seq with about `rate` of its symbols replaced by another symbol of {0..3}."""
    seq = np.asarray(seq, np.uint8).copy()
    hit = rng.random(len(seq)) < rate
    seq[hit] = (seq[hit] + rng.integers(1, 4, int(hit.sum()))) % 4
    return seq


def identical(rng, la, lb, lc, shift=0):
    """One random sequence s: a = s[:la], b = s[:lb], c = s[shift:shift+lc].
    The optimum is the diagonal y = x = z + shift."""
    s = rng.integers(0, 4, max(la, lb, shift + lc)).astype(np.uint8)
    return s[:la].copy(), s[:lb].copy(), s[shift:shift + lc].copy()


def related(rng, la, lb, lc):
    """One base sequence; each of a, b, c is the base with about three deleted
    blocks of 2..11 symbols and about 5 % substitutions, cut to length."""
    n = max(la, lb, lc) + 40                       # three blocks delete at most 33
    base = rng.integers(0, 4, n).astype(np.uint8)
    out = []
    for length in (la, lb, lc):
        keep = np.ones(n, bool)
        for _ in range(3):
            at, width = int(rng.integers(0, n - 11)), int(rng.integers(2, 12))
            keep[at:at + width] = False
        out.append(_sub(rng, base[keep], 0.05)[:length].copy())
    return tuple(out)


def planted(rng, la, lb, lc, run):
    """A random string of the 7 moves in runs of 1..run; every move emits one
    random symbol (3 % substituted per sequence) to the sequences it consumes.
    Stops when a sequence is full; the others are padded randomly."""
    want = (la, lb, lc)
    seqs = ([], [], [])
    full = False
    while not full:
        move = int(rng.integers(0, 7))
        for _ in range(int(rng.integers(1, run + 1))):
            sym = int(rng.integers(0, 4))
            for k in range(3):
                if CONSUMES[move][k]:
                    seqs[k].append((sym + int(rng.integers(1, 4))) % 4 if rng.random() < 0.03 else sym)
            full = any(len(seqs[k]) >= want[k] for k in range(3))
            if full:
                break
    return tuple(np.concatenate([np.asarray(seqs[k][:want[k]], np.uint8),
                                 rng.integers(0, 4, max(want[k] - len(seqs[k]), 0)).astype(np.uint8)])
                 for k in range(3))


def plan_tiles(tsa, n, la, lb, lc):
    """(TY, TZ, nty, ntz) of a triple under the current overrides, from
    tsa.describe_align_plan; a triple that is not tiled is one tile."""
    txt = tsa.describe_align_plan(n, la, lb, lc)
    m = re.search(r"^tiled tile=(\d+)x(\d+) tiles=(\d+)x(\d+) ", txt)
    return tuple(int(v) for v in m.groups()) if m else (lb, lc, 1, 1)


def path_cells(start, moves):
    """The cells (x, y, z) a path visits, in order."""
    pos, out = list(start), []
    for t in moves:
        pos = [p + d for p, d in zip(pos, CONSUMES[int(t)])]
        out.append(tuple(pos))
    return out


def path_geometry(start, moves, TY, TZ):
    """(tiles, ny, nz, ncorner): the set of tiles (ty, tz) the path's cells lie
    in and the number of moves between two cells that cross only a y seam,
    only a z seam, and both at once (a tile corner)."""
    tiles, ny, nz, ncorner = set(), 0, 0, 0
    prev = None
    for _, y, z in path_cells(start, moves):       # a path leaves its zero face with the first move: y, z >= 1
        tile = ((y - 1) // TY, (z - 1) // TZ)
        tiles.add(tile)
        if prev is not None and tile != prev:
            dy, dz = tile[0] != prev[0], tile[1] != prev[1]
            ny += dy and not dz
            nz += dz and not dy
            ncorner += dy and dz
        prev = tile
    return tiles, ny, nz, ncorner


def move_pairs(moves):
    """The distinct (previous move, next move) pairs of a path."""
    return {(int(p), int(n)) for p, n in zip(moves[:-1], moves[1:])}
