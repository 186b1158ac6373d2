"""The grid path of batched traceback (csrc/align_grid_kernel.hip, tb_walk_grid,
align_mode=grid, tsa_align_batch_grid): a triple whose (y,z) plane does not fit
one workgroup keeps the last row and the last column of every tile. A forward
launch per anti-diagonal of the tile grid sweeps that diagonal's tiles as
separate workgroups; then only the tile the walker stands in is swept again,
with pointers into a cube of one tile and only up to the walker's x, each sweep
followed by a segment walk that may leave through a y seam, a z seam or the
corner. Everything must come out as the oracle's independent traceback gives
it: score, start and moves.

The plan text, the argument checks and the schedule's CPU replay
(tools/align_grid_emu.py) need no device. Every test asserts on the oracle's
path (ac.path_geometry) that its inputs exercise what it is about."""
import ctypes
import functools
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

import _align_cases as ac  # noqa: E402
import test_align_paths as tp  # noqa: E402
import test_align_strip as ts  # noqa: E402

KWS = tp.KWS                                                       # the six parameter sets
SEEDS = (900, 901, 902)
EMU_TILES = [(4, 4), (5, 7), (1, 1), (13, 2)]
_same, _rand_triple, _cube_bytes, _geom, _strip_need, _raw_call = (
    ts._same, ts._rand_triple, ts._cube_bytes, ts._geom, ts._strip_need, ts._raw_call)


def _grid_need(la, lb, lc, tymax, tzmax):
    """(tile cube bytes, kept face bytes) of include/trialign.h's need formula."""
    TY, TZ, nty, ntz = _geom(lb, lc, tymax, tzmax)
    return 4 * TY * (la + TZ - 1) * TZ, 16 * ((nty - 1) * la * (lc + 1) + (ntz - 1) * la * lb)


def _path_tiles(ref, TY, TZ):
    """The tiles a reference alignment visits, in the order of the path."""
    out = []
    for _, y, z in ac.path_cells(ref[1], ref[2]):
        tile = ((y - 1) // TY, (z - 1) // TZ)
        if not out or out[-1] != tile:
            out.append(tile)
    return out


def _geometry(ref, TY, TZ):
    return ac.path_geometry(ref[1], ref[2], TY, TZ)


# ---- CPU ---------------------------------------------------------------------

def test_grid_plan_text(tsa):
    with tsa.overrides(align_mode="grid", align_tile="8x8"):
        assert tsa.describe_align_plan(1, 10, 20, 20) == "grid tile=7x7 tiles=3x3 lds=2080 cube=3136 faces=13120"
        assert (3136, 13120) == _grid_need(10, 20, 20, 8, 8)
        assert 3136 == 4 * 7 * (10 + 7 - 1) * 7 and 13120 == 16 * (2 * 10 * 21 + 2 * 10 * 20)
    with tsa.overrides(align_mode="grid", align_tile="4x4"):
        assert tsa.describe_align_plan(1, 8, 4, 4).startswith("resident")      # a fitting triple
        assert tsa.describe_align_plan(1, 8, 4, 5).startswith("grid tile=4x3 tiles=1x2 ")
    with tsa.overrides(align_mode="grids"):
        assert ts._plan_rc(tsa, 1, 8, 13, 13)[0] == tsa.TSA_EINVAL
    with tsa.overrides(align_mode="grid"):
        assert ts._plan_rc(tsa, 1, 8, 13, 13)[0] == tsa.TSA_OK
        for n in (1, 256):                                         # the default tile, any group size
            txt = tsa.describe_align_plan(n, 256, 256, 256)
            assert txt.startswith("grid tile=64x43 tiles=4x6 "), txt
            assert tuple(int(v) for v in re.search(r" cube=(\d+) faces=(\d+)$", txt).groups()) == \
                _grid_need(256, 256, 256, 64, 48)
    # without the override nothing changes: the plans of the parent
    assert tsa.describe_align_plan(1, 256, 256, 256) == "plane"
    assert tsa.describe_align_plan(256, 256, 256, 256) == "tiled tile=64x43 tiles=4x6 lds=91888 faces=%d" % (
        32 * 256 * 257 + 32 * 256 * 64)


def test_align_batch_grid_is_exported_and_validates_as_align_batch(tsa):
    """Validation comes before any device work: the same codes as tsa_align_batch's on any host."""
    assert "tsa_align_batch_grid" in tsa.EXPORTS
    assert hasattr(tsa.lib(), "tsa_align_batch_grid")
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "trialign.h")) as f:
        assert re.search(r"\bint tsa_align_batch_grid\(", f.read())
    p = tsa.TsaParams.default()
    seqs, offs = tsa.pack_batch([([0, 1], [1, 2], [2, 3]), ([0], [1], [2])])
    bad = seqs.copy()
    bad[1] = 9                                                     # a symbol > 4
    calls = [(seqs, offs, 2, p, null) for null in ("seqs", "offsets", "scores", "moves", "n_moves", "starts")]
    calls += [(seqs, offs, -1, p, None),
              (np.zeros(6, np.uint8), np.array([0, 3, 2, 6], np.int64), 1, p, None),      # non-monotone offsets
              (bad, offs, 2, p, None),
              (seqs, offs, 2, tsa.TsaParams.default(score_bits=3), None)]
    for args in calls:
        rc = _raw_call(tsa, "tsa_align_batch_grid", *args)
        assert rc == tsa.TSA_EINVAL, args[2:]
        assert rc == _raw_call(tsa, "tsa_align_batch", *args), args[2:]
    assert _raw_call(tsa, "tsa_align_batch_grid", np.zeros(1, np.uint8), np.zeros(1, np.int64), 0, p) == tsa.TSA_OK
    assert tsa.align_batch([], grid=True) == []
    with pytest.raises(tsa.TsaError) as e:
        tsa.align_batch([([0, 7], [1], [2])], grid=True)
    assert e.value.rc == tsa.TSA_EINVAL
    with pytest.raises(tsa.TsaError) as e:                         # one plan mode a call
        tsa.align_batch([], grid=True, lowmem=True)
    assert e.value.rc == tsa.TSA_EINVAL


def _emu(a, b, c, op, tile):
    import align_grid_emu
    return align_grid_emu.emulate(a, b, c, op.match, op.mismatch, op.gap_open, op.gap_extend, bool(op.s3_mode),
                                  op.score_bits, tile)


@pytest.mark.parametrize("kw", KWS)
def test_grid_schedule_emulated_matches_oracle(orc, kw):
    """tools/align_grid_emu.py -- the forward diagonals into poisoned kept
    faces, the walker's tile swept into a tile cube cleared before every sweep
    and trimmed to the walker's x, the segment walks, the early end -- against
    the oracle, move for move; and the tiles swept backward are exactly the
    tiles of the reference path, last first."""
    rng = np.random.default_rng(41 + len(kw) + kw.get("score_bits", 1))
    op = orc.default_params(**kw)
    shapes = [tuple(int(v) for v in rng.integers(1, 15, 3)) for _ in range(3)]
    trips = [_rand_triple(rng, *s, hi=5) for s in shapes + [(1, 9, 9), (9, 1, 9), (9, 9, 1), (1, 1, 1)]]
    trips += [ac.identical(rng, 14, 14, 14), ac.identical(rng, 6, 13, 9, shift=2)]
    crossings = np.zeros(3, int)
    for a, b, c in trips:
        ref = orc.align(a, b, c, op)
        for tile in EMU_TILES:
            got = _emu(a, b, c, op, tile)
            where = (kw, len(a), len(b), len(c), tile)
            assert _same(got, ref), where
            TY, TZ = _geom(len(b), len(c), *tile)[:2]
            assert got[3] == _path_tiles(ref, TY, TZ)[::-1], where
            crossings += _geometry(ref, TY, TZ)[1:]
    assert crossings.min() > 0, crossings                          # y seams, z seams and corners were all crossed


def test_grid_emu_sweeps_only_the_tiles_on_the_path(orc):
    """A diagonal path over a 4x4 grid has its 4 diagonal tiles swept and no other; one that ends in the last
    tile leaves all the others unswept."""
    import align_grid_emu
    op = orc.default_params()
    rng = np.random.default_rng(42)
    a, b, c = ac.identical(rng, 14, 14, 14)
    assert _emu(a, b, c, op, (4, 4))[3] == [(3, 3), (2, 2), (1, 1), (0, 0)]
    assert align_grid_emu.align(a, b, c, tile=(4, 4))[0] == 3 * 14
    seen = set()
    for _ in range(6):
        a, b, c = _rand_triple(rng, 3, 14, 14)
        ref = orc.align(a, b, c, op)
        got = _emu(a, b, c, op, (4, 4))
        assert _same(got, ref)
        assert got[3] == _path_tiles(ref, 4, 4)[::-1]
        assert set(got[3]) == _geometry(ref, 4, 4)[0]
        seen.add(tuple(got[3]))
    assert ((3, 3),) in seen                                       # some path stayed in the last tile


def test_grid_emu_geometry_is_the_library_s(tsa):
    import align_grid_emu
    for lb, lc, tile in ((13, 13, (4, 4)), (40, 1, (5, 7)), (130, 50, (64, 48)), (129, 96, (64, 48)), (6, 6, (1, 1))):
        geom = align_grid_emu.tile_geom(lb, lc, *tile)
        assert geom == _geom(lb, lc, *tile)
        with tsa.overrides(align_mode="grid", align_tile="%dx%d" % tile):
            txt = tsa.describe_align_plan(1, 8, lb, lc)
        assert txt.startswith("grid tile=%dx%d tiles=%dx%d " % geom), (lb, lc, tile, txt)
        assert txt.endswith(" cube=%d faces=%d" % _grid_need(8, lb, lc, *tile)), txt


# ---- GPU ---------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _ref(orc, key):
    """The triples of a named case and their oracle alignments, computed once."""
    trips = []
    if key == "seams":                                             # tile 8x8
        trips = [ac.related(np.random.default_rng(k), 24, 24, 24) for k in SEEDS]
        trips.append(ac.identical(np.random.default_rng(900), 20, 20, 20))
        trips.append(ac.identical(np.random.default_rng(900), 20, 20, 13, shift=7))
    elif key == "cells":                                           # tile 1x1: every cell of the plane a tile
        trips.append(ac.identical(np.random.default_rng(900), 5, 6, 6))
    elif key == "early":                                           # tile 8x8: 5x5 tiles, the path in the last
        trips = [_rand_triple(np.random.default_rng(k), 3, 40, 40) for k in SEEDS]
        trips.append(ac.identical(np.random.default_rng(900), 20, 20, 20))
    op = orc.default_params()
    return trips, [orc.align(a, b, c, op) for a, b, c in trips]


def _check(gpu, trips, ref, params=None, modes=("grid",), **ov):
    for mode in modes:
        with gpu.overrides(align_mode=mode, **ov):
            got = gpu.align_batch(trips, params)
        assert len(got) == len(trips)
        for i, (g, r) in enumerate(zip(got, ref)):
            assert _same(g, r), (mode, i, tuple(len(s) for s in trips[i]), g[:2], r[:2])


def _grid_launches(shapes, budget, tymax, tzmax):
    """[resident] + max (nty+ntz-2) + max (nty+ntz-1) summed over the chunks of include/trialign.h's rule;
    also the number of chunks."""
    total, chunks, i = 0, 0, 0
    while i < len(shapes):
        used, res, diag = 0, False, []
        while i < len(shapes):
            la, lb, lc = shapes[i]
            over = lb > tymax or lc > tzmax
            need = sum(_grid_need(la, lb, lc, tymax, tzmax)) if over else _cube_bytes(la, lb, lc)
            assert need <= budget
            if used + need > budget:
                break
            used += need
            if over:
                g = _geom(lb, lc, tymax, tzmax)
                diag.append(g[2] + g[3] - 1)
            else:
                res = True
            i += 1
        total += int(res) + (2 * max(diag) - 1 if diag else 0)
        chunks += 1
    return total, chunks


@pytest.mark.gpu
def test_gpu_grid_every_seam(gpu, orc):
    """Tile cap 8x8, all in one call: related 24^3 paths through 4 (seed 900: 1 y seam, 2 z seams) and 5 tiles
    (seeds 901, 902: 2 y seams, 2 z seams) of 3x3, the diagonal of 20^3 through 2 corners, and a shifted
    diagonal that starts off the y = 0 face and crosses one corner of a 3x2 grid. The first case also against strip, tiled
    and plane under the same tile."""
    trips, ref = _ref(orc, "seams")
    with gpu.overrides(align_mode="grid", align_tile="8x8"):
        assert gpu.describe_align_plan(1, 24, 24, 24).startswith("grid tile=8x8 tiles=3x3 ")
        assert gpu.describe_align_plan(1, 20, 20, 20).startswith("grid tile=7x7 tiles=3x3 ")
        assert gpu.describe_align_plan(1, 20, 20, 13).startswith("grid tile=7x7 tiles=3x2 ")
    geo = [_geometry(ref[i], 8, 8) for i in range(3)]
    for i, (tiles, ny, nz, ncorner) in enumerate(geo):             # y seams and z seams, one at a time
        assert ny >= 1 and nz >= 2 and ncorner == 0 and len(tiles) == ny + nz + 1, (i, geo[i])
    for tiles, ny, nz, ncorner in geo[1:]:                         # nty + ntz - 1 tiles: as many as a path can visit
        assert (len(tiles), ny, nz) == (5, 2, 2)
    assert _geometry(ref[3], 7, 7) == ({(0, 0), (1, 1), (2, 2)}, 0, 0, 2)
    assert _geometry(ref[4], 7, 7) == ({(1, 0), (2, 1)}, 0, 0, 1)
    assert tuple(ref[4][1]) == (7, 7, 0)
    _check(gpu, trips, ref, align_tile="8x8")
    _check(gpu, trips[:3], ref[:3], modes=("strip", "tiled", "plane"), align_tile="8x8")


@pytest.mark.gpu
def test_gpu_grid_every_cell_a_tile(gpu, orc):
    """identical (5,6,6) under 1x1: a 6x6 grid, 5 corners; 10 forward and 11 backward launches."""
    trips, ref = _ref(orc, "cells")
    tiles, ny, nz, ncorner = _geometry(ref[0], 1, 1)
    assert (ny, nz, ncorner) == (0, 0, 5) and tiles == {(k, k) for k in range(6)}
    with gpu.overrides(align_mode="grid", align_tile="1x1"):
        assert gpu.describe_align_plan(1, 5, 6, 6).startswith("grid tile=1x1 tiles=6x6 ")
        before = gpu.kernel_launch_count()
        got = gpu.align_batch(trips)
        assert gpu.kernel_launch_count() - before == 21
    assert _same(got[0], ref[0]), (got[0][:2], ref[0][:2])


@pytest.mark.gpu
def test_gpu_grid_early_end(gpu, orc):
    """Paths inside the last of 5x5 tiles: no other tile of theirs is swept backward, while a triple whose path
    crosses its grid is live in the same launches; the launches are queued all the same."""
    trips, ref = _ref(orc, "early")
    with gpu.overrides(align_mode="grid", align_tile="8x8"):
        assert gpu.describe_align_plan(1, 3, 40, 40).startswith("grid tile=8x8 tiles=5x5 ")
    for i in range(3):
        assert _geometry(ref[i], 8, 8)[0] == {(4, 4)}, i
    assert _geometry(ref[3], 7, 7)[0] == {(0, 0), (1, 1), (2, 2)}
    with gpu.overrides(align_mode="grid", align_tile="8x8"):
        before = gpu.kernel_launch_count()
        got = gpu.align_batch(trips)
        assert gpu.kernel_launch_count() - before == (5 + 5 - 2) + (5 + 5 - 1)
    for i, (g, r) in enumerate(zip(got, ref)):
        assert _same(g, r), (i, g[:2], r[:2])


@pytest.mark.gpu
@pytest.mark.parametrize("key,shape,tile,tiles", [("k2", (130, 130, 50), "44x25", "3x2"),
                                                  ("k3", (129, 129, 96), "43x48", "3x2")])
def test_gpu_grid_two_and_three_positions_a_thread(gpu, orc, key, shape, tile, tiles):
    """The default tile: 1100 positions (K = 2) and 2064 (K = 3); test_align_strip's identical and related cases."""
    trips, ref = ts._ref(orc, key)
    with gpu.overrides(align_mode="grid"):
        assert gpu.describe_align_plan(1, *shape).startswith("grid tile=%s tiles=%s " % (tile, tiles))
    TY, TZ = (int(v) for v in tile.split("x"))
    for i in range(len(trips)):
        tiles, ny, nz, ncorner = _geometry(ref[i], TY, TZ)
        assert len(tiles) >= 3 and ny >= 1 and nz + ncorner >= 1, i  # every path changes tile row and tile column
    _check(gpu, trips, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("ki", [1, 3, 5])
def test_gpu_grid_arithmetic(gpu, orc, ki):
    """TSA_S3_SOP, score_bits 6 (wrapped candidates, equal argmaxes) and a 16-bit set on 24 planted triples of
    lengths 8 .. 40 under 8x8."""
    trips, ref = tp._tiny(orc, ki)
    assert len(trips) == 24
    geo = [_geometry(r, *_geom(len(t[1]), len(t[2]), 8, 8)[:2]) for t, r in zip(trips, ref)]
    assert max(len(g[0]) for g in geo) >= 7
    assert sum(g[1] for g in geo) > 0 and sum(g[2] for g in geo) > 0
    assert ki == 3 or sum(g[3] for g in geo) > 0                   # corners too, but for the 6-bit paths
    _check(gpu, trips, ref, gpu.TsaParams.default(**KWS[ki]), align_tile="8x8")


@pytest.mark.gpu
def test_gpu_grid_mixed_batch(gpu, orc):
    """test_align_strip's mixed shapes -- resident triples, nty = 1, ntz = 1, lb != lc -- in one chunk and, under a
    cut budget, in at least 3: in the caller's order, with the counted launches of the header's rule."""
    trips, ref = ts._ref(orc, "mixed")
    shapes = [tuple(len(s) for s in t) for t in trips]
    with gpu.overrides(align_mode="grid", align_tile="8x8"):
        plans = [gpu.describe_align_plan(len(trips), *s) for s in shapes]
        assert [p.split()[0] for p in plans].count("resident") == 3
        grids = {tuple(int(v) for v in re.search(r"tiles=(\d+)x(\d+)", p).groups()) for p in plans
                 if p.startswith("grid")}
        assert any(g[0] == 1 for g in grids) and any(g[1] == 1 for g in grids) and (4, 4) in grids, grids
        before = gpu.kernel_launch_count()
        got = gpu.align_batch(trips)
        assert gpu.kernel_launch_count() - before == 1 + 6 + 7     # resident, then the 4x4 grid's diagonals
    assert _grid_launches(shapes, 1 << 40, 8, 8) == (14, 1)
    for i in range(len(trips)):
        assert _same(got[i], ref[i]), i
    need = [sum(_grid_need(*s, 8, 8)) if (s[1] > 8 or s[2] > 8) else _cube_bytes(*s) for s in shapes]
    budget = max(need) + min(need)
    want, chunks = _grid_launches(shapes, budget, 8, 8)
    assert chunks >= 3
    with gpu.overrides(align_mode="grid", align_tile="8x8", align_tb_bytes=budget):
        before = gpu.kernel_launch_count()
        first = gpu.align_batch(trips)
        count = gpu.kernel_launch_count() - before
        second = gpu.align_batch(trips)
    assert count == want
    for i in range(len(trips)):
        assert _same(first[i], ref[i]), i
        assert _same(second[i], ref[i]), i


@pytest.mark.gpu
def test_gpu_grid_aligns_what_the_strip_budget_refuses(gpu, orc):
    """12 x (10,20,20) under tile 8x8 with a budget of 20000 bytes: strip (need 25200) is TSA_ENOMEM, grid (need
    16256) gives the oracle's alignments; one byte below the grid need is TSA_ENOMEM."""
    trips, ref = ts._ref(orc, "capability")
    need = sum(_grid_need(10, 20, 20, 8, 8))
    assert need == 16256 and sum(_strip_need(10, 20, 20, 8, 8)) == 25200
    with gpu.overrides(align_mode="strip", align_tile="8x8", align_tb_bytes=20000):
        with pytest.raises(gpu.TsaError) as e:
            gpu.align_batch(trips)
        assert e.value.rc == gpu.TSA_ENOMEM
    for budget in (20000, need):
        with gpu.overrides(align_mode="grid", align_tile="8x8", align_tb_bytes=budget):
            before = gpu.kernel_launch_count()
            got = gpu.align_batch(trips)
            assert gpu.kernel_launch_count() - before == 12 * (4 + 5)  # a chunk per triple
        for i in range(12):
            assert _same(got[i], ref[i]), (budget, i)
    for kw in (dict(align_mode="grid"), dict()):
        with gpu.overrides(align_tile="8x8", align_tb_bytes=need - 1, **kw):
            with pytest.raises(gpu.TsaError) as e:
                gpu.align_batch(trips, grid=True)
            assert e.value.rc == gpu.TSA_ENOMEM


@pytest.mark.gpu
def test_gpu_grid_entry_point_keeps_a_set_align_mode(gpu, orc):
    """align_batch(grid=True) with no align_mode makes the grid launches; a set align_mode = plane holds and makes
    no counted launch."""
    trips, ref = _ref(orc, "seams")
    with gpu.overrides(align_tile="8x8"):
        before = gpu.kernel_launch_count()
        got = gpu.align_batch(trips, grid=True)
        assert gpu.kernel_launch_count() - before == 4 + 5         # 3x3 tiles
    assert all(_same(g, r) for g, r in zip(got, ref))
    with gpu.overrides(align_mode="plane", align_tile="8x8"):
        before = gpu.kernel_launch_count()
        got = gpu.align_batch(trips, grid=True)
        assert gpu.kernel_launch_count() - before == 0
    assert all(_same(g, r) for g, r in zip(got, ref))


@pytest.mark.gpu
def test_gpu_grid_unstaged_a(gpu, orc):
    """(163900,3,4) under 2x2: A does not fit LDS beside the tile and is read from global memory, forward and
    backward, next to triples that stage it."""
    trips, refs = tp._unstaged_cases(), tp._unstaged_refs(orc)
    shapes = [tuple(len(s) for s in t) for t in trips]
    assert shapes[2] == (163900, 3, 4)
    assert 32 * 3 * 3 + 2 + 2 + 163900 > tp.LDS_MAX                # align_stage_a declines for a 2x2 tile
    with gpu.overrides(align_mode="grid", align_tile="2x2"):
        assert gpu.describe_align_plan(4, 163900, 3, 4).startswith("grid tile=2x2 tiles=2x2 ")
    assert len(_geometry(refs[2], 2, 2)[0]) >= 2                   # the path changes tiles
    _check(gpu, trips, refs, align_tile="2x2")
