"""tsa_align_batch_grid_ends: the grid path of batched traceback with a free
end (the END forms of csrc/align_grid_kernel.hip). The forward launches sweep
every tile, the last one included, and keep one end key per tile; a helper
kernel takes the max over a triple's keys and writes score, end record and
walker record; the backward launches start at the end cell's tile, trimmed to
the end cell's x, and write pointer words alone.

The reference is tests/test_align_ends.py's: the oracle brute-forced over the
candidate prefixes, the first maximum in (x, y, z) order, then oracle.align on
those prefixes. Where all the prefixes are too many (the K = 2 and K = 3 cubes,
the unstaged A) the face candidates alone are brute-forced, and TSA_END_ANY
takes oracle.best_range where oracle.state_range shows that nothing wraps
(test_align_ends.test_unstaged_reference argues and checks that rule). Every
test first asserts on the reference alone what it claims to exercise.

Without the feature every test below fails on the missing symbol, the missing
`grid` keyword or the missing tools/align_grid_ends_emu.py."""
import ctypes
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG_DIR, ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import _align_cases as ac  # noqa: E402
import test_align_ends as te  # noqa: E402
import test_align_grid as tg  # noqa: E402
import test_align_paths as tp  # noqa: E402
import test_align_strip as ts  # noqa: E402

ref_end, refs_of, same, check_path, _early_cube, CASES = (
    te.ref_end, te.refs_of, te.same, te.check_path, te._early_cube, te.CASES)
_grid_need, _geometry, _path_tiles = tg._grid_need, tg._geometry, tg._path_tiles
_geom, _cube_bytes = ts._geom, ts._cube_bytes
KWS, MODES = te.KWS, te.MODES
FN = "tsa_align_batch_grid_ends"


def _tile_of(end, TY, TZ):
    return (end[1] - 1) // TY, (end[2] - 1) // TZ


def _uniform(seed, la, lb, lc):
    return te._uniform(np.random.default_rng(seed), la, lb, lc)


def _raw(tsa, fn, seqs, offsets, n, p, end_mode, null=None):
    """fn (tsa_align_batch_ends or tsa_align_batch_grid_ends) with fresh output
    buffers; the argument named by `null` is passed as NULL."""
    u8, i32, i64 = (ctypes.POINTER(t) for t in (ctypes.c_uint8, ctypes.c_int32, ctypes.c_int64))
    seqs = np.ascontiguousarray(seqs, np.uint8)
    offsets = np.ascontiguousarray(offsets, np.int64)
    m = max(abs(n), 1)
    out = dict(scores=np.zeros(m, np.int32), moves=np.zeros(max(len(seqs), 1), np.uint8),
               n_moves=np.zeros(m, np.int32), starts=np.zeros(3 * m, np.int32), ends=np.zeros(3 * m, np.int32))
    arg = lambda k, t: None if k == null else out[k].ctypes.data_as(t)
    return getattr(tsa.lib(), fn)(None if null == "seqs" else seqs.ctypes.data_as(u8),
                                  None if null == "offsets" else offsets.ctypes.data_as(i64), n, ctypes.byref(p),
                                  end_mode, arg("scores", i32), arg("moves", u8), arg("n_moves", i32),
                                  arg("starts", i32), arg("ends", i32), 0)


# ---- CPU: the interface ---------------------------------------------------------

def test_grid_ends_is_exported(tsa):
    import inspect
    assert FN in tsa.EXPORTS and hasattr(tsa.lib(), FN)
    with open(os.path.join(ROOT, "include", "trialign.h")) as f:
        assert re.search(r"\bint tsa_align_batch_grid_ends\(", f.read())
    assert inspect.signature(tsa.align_batch_ends).parameters["grid"].default is False
    assert tsa.align_batch_ends([], end="face", grid=True) == []


def test_grid_ends_validates_as_align_batch_ends(tsa):
    """Validation comes before any device work: the codes of tsa_align_batch_ends
    on any host, TSA_OK for an empty batch and TSA_ENODEV without a device."""
    p = tsa.TsaParams.default()
    seqs, offs = tsa.pack_batch([([0, 1], [1, 2], [2, 3]), ([0], [1], [2])])
    bad = seqs.copy()
    bad[1] = 9                                                     # a symbol > 4
    calls = [(seqs, offs, 2, p, null) for null in ("seqs", "offsets", "scores", "moves", "n_moves", "starts", "ends")]
    calls += [(seqs, offs, -1, p, None),
              (np.zeros(6, np.uint8), np.array([0, 3, 2, 6], np.int64), 1, p, None),      # non-monotone offsets
              (bad, offs, 2, p, None),
              (seqs, offs, 2, tsa.TsaParams.default(score_bits=3), None)]
    for mode in (tsa.END_CORNER, tsa.END_FACE, tsa.END_ANY):
        for s, o, n, q, null in calls:
            rc = _raw(tsa, FN, s, o, n, q, mode, null)
            assert rc == tsa.TSA_EINVAL, (mode, n, null)
            assert rc == _raw(tsa, "tsa_align_batch_ends", s, o, n, q, mode, null)
        assert _raw(tsa, FN, np.zeros(1, np.uint8), np.zeros(1, np.int64), 0, p, mode) == tsa.TSA_OK
    for mode in (3, -1):
        assert _raw(tsa, FN, seqs, offs, 2, p, mode) == tsa.TSA_EINVAL
        assert _raw(tsa, FN, np.zeros(1, np.uint8), np.zeros(1, np.int64), 0, p, mode) == tsa.TSA_EINVAL
    with pytest.raises(tsa.TsaError) as e:
        tsa.align_batch_ends([([0, 7], [1], [2])], end="any", grid=True)
    assert e.value.rc == tsa.TSA_EINVAL
    with pytest.raises(tsa.TsaError) as e:
        tsa.align_batch_ends([([0], [1], [2])], end="middle", grid=True)
    assert e.value.rc == tsa.TSA_EINVAL
    if tsa.device_count() == 0:                                    # no CPU fall-back
        for end in ("corner", "face", "any"):
            with pytest.raises(tsa.TsaError) as e:
                tsa.align_batch_ends([([0, 1], [0, 1], [0, 1])], end=end, grid=True)
            assert e.value.rc == tsa.TSA_ENODEV


def test_grid_ends_overrides(tsa):
    """align_mode = plane or strip: TSA_EINVAL under face and any, found without
    a device. grid, resident, tiled and no override go on to the device, and so
    does corner under every one of them. tsa_align_batch_ends itself still
    refuses grid."""
    p = tsa.TsaParams.default()
    seqs, offs = tsa.pack_batch([([0, 1], [1, 2], [2, 3])])
    beyond = tsa.TSA_OK if tsa.device_count() > 0 else tsa.TSA_ENODEV
    for mode in ("plane", "strip"):
        with tsa.overrides(align_mode=mode):
            assert _raw(tsa, FN, seqs, offs, 1, p, tsa.END_ANY) == tsa.TSA_EINVAL, mode
            assert _raw(tsa, FN, seqs, offs, 1, p, tsa.END_FACE) == tsa.TSA_EINVAL, mode
            assert _raw(tsa, FN, seqs, offs, 1, p, tsa.END_CORNER) == beyond, mode
    for mode in ("grid", "resident", "tiled"):
        with tsa.overrides(align_mode=mode):
            for end in (tsa.END_CORNER, tsa.END_FACE, tsa.END_ANY):
                assert _raw(tsa, FN, seqs, offs, 1, p, end) == beyond, (mode, end)
    for end in (tsa.END_CORNER, tsa.END_FACE, tsa.END_ANY):
        assert _raw(tsa, FN, seqs, offs, 1, p, end) == beyond, end
    with tsa.overrides(align_mode="grid"):
        assert _raw(tsa, "tsa_align_batch_ends", seqs, offs, 1, p, tsa.END_ANY) == tsa.TSA_EINVAL
    with tsa.overrides(align_mode="grids"):
        assert _raw(tsa, FN, seqs, offs, 1, p, tsa.END_ANY) == tsa.TSA_EINVAL


def test_cli_grid_option():
    """--grid without --align is a usage error (exit 2); with --align it gets as
    far as the device, and --end corner --grid prints what --grid prints."""
    cli = os.path.join(PKG_DIR, "bin", "tsa")
    dat = os.path.join(ROOT, "tests", "golden", "dat")
    files = [f"{dat}/A_seq.dat", f"{dat}/B_seq.dat", f"{dat}/C_seq.dat"]
    run = lambda *extra: subprocess.run([cli, *files, *extra], capture_output=True, text=True)
    assert run("--grid").returncode == 2
    assert run("--grid", "--end", "any").returncode == 2
    assert run("--score-end", "any", "--grid").returncode == 2
    for end in (None, "corner", "face", "any"):
        r = run("--align", "--grid", *(("--end", end) if end else ()))
        if r.returncode == 0:
            assert "alignment start" in r.stdout
            assert ("alignment end (x1,y1,z1) = (" in r.stdout) == (end in ("face", "any"))
        else:
            assert r.returncode == 1 and "no HIP device" in r.stderr and "usage" not in r.stderr
    plain, corner = run("--align", "--grid"), run("--align", "--end", "corner", "--grid")
    assert (plain.returncode, plain.stdout) == (corner.returncode, corner.stdout)


# ---- CPU: the replay ------------------------------------------------------------

def _emu(a, b, c, mode, op, tile):
    import align_grid_ends_emu as emu
    return emu.emulate(a, b, c, emu.END_MODES[mode], *te._emu_args(op), tile=tile)


def _check_replay(orc, a, b, c, kw, mode, tile):
    ref, _ = ref_end(orc, a, b, c, kw, mode)
    got = _emu(a, b, c, mode, orc.default_params(**kw), tile)
    assert same(got, ref), (kw, mode, tile, got[3], ref[3])
    TY, TZ = _geom(len(b), len(c), *tile)[:2]
    tiles = _path_tiles(ref, TY, TZ)[::-1]
    assert got[4] == tiles and tiles[0] == _tile_of(ref[3], TY, TZ), (kw, mode, tile, got[4], tiles)
    return ref


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", range(len(KWS)))
def test_grid_ends_replay_matches_oracle(orc, mode, k):
    """tools/align_grid_ends_emu.py on the (13, 11, 16) triple of seed 114 under
    5x7 (3 x 3 tiles of 4 x 6), every parameter set: move for move, end for end,
    and the tiles swept backward are those of the reference path, last first,
    from the end cell's tile."""
    ov, trips, kws = CASES["tiled_k1_3x3"]
    assert kws[k] == KWS[k] and te._tile(ov) == (5, 7) and _geom(11, 16, 5, 7) == (4, 6, 3, 3)
    refs_of(orc, "tiled_k1_3x3", k, mode)                          # the end off the corner, a tied maximum
    _check_replay(orc, *trips[0], KWS[k], mode, (5, 7))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("tile", [(1, 1), (4, 4), (13, 2)])
def test_grid_ends_replay_other_tiles(orc, mode, tile):
    """The same triple with every cell a tile, under square tiles and under
    1 x 8 tiles of a whole column."""
    a, b, c = CASES["tiled_k1_3x3"][1][0]
    for kw in (dict(), dict(score_bits=4)):
        _check_replay(orc, a, b, c, kw, mode, tile)


@pytest.mark.parametrize("mode", MODES)
def test_grid_ends_replay_early_cube(orc, mode):
    """The best cell in tile (0,0) of 3 x 3: one tile is swept backward."""
    a, b, c = _early_cube()
    ref = _check_replay(orc, a, b, c, {}, mode, (5, 7))
    assert _geom(len(b), len(c), 5, 7)[2:] == (3, 3)
    if mode == "any":
        assert ref[3] == (4, 4, 4) and _path_tiles(ref, 4, 6) == [(0, 0)]
    assert _tile_of(ref[3], 4, 6) != (2, 2)


def test_grid_ends_replay_corner_is_the_grid_replay(orc):
    import align_grid_emu
    import align_grid_ends_emu as emu
    a, b, c = CASES["tiled_k1_3x3"][1][0]
    s, st, mv, end, swept = emu.emulate(a, b, c, emu.END_CORNER, tile=(5, 7))
    r = align_grid_emu.emulate(a, b, c, tile=(5, 7))
    assert (s, st, swept) == (r[0], r[1], r[3]) and np.array_equal(mv, r[2]) and end == (13, 11, 16)


# ---- GPU -------------------------------------------------------------------------

def _grid_ends(gpu, trips, mode, params=None, **ov):
    with gpu.overrides(**ov):
        before = gpu.kernel_launch_count()
        got = gpu.align_batch_ends(trips, params, end=mode, grid=True)
        return got, gpu.kernel_launch_count() - before


def _assert_same(gpu, trips, got, refs, params=None, rescore=True, what=None):
    assert len(got) == len(trips) == len(refs)
    for i, (t, g, r) in enumerate(zip(trips, got, refs)):
        assert same(g, r), (what, i, g[0], g[1], g[3], r[0], r[1], r[3])
        check_path(gpu, *t, g, params, rescore=rescore)


@functools.lru_cache(maxsize=None)
def _seams():
    return [ac.related(np.random.default_rng(k), 24, 24, 24) for k in (900, 901, 902)]


# (end cell, end tile, tiles on the path, y seams, z seams, tied) per seed and mode under 8x8
SEAM_FACTS = {
    (900, "face"): ((15, 24, 13), (2, 1), 3, 1, 1, False),
    (900, "any"): ((9, 23, 20), (2, 2), 2, 0, 1, True),
    (901, "face"): ((16, 24, 22), (2, 2), 5, 2, 2, False),
    (901, "any"): ((16, 24, 22), (2, 2), 5, 2, 2, False),
    (902, "face"): ((19, 13, 24), (1, 2), 4, 1, 2, True),
    (902, "any"): ((17, 15, 12), (1, 1), 3, 1, 1, True),
}


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_gpu_grid_ends_seams_from_an_end_tile_that_is_not_the_last(gpu, orc, mode):
    """related 24^3 under 8x8 (3 x 3 tiles): end tiles (2,1), (1,2) and (1,1)
    besides the last, paths over 2 .. 5 tiles through y and z seams. Equal to the
    reference and to the tiled END kernel under the same tile; 5 + 5 launches."""
    trips = _seams()
    out = [ref_end(orc, a, b, c, {}, mode) for a, b, c in trips]
    for seed, (ref, tied) in zip((900, 901, 902), out):
        tiles, ny, nz, ncorner = _geometry(ref, 8, 8)
        assert (ref[3], _tile_of(ref[3], 8, 8), len(tiles), ny, nz, tied) == SEAM_FACTS[seed, mode], (seed, mode)
        assert ncorner == 0
    refs = [r for r, _ in out]
    with gpu.overrides(align_mode="grid", align_tile="8x8"):
        assert gpu.describe_align_plan(1, 24, 24, 24).startswith("grid tile=8x8 tiles=3x3 ")
    got, launches = _grid_ends(gpu, trips, mode, align_tile="8x8")
    assert launches == 5 + 5
    _assert_same(gpu, trips, got, refs, what=mode)
    with gpu.overrides(align_mode="tiled", align_tile="8x8"):
        tiled = gpu.align_batch_ends(trips, end=mode)
    for g, w in zip(got, tiled):
        assert same(g, w)


@pytest.mark.gpu
def test_gpu_grid_ends_corner_write_trap(gpu, orc):
    """Uniform seed 184 (13, 11, 16) under 5x7, face: the end (13, 11, 14) lies in
    the last tile with x1 == la, so backward launch 0 sweeps the corner too. Its
    score and final states must not replace the end's score and record."""
    a, b, c = _uniform(184, 13, 11, 16)
    ref, _ = ref_end(orc, a, b, c, {}, "face")
    tiles, ny, nz, _ = _geometry(ref, 4, 6)
    assert ref[3] == (13, 11, 14) and _tile_of(ref[3], 4, 6) == (2, 2) and (len(tiles), ny, nz) == (5, 2, 2)
    got, launches = _grid_ends(gpu, [(a, b, c)], "face", align_tile="5x7")
    assert launches == 5 + 5
    with gpu.overrides(align_tile="5x7"):
        corner = gpu.align_batch([(a, b, c)], grid=True)[0]
    assert corner[0] == orc.score(a, b, c) != ref[0]
    assert got[0][0] == ref[0] != corner[0] and got[0][3] == ref[3] != (13, 11, 16)
    _assert_same(gpu, [(a, b, c)], got, [ref])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", range(len(KWS)))
def test_gpu_grid_ends_trim_and_early_tiles(gpu, orc, mode, k):
    """Seed 114 (13, 11, 16) under 5x7, every parameter set: ends in the last
    tile below la (launch 0 is trimmed) and in earlier tiles, all tied."""
    trips = CASES["tiled_k1_3x3"][1]
    ref, tied = ref_end(orc, *trips[0], KWS[k], mode)
    assert tied
    want = {(0, "face"): ((5, 11, 14), (2, 2)), (0, "any"): ((4, 9, 12), (2, 1)),
            (5, "face"): ((2, 11, 4), (2, 0)), (5, "any"): ((2, 2, 3), (0, 0))}.get((k, mode))
    if want:
        assert (ref[3], _tile_of(ref[3], 4, 6)) == want
    if (k, mode) == (0, "face"):
        assert len(_geometry(ref, 4, 6)[0]) == 3 and ref[3][0] < 13
    p = gpu.TsaParams.default(**KWS[k])
    got, launches = _grid_ends(gpu, trips, mode, p, align_tile="5x7")
    assert launches == 5 + 5
    _assert_same(gpu, trips, got, [ref], p, rescore=KWS[k].get("score_bits", 12) not in (4, 6), what=(KWS[k], mode))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_gpu_grid_ends_early_cube(gpu, orc, mode):
    """The end in tile (0,0) of 3 x 3: one tile on the path, and the launches
    are queued all the same."""
    a, b, c = _early_cube()
    ref, _ = ref_end(orc, a, b, c, {}, mode)
    if mode == "any":
        assert ref[3] == (4, 4, 4) and _tile_of(ref[3], 4, 6) == (0, 0)
    assert _tile_of(ref[3], 4, 6) != (2, 2)
    got, launches = _grid_ends(gpu, [(a, b, c)], mode, align_tile="5x7")
    assert launches == 5 + 5
    _assert_same(gpu, [(a, b, c)], got, [ref])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_gpu_grid_ends_every_cell_a_tile(gpu, orc, mode):
    """identical (5, 6, 6) under 1x1: 36 tiles, 36 slots, 11 + 11 launches."""
    a, b, c = ac.identical(np.random.default_rng(900), 5, 6, 6)
    ref, _ = ref_end(orc, a, b, c, {}, mode)
    assert _tile_of(ref[3], 1, 1) != (5, 5)
    with gpu.overrides(align_mode="grid", align_tile="1x1"):
        assert gpu.describe_align_plan(1, 5, 6, 6).startswith("grid tile=1x1 tiles=6x6 ")
    got, launches = _grid_ends(gpu, [(a, b, c)], mode, align_tile="1x1")
    assert launches == 11 + 11
    _assert_same(gpu, [(a, b, c)], got, [ref])


def _planted(seed, la, lb, lc, offb, offc):
    """A core s of la symbols: a = s, b = head + s + tail, c = head + s + tail."""
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 4, la).astype(np.uint8)
    out = [s]
    for ln, off in ((lb, offb), (lc, offc)):
        head = rng.integers(0, 4, off).astype(np.uint8)
        tail = rng.integers(0, 4, ln - off - la).astype(np.uint8)
        out.append(np.concatenate([head, s, tail]))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _face_scores(orc, key, kwkey):
    """MAX7 of every face candidate of a triple, as {(x, y, z): score}: the
    prefixes with x == la or y == lb or z == lc alone."""
    a, b, c = (np.frombuffer(s, np.uint8) for s in key)
    la, lb, lc = len(a), len(b), len(c)
    cells = [(x, y, z) for x in range(1, la + 1) for y in range(1, lb + 1) for z in range(1, lc + 1)
             if x == la or y == lb or z == lc]
    parts, offs = [], [0]
    for x, y, z in cells:
        parts += [a[:x], b[:y], c[:z]]
        offs += [offs[-1] + x, offs[-1] + x + y, offs[-1] + x + y + z]
    v = orc.score_batch(np.concatenate(parts), np.asarray(offs, np.int64), orc.default_params(**dict(kwkey)),
                        nthreads=min(8, os.cpu_count() or 1))
    return cells, np.asarray(v, np.int64)


def _ref_big(orc, a, b, c, kw, mode):
    """((score, start, moves, end), tied) where all the prefixes are too many:
    face by brute force over the face candidates, any by oracle.best_range,
    which holds where nothing wraps (asserted)."""
    op = orc.default_params(**kw)
    if mode == "face":
        cells, v = _face_scores(orc, (a.tobytes(), b.tobytes(), c.tobytes()), tuple(sorted(kw.items())))
        best = int(v.max())
        end = cells[int(np.argmax(v))]                             # cells are in (x, y, z) order: the first maximum
        tied = int((v == best).sum()) > 1
    else:
        lo, hi = orc.state_range(a, b, c, op)
        half = 1 << (op.score_bits - 1) if op.score_bits else 1 << 30
        assert -half < lo and hi < half - 1                        # nothing wraps
        br = orc.best_range(a, b, c, op)
        best, end, tied = br.bmax, tuple(br.at_max), None
    s, st, mv = orc.align(a[:end[0]], b[:end[1]], c[:end[2]], op)
    assert s == best
    return (s, st, mv, end), tied


# shape, offb, offc, align_tile, tiles, positions, end, tiles on the path, (y seams, z seams, corners), corner score
PLANTED = {
    "k2": ((12, 70, 60), 29, 27, "35x30", (2, 2), 1050, (12, 41, 39), [(0, 0), (0, 1), (1, 1)], (1, 1, 0), -3),
    "k3_2x1": ((12, 96, 44), 43, 20, "48x44", (2, 1), 2112, (12, 55, 32), [(0, 0), (1, 0)], (1, 0, 0), -3),
    "k3_2x2": ((12, 96, 88), 43, 39, "48x44", (2, 2), 2112, (12, 55, 51), [(0, 0), (1, 1)], (0, 0, 1), 0),
}


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(PLANTED))
def test_gpu_grid_ends_two_and_three_positions_a_thread(gpu, orc, name, mode):
    """A planted core under the default parameters: K = 2 and K = 3, forward and
    backward; the K = 2 end lies in the last tile with x1 == la (the trap again)."""
    shape, offb, offc, tile, grid, pos, end, path, seams, corner = PLANTED[name]
    a, b, c = _planted(7, *shape, offb, offc)
    TY, TZ, nty, ntz = _geom(shape[1], shape[2], *(int(v) for v in tile.split("x")))
    assert (nty, ntz) == grid and TY * TZ == pos and (pos > 1024) and ((pos > 2048) == name.startswith("k3"))
    assert orc.state_range(a, b, c) == (-15, 36)
    ref, _ = _ref_big(orc, a, b, c, {}, mode)
    assert ref[0] == 36 and ref[3] == end and orc.score(a, b, c) == corner
    assert _path_tiles(ref, TY, TZ) == path and _geometry(ref, TY, TZ)[1:] == seams
    if name == "k2":
        assert _tile_of(end, TY, TZ) == (nty - 1, ntz - 1) and end[0] == shape[0]
    got, launches = _grid_ends(gpu, [(a, b, c)], mode, align_tile=tile)
    assert launches == 2 * (nty + ntz - 1)
    _assert_same(gpu, [(a, b, c)], got, [ref], what=(name, mode))


# the first seeds from 7 on whose planted triple, under score_bits = 4, ends off
# the corner with a tied maximum among the face candidates
PLANTED_4BIT_SEED = {"k2": 7, "k3_2x1": 7, "k3_2x2": 7}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PLANTED))
def test_gpu_grid_ends_two_and_three_positions_wrapped(gpu, orc, name):
    """The same shapes under score_bits = 4, where every state wraps: the face
    candidates by brute force (TSA_END_ANY has no reference here short of all
    la*lb*lc prefixes, which is beyond a few seconds: it is not run)."""
    shape, offb, offc, tile = PLANTED[name][:4]
    a, b, c = _planted(PLANTED_4BIT_SEED[name], *shape, offb, offc)
    kw = dict(score_bits=4)
    ref, tied = _ref_big(orc, a, b, c, kw, "face")
    assert ref[3] != shape and tied                                # the conditions of refs_of
    p = gpu.TsaParams.default(**kw)
    got, _ = _grid_ends(gpu, [(a, b, c)], "face", p, align_tile=tile)
    _assert_same(gpu, [(a, b, c)], got, [ref], p, rescore=False, what=name)


def _launches(shapes, budget, tymax, tzmax):
    """Sum over the chunks of [resident] + 2 * max (nty+ntz-1), include/trialign.h's
    rule for tsa_align_batch_grid_ends; also the number of chunks."""
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
        total += int(res) + (2 * max(diag) if diag else 0)
        chunks += 1
    return total, chunks


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_gpu_grid_ends_mixed_batch(gpu, orc, mode):
    """Resident triples between grid triples of 1 x 3, 2 x 1, 3 x 3 and 4 x 4
    tiles, in one chunk and in at least 3: the caller's order, the counted
    launches of the header's rule, and a second call over the first call's
    slots gives the same."""
    trips = ts._ref(orc, "mixed")[0]
    shapes = [tuple(len(s) for s in t) for t in trips]
    refs = [ref_end(orc, a, b, c, {}, mode)[0] for a, b, c in trips]
    with gpu.overrides(align_mode="grid", align_tile="8x8"):
        plans = [gpu.describe_align_plan(len(trips), *s) for s in shapes]
    kinds = [p.split()[0] for p in plans]
    assert kinds.count("resident") == 3 and kinds[0] == "resident" and kinds[1] == "grid"
    grids = {tuple(int(v) for v in re.search(r"tiles=(\d+)x(\d+)", p).groups()) for p in plans if p.startswith("grid")}
    assert any(g[0] == 1 for g in grids) and any(g[1] == 1 for g in grids) and (3, 3) in grids, grids
    got, launches = _grid_ends(gpu, trips, mode, align_tile="8x8")
    assert launches == 1 + 7 + 7 == _launches(shapes, 1 << 40, 8, 8)[0]
    _assert_same(gpu, trips, got, refs, what=mode)
    need = [sum(_grid_need(*s, 8, 8)) if (s[1] > 8 or s[2] > 8) else _cube_bytes(*s) for s in shapes]
    budget = max(need) + min(need)
    want, chunks = _launches(shapes, budget, 8, 8)
    assert chunks >= 3
    first, launches = _grid_ends(gpu, trips, mode, align_tile="8x8", align_tb_bytes=budget)
    second, again = _grid_ends(gpu, trips, mode, align_tile="8x8", align_tb_bytes=budget)
    assert launches == again == want
    _assert_same(gpu, trips, first, refs, what=mode)
    _assert_same(gpu, trips, second, refs, what=mode)


@pytest.mark.gpu
def test_gpu_grid_ends_aligns_what_the_tiled_budget_refuses(gpu, orc):
    """12 x (10, 20, 20) under 8x8 with a budget of 20000 bytes: the tiled END
    kernel needs the cube of 46400 bytes and is TSA_ENOMEM, the grid needs 16256
    and gives the reference in both modes; one byte less is TSA_ENOMEM."""
    trips = ts._ref(orc, "capability")[0]
    need = sum(_grid_need(10, 20, 20, 8, 8))
    assert need == 16256 and _cube_bytes(10, 20, 20) == 46400
    for mode in MODES:
        with gpu.overrides(align_mode="tiled", align_tile="8x8", align_tb_bytes=20000):
            with pytest.raises(gpu.TsaError) as e:
                gpu.align_batch_ends(trips, end=mode)
            assert e.value.rc == gpu.TSA_ENOMEM
        refs = [ref_end(orc, a, b, c, {}, mode)[0] for a, b, c in trips]
        for budget in (20000, need):
            got, launches = _grid_ends(gpu, trips, mode, align_tile="8x8", align_tb_bytes=budget)
            assert launches == 12 * (5 + 5)                        # a chunk per triple
            _assert_same(gpu, trips, got, refs, what=(mode, budget))
        with gpu.overrides(align_tile="8x8", align_tb_bytes=need - 1):
            with pytest.raises(gpu.TsaError) as e:
                gpu.align_batch_ends(trips, end=mode, grid=True)
            assert e.value.rc == gpu.TSA_ENOMEM


@pytest.mark.gpu
def test_gpu_grid_ends_corner_is_align_batch_grid(gpu):
    """TSA_END_CORNER: align_batch(grid=True) output for output, ends = the
    lengths, the corner grid's launch count; also under align_mode = plane."""
    trips = _seams() + [_uniform(51, 4, 70, 9), _uniform(52, 6, 5, 7)]
    for ov, launches in ((dict(align_tile="8x8"), None), (dict(align_tile="8x8", align_mode="plane"), 0)):
        with gpu.overrides(**ov):
            before = gpu.kernel_launch_count()
            want = gpu.align_batch(trips, grid=True)
            mid = gpu.kernel_launch_count()
            got = gpu.align_batch_ends(trips, end="corner", grid=True)
            after = gpu.kernel_launch_count()
        assert after - mid == mid - before and (launches is None or after - mid == launches)
        if launches is None:
            assert after - mid == 1 + (9 + 2 - 2) + (9 + 2 - 1)     # resident; (4, 70, 9) has 9 x 2 tiles
        for t, g, w in zip(trips, got, want):
            assert g[0] == w[0] and g[1] == w[1] and np.array_equal(g[2], w[2]), ov
            assert g[3] == tuple(len(s) for s in t)


@pytest.mark.gpu
def test_gpu_grid_ends_unstaged_a(gpu, orc):
    """(163900, 3, 4) under 2x2: A is read from global memory, forward with the
    fold and backward, next to triples that stage it. TSA_END_ANY alone: its
    reference is oracle.best_range; the 163900 * 6 + 12 face candidates, each a
    cube of up to 2 million cells, are beyond a few seconds of brute force."""
    trips = tp._unstaged_cases()
    shapes = [tuple(len(s) for s in t) for t in trips]
    assert shapes[2] == (163900, 3, 4)
    assert 32 * 3 * 3 + 2 + 2 + 163900 > tp.LDS_MAX                # align_stage_a declines for a 2x2 tile
    with gpu.overrides(align_mode="grid", align_tile="2x2"):
        assert gpu.describe_align_plan(4, 163900, 3, 4).startswith("grid tile=2x2 tiles=2x2 ")
    refs = [_ref_big(orc, a, b, c, {}, "any")[0] for a, b, c in trips]
    assert refs[2][3] == (47, 2, 4) and refs[2][0] == 6            # the last tile, trimmed far below la
    got, _ = _grid_ends(gpu, trips, "any", align_tile="2x2")
    _assert_same(gpu, trips, got, refs)
