"""The tiled resident traceback kernel (csrc/align_tiled_kernel.hip) and its
dispatch: under align_mode=tiled a triple whose (y,z) plane does not fit one
workgroup is swept tile by tile by one workgroup, the tiles chained through
face buffers, and must come out as the oracle's independent traceback gives it
-- score, start and moves. tsa_describe_align_plan names the path on any host;
the tiled schedule itself is replayed on the CPU by tools/align_tiled_emu.py.

Balanced tiles (align_tile_geom) cut (8,130,130) into 3 x 3 tiles of 44 x 44
whose edge tiles are 42 wide, not 64 + 64 + 2; narrow edge tiles are what the
tiny-cube cases under align_tile have (lengths 1..40 under 5x7 and 3x16)."""
import ctypes
import functools
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

# the parameter sets of test_align_batch.KWS
KWS = [dict(), dict(s3_mode=1), dict(score_bits=0), dict(score_bits=6),
       dict(match=3, mismatch=-1, gap_open=2, gap_extend=2, score_bits=16)]

# The default rule DESIGN.md 4.7 records: without an override a chunk's
# over-capacity triples are tiled when there are at least this many of them,
# and take the plane sweep otherwise (profiles/align_tiled.jsonl).
DEFAULT_TILED_MIN_GROUP = 256


def _rand_triple(rng, la, lb, lc, hi=5):
    return tuple(rng.integers(0, hi, n).astype(np.uint8) for n in (la, lb, lc))


def _same(got, ref):
    return got[0] == ref[0] and tuple(got[1]) == tuple(ref[1]) and np.array_equal(got[2], ref[2])


def _cube_bytes(la, lb, lc):
    return 4 * lb * (la + lc - 1) * lc


def _plan_rc(tsa, n, la, lb, lc):
    buf = ctypes.create_string_buffer(256)
    rc = tsa.lib().tsa_describe_align_plan(n, la, lb, lc, ctypes.byref(tsa.TsaParams.default()), buf, len(buf))
    return rc, buf.value.decode()


# ---- CPU ---------------------------------------------------------------------

def test_describe_align_plan_is_exported_and_host_only(tsa):
    assert "tsa_describe_align_plan" in tsa.EXPORTS
    assert hasattr(tsa.lib(), "tsa_describe_align_plan") and callable(tsa.describe_align_plan)
    assert tsa.describe_align_plan(1, 64, 64, 64).startswith("resident")
    with tsa.overrides(align_mode="tiled"):
        assert tsa.describe_align_plan(1, 64, 64, 64).startswith("resident")
        txt = tsa.describe_align_plan(1, 8, 64, 72)
        assert txt.startswith("tiled ") and " tiles=1x2 " in txt and " tile=64x36 " in txt, txt
        assert re.search(r" lds=\d+ faces=\d+$", txt), txt
    with tsa.overrides(align_mode="tiled", align_tile="4x4"):
        txt = tsa.describe_align_plan(1, 8, 13, 13)
        assert txt.startswith("tiled ") and " tiles=4x4 " in txt and " tile=4x4 " in txt, txt
        assert tsa.describe_align_plan(1, 8, 4, 4).startswith("resident")     # within the tile
        assert tsa.describe_align_plan(1, 8, 4, 5).startswith("tiled ")       # fits a workgroup, exceeds the tile
    with tsa.overrides(align_mode="plane"):
        for shape in ((1, 1, 1), (64, 64, 64), (8, 64, 72), (256, 256, 256)):
            assert tsa.describe_align_plan(512, *shape) == "plane"
    with tsa.overrides(align_mode="resident"):
        assert tsa.describe_align_plan(512, 8, 64, 72) == "plane"
        assert tsa.describe_align_plan(512, 8, 64, 64).startswith("resident")
    p = tsa.TsaParams.default()
    buf = ctypes.create_string_buffer(64)
    L = tsa.lib()
    assert L.tsa_describe_align_plan(0, 8, 8, 8, ctypes.byref(p), buf, 64) == tsa.TSA_EINVAL
    assert L.tsa_describe_align_plan(1, 8, 0, 8, ctypes.byref(p), buf, 64) == tsa.TSA_EINVAL
    assert L.tsa_describe_align_plan(1, 8, 8, 8, ctypes.byref(p), None, 64) == tsa.TSA_EINVAL
    assert L.tsa_describe_align_plan(1, 8, 8, 8, ctypes.byref(p), buf, 0) == tsa.TSA_EINVAL


def test_describe_align_plan_default_rule(tsa):
    """No override: a fitting triple is resident; an over-capacity group is
    tiled from DEFAULT_TILED_MIN_GROUP triples on and takes
    the plane sweep below that."""
    assert tsa.get_overrides() == {}
    for n in (1, 8, 64, 255, 256, 512, 65535):
        assert tsa.describe_align_plan(n, 64, 64, 64).startswith("resident")
        for shape in ((8, 64, 72), (128, 128, 128), (256, 256, 256)):
            want = "tiled" if n >= DEFAULT_TILED_MIN_GROUP else "plane"
            assert tsa.describe_align_plan(n, *shape).split()[0] == want, (n, shape)


def test_align_tile_override(tsa):
    assert "align_tile" in tsa.OVERRIDES
    L = tsa.lib()
    assert L.tsa_set_override(b"align_tile", b"5x7") == tsa.TSA_OK
    assert tsa.get_overrides() == {"align_tile": "5x7"}
    assert _plan_rc(tsa, 1, 8, 13, 13)[0] == tsa.TSA_OK
    with tsa.overrides(align_mode="tiled"):
        rc, txt = _plan_rc(tsa, 1, 8, 13, 13)
        assert rc == tsa.TSA_OK and " tile=5x7 tiles=3x2 " in txt, txt
    # malformed, an edge below 1, over the capacity (64 x 72 is over the resident one, 64 x 49 over 3072
    # positions, 1 x 3072 over the LDS)
    for bad in ("", "5", "5x", "x7", "5x7x2", "5*7", " 5x7", "5x7 ", "-5x7", "5x-7", "0x7", "5x0", "a", "5;7",
                "64x72", "72x64", "64x49", "4097x1", "1x4097", "1x3072", "99999999999x1"):
        with tsa.overrides(align_tile=bad):
            assert _plan_rc(tsa, 1, 8, 13, 13)[0] == tsa.TSA_EINVAL, bad
    for good in ("1x1", "64x48", "48x64", "1x2500", "2500x1", "13x2"):
        with tsa.overrides(align_tile=good, align_mode="tiled"):
            assert _plan_rc(tsa, 1, 8, 100, 100)[0] == tsa.TSA_OK, good
    with tsa.overrides(align_mode="tilted"):
        assert _plan_rc(tsa, 1, 8, 13, 13)[0] == tsa.TSA_EINVAL


def _emu_align(a, b, c, op, tile):
    import align_tiled_emu
    return align_tiled_emu.align(a, b, c, op.match, op.mismatch, op.gap_open, op.gap_extend, bool(op.s3_mode),
                                 op.score_bits, tile)


EMU_TILES = [(4, 4), (5, 7), (1, 1), (13, 2)]


@pytest.mark.parametrize("kw", KWS)
def test_tiled_schedule_emulated_matches_oracle(orc, kw):
    """tools/align_tiled_emu.py -- per-tile zeroed buffers, face positions that
    publish from poisoned, parity double-buffered face arrays, last-row and
    last-column stores, the history reset -- against the oracle, move for
    move. 13 under 4x4 is four tiles an axis: both parities of both faces are
    reused."""
    rng = np.random.default_rng(11 + len(kw) + kw.get("score_bits", 1))
    op = orc.default_params(**kw)
    shapes = [tuple(int(v) for v in rng.integers(1, 14, 3)) for _ in range(4)]
    for la, lb, lc in shapes + [(13, 13, 13), (5, 12, 11), (1, 9, 9), (9, 1, 9), (9, 9, 1), (1, 1, 1)]:
        a, b, c = _rand_triple(rng, la, lb, lc)
        ref = orc.align(a, b, c, op)
        for tile in EMU_TILES:
            assert _same(_emu_align(a, b, c, op, tile), ref), (kw, la, lb, lc, tile)


def test_tiled_schedule_emulated_all_a(orc):
    for n in (1, 2, 7):
        z = np.zeros(n, np.uint8)
        for tile in EMU_TILES:
            s, st, mv = _emu_align(z, z, z, orc.default_params(), tile)
            assert s == 3 * n and st == (0, 0, 0) and list(mv) == [0] * n, (n, tile)


@pytest.mark.parametrize("kw", [dict(), dict(match=3, mismatch=-1, go=2, ge=2, sop=True, bits=6)])
def test_tiled_emu_of_one_tile_is_the_resident_emu(kw):
    """Both replays run the one step of tools/align_emu.py. With a tile cap of
    at least (lb, lc) the tiled schedule is one tile with no face -- steps from
    q = 1 -- and must give the resident schedule's (q from 2) score, final
    states and pointer word of every cell."""
    import align_emu
    import align_tiled_emu
    rng = np.random.default_rng(21)
    for (la, lb, lc), tile in (((1, 1, 1), (1, 1)), ((7, 1, 5), (1, 5)), ((6, 9, 4), (64, 48))):
        a, b, c = _rand_triple(rng, la, lb, lc)
        res = align_emu.emulate(a, b, c, **kw)
        til = align_tiled_emu.emulate(a, b, c, tile=tile, **kw)
        assert align_tiled_emu.tile_geom(lb, lc, *tile)[2:] == (1, 1)
        assert len(res[2]) == la * lb * lc
        assert til == res, (kw, la, lb, lc)


def test_tiled_emu_geometry_is_the_library_s(tsa):
    """The replay's tile grid is the one tsa_describe_align_plan reports."""
    import align_tiled_emu
    for lb, lc, tile in ((13, 13, (4, 4)), (40, 1, (5, 7)), (130, 130, (64, 48)), (1, 4097, (64, 48)), (9, 33, (3, 16))):
        TY, TZ, nty, ntz = align_tiled_emu.tile_geom(lb, lc, *tile)
        with tsa.overrides(align_mode="tiled", align_tile="%dx%d" % tile):
            txt = tsa.describe_align_plan(1, 8, lb, lc)
        assert " tile=%dx%d tiles=%dx%d " % (TY, TZ, nty, ntz) in txt, (lb, lc, tile, txt)


# ---- GPU ---------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _tiny(orc, ki):
    """24 random triples with lengths 1..40 and their oracle alignments, once per parameter set."""
    kw = KWS[ki]
    rng = np.random.default_rng(700 + len(kw) + kw.get("score_bits", 1))
    trips = [_rand_triple(rng, *(int(v) for v in rng.integers(1, 41, 3))) for _ in range(24)]
    return trips, [orc.align(a, b, c, orc.default_params(**kw)) for a, b, c in trips]


@pytest.mark.gpu
@pytest.mark.parametrize("tile", ["5x7", "3x16"])
@pytest.mark.parametrize("ki", range(len(KWS)))
def test_gpu_align_tiled_tiny_cubes_many_tiles(gpu, orc, ki, tile):
    """Up to 8 x 6 (14 x 3) tiles per cube, edge tiles of every width, wrapped
    candidates and equal argmaxes under score_bits=6."""
    trips, ref = _tiny(orc, ki)
    p = gpu.TsaParams.default(**KWS[ki])
    with gpu.overrides(align_mode="tiled", align_tile=tile):
        got = gpu.align_batch(trips, p)
    with gpu.overrides(align_mode="plane"):
        pla = gpu.align_batch(trips, p)
    assert len(got) == 24
    for i, t in enumerate(trips):
        shape = tuple(len(s) for s in t)
        assert _same(got[i], ref[i]), (i, shape)
        assert _same(got[i], pla[i]), (i, shape)


CROSS = [(8, 64, 72), (8, 72, 64), (8, 65, 65), (8, 64, 64), (8, 130, 130), (8, 1, 4097), (1, 1, 1), (8, 4097, 1),
         (150, 70, 5), (40, 129, 129)]


@pytest.mark.gpu
def test_gpu_align_tiled_real_tile_sizes(gpu, orc):
    """One batch under the default tile, caller order kept: the smallest shapes
    that cross it (1 x 2, 2 x 2 and 3 x 3 grids, a single row of 86 tiles, a
    single column of 65, LA beyond lb + lc), mixed with triples that stay
    resident. The sequences are independent random ones, so the optimal paths
    are short and stay in one tile -- only (40,129,129) crosses a y and a z
    seam; paths across seams and tile corners are test_align_paths.py's."""
    rng = np.random.default_rng(43)
    trips = [_rand_triple(rng, *s) for s in CROSS]
    with gpu.overrides(align_mode="tiled"):
        plans = [gpu.describe_align_plan(len(CROSS), *s).split()[0] for s in CROSS]
        got = gpu.align_batch(trips)
    assert plans.count("tiled") == 7 and plans.count("resident") == 3, plans
    for (a, b, c), g, shape in zip(trips, got, CROSS):
        assert _same(g, orc.align(a, b, c)), shape


@pytest.mark.gpu
def test_gpu_align_tiled_launch_accounting(gpu, orc):
    """One launch per chunk for the tiled group, one more when the chunk also
    holds fitting triples; the plane sweep is not counted."""
    rng = np.random.default_rng(44)
    over = [_rand_triple(rng, 8, 64, 72) for _ in range(3)]
    fit = [_rand_triple(rng, 8, 16, 16) for _ in range(3)]
    mixed = [t for pair in zip(over, fit) for t in pair]
    ref = [orc.align(a, b, c) for a, b, c in mixed]

    def launches(trips, want, **ov):
        with gpu.overrides(**ov):
            before = gpu.kernel_launch_count()
            got = gpu.align_batch(trips)
            return gpu.kernel_launch_count() - before, all(_same(g, r) for g, r in zip(got, want))

    assert launches(over, ref[0::2], align_mode="tiled") == (1, True)
    assert launches(mixed, ref, align_mode="tiled") == (2, True)
    budget = _cube_bytes(8, 64, 72) + _cube_bytes(8, 16, 16)       # chunks of one over-capacity and one fitting triple
    assert launches(mixed, ref, align_mode="tiled", align_tb_bytes=budget) == (6, True)
    assert launches(over, ref[0::2], align_mode="tiled", align_tb_bytes=_cube_bytes(8, 64, 72)) == (3, True)
    assert launches(mixed, ref, align_mode="plane") == (0, True)


@pytest.mark.gpu
def test_gpu_align_tiled_face_workspace_reuse(gpu, orc, synth):
    """12 triples of (10,20,20) in 3 x 3 tiles under a budget of 5 cubes: the
    face workspace serves several triples and three chunks, and a second call
    gives the same -- no state is carried between calls."""
    trips = [synth.triple(800 + i, 10, 20, 20) for i in range(12)]
    ref = [orc.align(a, b, c) for a, b, c in trips]
    with gpu.overrides(align_mode="tiled", align_tile="8x8", align_tb_bytes=5 * _cube_bytes(10, 20, 20)):
        assert " tiles=3x3 " in gpu.describe_align_plan(12, 10, 20, 20)
        before = gpu.kernel_launch_count()
        first = gpu.align_batch(trips)
        assert gpu.kernel_launch_count() - before == 3
        second = gpu.align_batch(trips)
    for i in range(12):
        assert _same(first[i], ref[i]), i
        assert _same(second[i], ref[i]), i


@pytest.mark.gpu
def test_gpu_align_mode_resident_keeps_its_route(gpu, orc):
    """align_mode=resident still sends (8,64,72) to the plane sweep: the
    result is the oracle's and no counted launch is made for it."""
    rng = np.random.default_rng(45)
    a, b, c = _rand_triple(rng, 8, 64, 72)
    with gpu.overrides(align_mode="resident"):
        assert gpu.describe_align_plan(1, 8, 64, 72) == "plane"
        before = gpu.kernel_launch_count()
        got = gpu.align_batch([(a, b, c)])
        assert gpu.kernel_launch_count() - before == 0
    assert _same(got[0], orc.align(a, b, c))
    assert _same(got[0], gpu.align(a, b, c))


@pytest.mark.gpu
def test_gpu_align_default_rule(gpu, orc):
    """No override: DEFAULT_TILED_MIN_GROUP over-capacity triples in a chunk
    take the tiled kernel (one counted launch), one fewer the plane sweep
    (none); either way every triple equals the oracle."""
    rng = np.random.default_rng(46)
    trips = [_rand_triple(rng, 1, 65, 65) for _ in range(DEFAULT_TILED_MIN_GROUP)]
    ref = [orc.align(a, b, c) for a, b, c in trips]
    assert gpu.get_overrides() == {}
    for n, want in ((DEFAULT_TILED_MIN_GROUP, 1), (DEFAULT_TILED_MIN_GROUP - 1, 0)):
        before = gpu.kernel_launch_count()
        got = gpu.align_batch(trips[:n])
        assert gpu.kernel_launch_count() - before == want, n
        assert all(_same(g, r) for g, r in zip(got, ref)), n
