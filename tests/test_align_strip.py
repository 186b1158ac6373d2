"""The strip path of batched traceback (csrc/align_strip_kernel.hip,
tb_walk_strip, align_mode=strip, tsa_align_batch_lowmem): a triple whose (y,z)
plane does not fit one workgroup keeps the pointers of one tile row -- a strip
-- at a time. A forward launch keeps the last row of every strip but the last,
then the strips are swept again last to first, each followed by a segment walk,
and the strips above a path's end are skipped. Everything must come out as the
oracle's independent traceback gives it: score, start and moves.

The plan text, the argument checks and the schedule's CPU replay
(tools/align_strip_emu.py) need no device."""
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

# the parameter sets of test_align_tiled.KWS, and score_bits=9
KWS = [dict(), dict(s3_mode=1), dict(score_bits=0), dict(score_bits=6),
       dict(match=3, mismatch=-1, gap_open=2, gap_extend=2, score_bits=16), dict(score_bits=9)]
SEEDS = (900, 901, 902, 903)


def _rand_triple(rng, la, lb, lc, hi=4):
    return tuple(rng.integers(0, hi, n).astype(np.uint8) for n in (la, lb, lc))


def _same(got, ref):
    return got[0] == ref[0] and tuple(got[1]) == tuple(ref[1]) and np.array_equal(got[2], ref[2])


def _cube_bytes(la, lb, lc):
    return 4 * lb * (la + lc - 1) * lc


def _geom(lb, lc, tymax, tzmax):
    nty, ntz = -(-lb // tymax), -(-lc // tzmax)
    return -(-lb // nty), -(-lc // ntz), nty, ntz


def _strip_need(la, lb, lc, tymax, tzmax):
    """(strip cube bytes, face bytes) of include/trialign.h's need formula."""
    TY, _, nty, _ = _geom(lb, lc, tymax, tzmax)
    return 4 * TY * (la + lc - 1) * lc, 16 * ((nty - 1) * la * (lc + 1) + 2 * la * TY)


def _strips(ref, TY):
    """The strips the cells of a reference alignment lie in."""
    return {(y - 1) // TY for _, y, _ in ac.path_cells(ref[1], ref[2])}


def _plan_rc(tsa, n, la, lb, lc):
    buf = ctypes.create_string_buffer(256)
    rc = tsa.lib().tsa_describe_align_plan(n, la, lb, lc, ctypes.byref(tsa.TsaParams.default()), buf, len(buf))
    return rc, buf.value.decode()


# ---- CPU ---------------------------------------------------------------------

def test_strip_plan_text(tsa):
    with tsa.overrides(align_mode="strip", align_tile="8x8"):
        txt = tsa.describe_align_plan(1, 10, 20, 20)
        assert txt.startswith("strip tile=7x7 tiles=3x3 "), txt
        m = re.search(r" lds=(\d+) cube=(\d+) faces=(\d+)$", txt)
        assert m, txt
        assert int(m.group(2)) == 4 * 7 * 29 * 20
        assert int(m.group(3)) == 16 * (2 * 10 * 21 + 2 * 10 * 7)
        assert (int(m.group(2)), int(m.group(3))) == _strip_need(10, 20, 20, 8, 8)
    with tsa.overrides(align_mode="strip", align_tile="4x4"):
        assert tsa.describe_align_plan(1, 8, 4, 4).startswith("resident")     # a fitting triple
        assert tsa.describe_align_plan(1, 8, 4, 5).startswith("strip tile=4x3 tiles=1x2 ")
    with tsa.overrides(align_mode="strip"):                                     # the default tile, any group size
        assert tsa.describe_align_plan(1, 64, 64, 64).startswith("resident")
        for n in (1, 256):
            assert tsa.describe_align_plan(n, 256, 256, 256).startswith("strip tile=64x43 tiles=4x6 ")
    # without the override nothing strips
    for n in (1, 256):
        assert not tsa.describe_align_plan(n, 256, 256, 256).startswith("strip")


def test_strip_unknown_mode_is_einval(tsa):
    with tsa.overrides(align_mode="strips"):
        assert _plan_rc(tsa, 1, 8, 13, 13)[0] == tsa.TSA_EINVAL
    with tsa.overrides(align_mode="strip"):
        assert _plan_rc(tsa, 1, 8, 13, 13)[0] == tsa.TSA_OK


def test_align_batch_lowmem_is_exported(tsa):
    assert "tsa_align_batch_lowmem" in tsa.EXPORTS
    assert hasattr(tsa.lib(), "tsa_align_batch_lowmem")
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "trialign.h")) as f:
        assert re.search(r"\bint tsa_align_batch_lowmem\(", f.read())


def _raw_call(tsa, fn, seqs, offsets, n, p, null=None):
    """fn (a C entry point's name) with fresh output buffers; the output named by `null` is passed as NULL."""
    u8, i32, i64 = (ctypes.POINTER(t) for t in (ctypes.c_uint8, ctypes.c_int32, ctypes.c_int64))
    seqs = np.ascontiguousarray(seqs, np.uint8)
    offsets = np.ascontiguousarray(offsets, np.int64)
    m = max(abs(n), 1)
    out = dict(scores=np.zeros(m, np.int32), moves=np.zeros(max(len(seqs), 1), np.uint8),
               n_moves=np.zeros(m, np.int32), starts=np.zeros(3 * m, np.int32))
    arg = lambda k, t: None if k == null else out[k].ctypes.data_as(t)
    return getattr(tsa.lib(), fn)(None if null == "seqs" else seqs.ctypes.data_as(u8),
                                  None if null == "offsets" else offsets.ctypes.data_as(i64), n, ctypes.byref(p),
                                  arg("scores", i32), arg("moves", u8), arg("n_moves", i32), arg("starts", i32), 0)


def test_align_batch_lowmem_validates_as_align_batch(tsa):
    """Validation comes before any device work: the same codes as tsa_align_batch's on any host."""
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
        rc = _raw_call(tsa, "tsa_align_batch_lowmem", *args)
        assert rc == tsa.TSA_EINVAL, args[2:]
        assert rc == _raw_call(tsa, "tsa_align_batch", *args), args[2:]
    assert _raw_call(tsa, "tsa_align_batch_lowmem", np.zeros(1, np.uint8), np.zeros(1, np.int64), 0, p) == tsa.TSA_OK
    assert tsa.align_batch([], lowmem=True) == []
    with pytest.raises(tsa.TsaError) as e:
        tsa.align_batch([([0, 7], [1], [2])], lowmem=True)
    assert e.value.rc == tsa.TSA_EINVAL


def _emu(a, b, c, op, tile):
    import align_strip_emu
    return align_strip_emu.emulate(a, b, c, op.match, op.mismatch, op.gap_open, op.gap_extend, bool(op.s3_mode),
                                   op.score_bits, tile)


EMU_TILES = [(4, 4), (5, 7), (1, 1), (13, 2)]


@pytest.mark.parametrize("kw", KWS)
def test_strip_schedule_emulated_matches_oracle(orc, kw):
    """tools/align_strip_emu.py -- the forward pass into poisoned kept faces,
    the strips last to first into a strip cube cleared before every sweep, the
    segment walks, the early end -- against the oracle, move for move. Random
    symbols give short paths (early ends), identical sequences paths through
    every strip."""
    rng = np.random.default_rng(31 + len(kw) + kw.get("score_bits", 1))
    op = orc.default_params(**kw)
    shapes = [tuple(int(v) for v in rng.integers(1, 15, 3)) for _ in range(3)]
    trips = [_rand_triple(rng, *s, hi=5) for s in shapes + [(13, 13, 13), (1, 9, 9), (9, 1, 9), (9, 9, 1), (1, 1, 1)]]
    trips += [ac.identical(rng, 14, 14, 14), ac.identical(rng, 6, 13, 9, shift=2)]
    for a, b, c in trips:
        ref = orc.align(a, b, c, op)
        for tile in EMU_TILES:
            assert _same(_emu(a, b, c, op, tile), ref), (kw, len(a), len(b), len(c), tile)


def test_strip_emu_sweeps_only_down_to_the_path_s_end(orc):
    """A path through every strip has every strip swept, last first; one that
    ends in the last strip leaves the others unswept -- as many strips as the
    reference path visits, in both cases."""
    import align_strip_emu
    op = orc.default_params()
    rng = np.random.default_rng(32)
    a, b, c = ac.identical(rng, 14, 14, 14)
    assert _emu(a, b, c, op, (4, 4))[3] == [3, 2, 1, 0]
    assert align_strip_emu.align(a, b, c, tile=(4, 4))[0] == 3 * 14
    seen = set()
    for _ in range(6):
        a, b, c = _rand_triple(rng, 3, 14, 14)
        ref = orc.align(a, b, c, op)
        got = _emu(a, b, c, op, (4, 4))
        assert _same(got, ref)
        want = sorted(_strips(ref, 4), reverse=True)
        assert got[3] == list(range(3, want[-1] - 1, -1)) and want == got[3], (want, got[3])
        seen.add(len(got[3]))
    assert min(seen) == 1                                          # some path ended in the last strip


def test_strip_emu_geometry_is_the_library_s(tsa):
    import align_tiled_emu
    for lb, lc, tile in ((13, 13, (4, 4)), (40, 1, (5, 7)), (130, 50, (64, 48)), (129, 96, (64, 48)), (6, 6, (1, 1))):
        geom = align_tiled_emu.tile_geom(lb, lc, *tile)
        assert geom == _geom(lb, lc, *tile)
        with tsa.overrides(align_mode="strip", align_tile="%dx%d" % tile):
            txt = tsa.describe_align_plan(1, 8, lb, lc)
        assert txt.startswith("strip tile=%dx%d tiles=%dx%d " % geom), (lb, lc, tile, txt)


# ---- GPU ---------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _ref(orc, key, kwi=0):
    """The triples of a named case and their oracle alignments, computed once."""
    trips = []
    if key == "seams":                                             # tile 8x8: 3 strips of 7
        for k in SEEDS:
            trips.append(ac.identical(np.random.default_rng(k), 20, 20, 20))
        trips.append(ac.related(np.random.default_rng(900), 24, 24, 24))
    elif key == "rows":                                            # tile 1x1: every row a strip
        trips.append(ac.identical(np.random.default_rng(900), 5, 6, 6))
        trips.append(_rand_triple(np.random.default_rng(901), 5, 6, 6))
    elif key == "early":                                           # tile 8x8: 5 strips, the path in the last
        for k in SEEDS:
            trips.append(_rand_triple(np.random.default_rng(k), 3, 40, 40))
        trips.insert(2, ac.identical(np.random.default_rng(900), 20, 20, 20))
    elif key in ("k2", "k3"):                                      # default tile: 44x25 / 43x48 positions
        shape = (130, 130, 50) if key == "k2" else (129, 129, 96)
        for k in SEEDS:
            trips.append(ac.identical(np.random.default_rng(k), *shape))
        trips.append(ac.related(np.random.default_rng(900), *shape))
    elif key == "mixed":                                           # tile 8x8: resident, 1, 2 and 4 strips, lb != lc
        rng = np.random.default_rng(900)
        for shape in ((6, 8, 8), (9, 30, 12), (5, 8, 20), (12, 16, 9), (7, 5, 3), (10, 20, 20), (4, 27, 31),
                      (6, 3, 8), (11, 9, 8)):
            trips.append(ac.related(rng, *shape) if shape[1] > 8 else _rand_triple(rng, *shape))
    elif key == "capability":
        import tsa_amd.synth as synth
        trips = [synth.triple(800 + i, 10, 20, 20) for i in range(12)]
    op = orc.default_params(**KWS[kwi])
    return trips, [orc.align(a, b, c, op) for a, b, c in trips]


def _check_all_modes(gpu, trips, ref, params=None, **ov):
    """strip, tiled and plane under the same overrides: all equal to the oracle, so to each other."""
    for mode in ("strip", "tiled", "plane"):
        with gpu.overrides(align_mode=mode, **ov):
            got = gpu.align_batch(trips, params)
        assert len(got) == len(trips)
        for i, (g, r) in enumerate(zip(got, ref)):
            assert _same(g, r), (mode, i, tuple(len(s) for s in trips[i]))


@pytest.mark.gpu
def test_gpu_strip_every_seam(gpu, orc):
    """Paths that visit strips 0, 1 and 2 of 3 (tile 8x8: strips of 7 rows): every walk segment hands over."""
    trips, ref = _ref(orc, "seams")
    with gpu.overrides(align_mode="strip", align_tile="8x8"):
        assert gpu.describe_align_plan(1, 20, 20, 20).startswith("strip tile=7x7 tiles=3x3 ")
    for i in range(len(SEEDS)):
        assert _strips(ref[i], 7) == {0, 1, 2}, i
    _check_all_modes(gpu, trips, ref, align_tile="8x8")


@pytest.mark.gpu
def test_gpu_strip_every_row_a_strip(gpu, orc):
    trips, ref = _ref(orc, "rows")
    with gpu.overrides(align_mode="strip", align_tile="1x1"):
        assert gpu.describe_align_plan(1, 5, 6, 6).startswith("strip tile=1x1 tiles=6x6 ")
    assert _strips(ref[0], 1) == set(range(6))
    _check_all_modes(gpu, trips, ref, align_tile="1x1")


@pytest.mark.gpu
def test_gpu_strip_early_end(gpu, orc):
    """Paths inside the last of 5 strips: the four strips above are skipped, while a triple whose path crosses
    all of its strips is live in the same launches."""
    trips, ref = _ref(orc, "early")
    with gpu.overrides(align_mode="strip", align_tile="8x8"):
        assert gpu.describe_align_plan(1, 3, 40, 40).startswith("strip tile=8x8 tiles=5x5 ")
    for i in (0, 1, 3, 4):
        assert _strips(ref[i], 8) == {4}, i
    assert _strips(ref[2], 7) == {0, 1, 2}
    _check_all_modes(gpu, trips, ref, align_tile="8x8")


@pytest.mark.gpu
@pytest.mark.parametrize("key,shape,tile,tiles", [("k2", (130, 130, 50), "44x25", "3x2"),
                                                  ("k3", (129, 129, 96), "43x48", "3x2")])
def test_gpu_strip_two_and_three_positions_a_thread(gpu, orc, key, shape, tile, tiles):
    """The default tile: 1100 positions (K = 2) and 2064 (K = 3), paths through all 3 strips."""
    trips, ref = _ref(orc, key)
    with gpu.overrides(align_mode="strip"):
        assert gpu.describe_align_plan(1, *shape).startswith("strip tile=%s tiles=%s " % (tile, tiles))
    TY = int(tile.split("x")[0])
    for i in range(len(SEEDS)):
        assert _strips(ref[i], TY) == {0, 1, 2}, i
    _check_all_modes(gpu, trips, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("kwi", [3, 5, 1])
def test_gpu_strip_arithmetic(gpu, orc, kwi):
    """score_bits 6 and 9 (wrapped candidates, equal argmaxes) and TSA_S3_SOP on the 3-strip shapes."""
    trips, ref = _ref(orc, "seams", kwi)
    _check_all_modes(gpu, trips, ref, gpu.TsaParams.default(**KWS[kwi]), align_tile="8x8")


def _expected_launches(shapes, budget, tymax, tzmax):
    """[resident] + [forward] + S summed over the chunks of include/trialign.h's rule."""
    total, i = 0, 0
    while i < len(shapes):
        used, res, nty = 0, False, []
        while i < len(shapes):
            la, lb, lc = shapes[i]
            over = lb > tymax or lc > tzmax
            need = sum(_strip_need(la, lb, lc, tymax, tzmax)) if over else _cube_bytes(la, lb, lc)
            assert need <= budget
            if used + need > budget:
                break
            used += need
            if over:
                nty.append(_geom(lb, lc, tymax, tzmax)[2])
            else:
                res = True
            i += 1
        total += int(res) + (int(max(nty) >= 2) + max(nty) if nty else 0)
    return total


@pytest.mark.gpu
def test_gpu_strip_mixed_batch(gpu, orc):
    """Resident triples and strip triples of 1, 2 and 4 strips in one call, in the caller's order; the counted
    launches are [resident] + [forward] + S; under a cut budget the batch takes several chunks."""
    trips, ref = _ref(orc, "mixed")
    shapes = [tuple(len(s) for s in t) for t in trips]
    with gpu.overrides(align_mode="strip", align_tile="8x8"):
        plans = [gpu.describe_align_plan(len(trips), *s) for s in shapes]
        assert [p.split()[0] for p in plans].count("resident") == 3
        assert {int(re.search(r"tiles=(\d+)x", p).group(1)) for p in plans if p.startswith("strip")} == {1, 2, 3, 4}
        before = gpu.kernel_launch_count()
        got = gpu.align_batch(trips)
        assert gpu.kernel_launch_count() - before == 1 + 1 + 4
    assert all(_same(g, r) for g, r in zip(got, ref))
    need = [sum(_strip_need(*s, 8, 8)) if (s[1] > 8 or s[2] > 8) else _cube_bytes(*s) for s in shapes]
    budget = max(need) + min(need)
    assert _expected_launches(shapes, 1 << 40, 8, 8) == 6
    with gpu.overrides(align_mode="strip", align_tile="8x8", align_tb_bytes=budget):
        before = gpu.kernel_launch_count()
        first = gpu.align_batch(trips)
        count = gpu.kernel_launch_count() - before
        second = gpu.align_batch(trips)
    assert count == _expected_launches(shapes, budget, 8, 8) and count > 6
    for i in range(len(trips)):
        assert _same(first[i], ref[i]), i
        assert _same(second[i], ref[i]), i
    _check_all_modes(gpu, trips, ref, align_tile="8x8")


@pytest.mark.gpu
def test_gpu_strip_aligns_what_the_cube_budget_refuses(gpu, orc):
    """12 x (10,20,20) under tile 8x8 with a budget between one triple's strip need and its full cube: tiled is
    TSA_ENOMEM, strip and lowmem=True give the oracle's alignments; one byte below the strip need is TSA_ENOMEM."""
    trips, ref = _ref(orc, "capability")
    need = sum(_strip_need(10, 20, 20, 8, 8))
    cube = _cube_bytes(10, 20, 20)
    assert need == 25200 and need < 30000 < cube
    with gpu.overrides(align_mode="tiled", align_tile="8x8", align_tb_bytes=30000):
        with pytest.raises(gpu.TsaError) as e:
            gpu.align_batch(trips)
        assert e.value.rc == gpu.TSA_ENOMEM
    with gpu.overrides(align_tile="8x8", align_tb_bytes=30000):
        with pytest.raises(gpu.TsaError) as e:                     # not lowmem, no mode: the cube is over the budget
            gpu.align_batch(trips)
        assert e.value.rc == gpu.TSA_ENOMEM
    for budget in (30000, need):
        with gpu.overrides(align_mode="strip", align_tile="8x8", align_tb_bytes=budget):
            before = gpu.kernel_launch_count()
            got = gpu.align_batch(trips)
            assert gpu.kernel_launch_count() - before == 12 * 4    # a chunk per triple: forward + 3 strips
        with gpu.overrides(align_tile="8x8", align_tb_bytes=budget):
            low = gpu.align_batch(trips, lowmem=True)
        for i in range(12):
            assert _same(got[i], ref[i]), (budget, i)
            assert _same(low[i], ref[i]), (budget, i)
    with gpu.overrides(align_mode="strip", align_tile="8x8", align_tb_bytes=need - 1):
        with pytest.raises(gpu.TsaError) as e:
            gpu.align_batch(trips)
        assert e.value.rc == gpu.TSA_ENOMEM
    with gpu.overrides(align_tile="8x8", align_tb_bytes=need - 1):
        with pytest.raises(gpu.TsaError) as e:
            gpu.align_batch(trips, lowmem=True)
        assert e.value.rc == gpu.TSA_ENOMEM


@pytest.mark.gpu
def test_gpu_lowmem_keeps_a_set_align_mode(gpu, orc):
    """A set align_mode holds under lowmem=True: plane makes no counted launch; without it lowmem strips."""
    trips, ref = _ref(orc, "seams")
    with gpu.overrides(align_mode="plane", align_tile="8x8"):
        before = gpu.kernel_launch_count()
        got = gpu.align_batch(trips, lowmem=True)
        assert gpu.kernel_launch_count() - before == 0
    assert all(_same(g, r) for g, r in zip(got, ref))
    with gpu.overrides(align_tile="8x8"):
        before = gpu.kernel_launch_count()
        got = gpu.align_batch(trips, lowmem=True)
        assert gpu.kernel_launch_count() - before == 1 + 3         # forward + 3 strips (24 rows: 3 strips of 8)
    assert all(_same(g, r) for g, r in zip(got, ref))
