"""tsa_align_batch on inputs whose optimal path runs through the whole cube.

The traceback tests of test_align_batch.py and test_align_tiled.py compare
score, start and moves with the oracle, which looks only at the cells on the
one optimal path; with independent random sequences that path is short and
stays near the end corner, inside one tile. Here the inputs (tests/_align_cases.py:
identical, related, planted) have long paths, and the CPU tests below state on
the oracle's own paths what makes the GPU comparison sensitive: seams and tile
corners crossed, tiles visited, move states and transitions seen. A GPU test can
then not pass on a path that misses the seams.

Also reached here, and by nothing else: A read from global memory because it
does not fit in LDS next to the planes (la >= 163711 at lb = lc = 1), the
65535-triple chunk cap, the default tiled/plane rule decided per chunk inside
one call, and the moves layout when offsets[0] != 0.

Which instantiation a tiled launch runs follows from the largest tile of the
call (1024 positions per K): the list K1 as a whole is a K = 2 launch, since
49 x 35 = 1715 positions, so its 33 x 25 cases also go through a call of their
own, which is the K = 1 launch at a real tile size. (70,65,49) and (60,49,70)
fit the resident kernel, so they are tiled only with align_tile spelled out;
64x48 is the default tile."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

import _align_cases as ac  # noqa: E402

# the parameter sets of test_align_batch.KWS, and one more
KWS = [dict(), dict(s3_mode=1), dict(score_bits=0), dict(score_bits=6),
       dict(match=3, mismatch=-1, gap_open=2, gap_extend=2, score_bits=16),
       dict(match=2, mismatch=-3, gap_open=3, gap_extend=1, score_bits=16)]

TILED_NT = 1024  # positions per K of a tiled launch (csrc/align_tiled_kernel.hip)

# name -> (overrides on top of align_mode=tiled, shapes with their tile and grid, extra identical shifts)
LISTS = {
    "K1": (dict(align_tile="64x48"), [((70, 65, 49), (33, 25, 2, 2)), ((60, 49, 70), (49, 35, 1, 2))],
           [((70, 65, 49), 8)]),
    "K2": (dict(), [((70, 65, 65), (33, 33, 2, 2)), ((130, 130, 130), (44, 44, 3, 3))], []),
    "K3": (dict(), [((80, 64, 72), (64, 36, 1, 2)), ((128, 128, 96), (64, 48, 2, 2))], [((128, 128, 96), 16)]),
}
LIST_SEED = {"K1": 101, "K2": 102, "K3": 103}
# the calls of a list: (expected K, the tiles whose cases go into the call)
CALLS = {"K1": [(2, None), (1, (33, 25))], "K2": [(2, None)], "K3": [(3, None)]}

RESIDENT = [(1, (40, 30, 30)), (2, (60, 40, 45)), (4, (70, 64, 64))]  # (K of align_kernel.hip, shape)

UNSTAGED = [(163710, 1, 1), (163711, 1, 1), (163900, 3, 4)]
LDS_MAX = 160 * 1024


def _same(got, ref):
    return got[0] == ref[0] and tuple(got[1]) == tuple(ref[1]) and np.array_equal(got[2], ref[2])


def _cube_bytes(la, lb, lc):
    return 4 * lb * (la + lc - 1) * lc


@functools.lru_cache(maxsize=None)
def _list_cases(name):
    """[(kind, shape, tile, (a, b, c))] of a real-tile-size list."""
    _, shapes, shifted = LISTS[name]
    rng = np.random.default_rng(LIST_SEED[name])
    out = []
    for shape, tile in shapes:
        out.append(("identical", shape, tile, ac.identical(rng, *shape)))
        out.append(("related", shape, tile, ac.related(rng, *shape)))
        out.append(("planted", shape, tile, ac.planted(rng, *shape, 10)))
    tiles = dict(shapes)
    for shape, shift in shifted:
        out.append(("identical+%d" % shift, shape, tiles[shape], ac.identical(rng, *shape, shift=shift)))
    return out


@functools.lru_cache(maxsize=None)
def _list_refs(orc, name):
    return [orc.align(*t) for _, _, _, t in _list_cases(name)]


@functools.lru_cache(maxsize=None)
def _tiny(orc, ki):
    """24 planted triples with lengths 8..40 and their oracle alignments, once per parameter set."""
    rng = np.random.default_rng(900 + ki)
    trips = [ac.planted(rng, *(int(v) for v in rng.integers(8, 41, 3)), 10) for _ in range(24)]
    return trips, [orc.align(a, b, c, orc.default_params(**KWS[ki])) for a, b, c in trips]


@functools.lru_cache(maxsize=None)
def _resident_cases(shape):
    rng = np.random.default_rng(200 + shape[0])
    return [ac.identical(rng, *shape), ac.related(rng, *shape), ac.planted(rng, *shape, 10)]


@functools.lru_cache(maxsize=None)
def _unstaged_cases():
    """A random, its last 6 symbols 2 0 3 1 2 0 (neighbours differ); b and c
    copies of A's last symbols, c one symbol behind b. Then one small triple."""
    rng = np.random.default_rng(300)
    out = []
    for la, lb, lc in UNSTAGED:
        a = rng.integers(0, 4, la).astype(np.uint8)
        a[-6:] = (2, 0, 3, 1, 2, 0)
        out.append((a, a[la - lb:].copy(), a[la - lc - 1:la - 1].copy()))
    out.append(tuple(rng.integers(0, 4, n).astype(np.uint8) for n in (20, 16, 16)))
    return out


@functools.lru_cache(maxsize=None)
def _unstaged_refs(orc):
    return [orc.align(*t) for t in _unstaged_cases()]


def _seven():
    """7 distinct triples of lengths 1..2, each with lb or lc = 2: over a 1x1 tile."""
    rng = np.random.default_rng(400)
    shapes = [(1, 2, 1), (2, 1, 2), (1, 2, 2), (2, 2, 1), (2, 2, 2), (1, 1, 2), (2, 2, 2)]
    return [tuple(rng.integers(0, 4, n).astype(np.uint8) for n in s) for s in shapes]


# ---- CPU: the generators and the geometry ------------------------------------

def test_recipes_shapes_and_alphabet():
    rng = np.random.default_rng(1)
    for la, lb, lc in ((1, 1, 1), (8, 40, 9), (70, 65, 49)):
        for t in (ac.identical(rng, la, lb, lc), ac.identical(rng, la, lb, lc, shift=3), ac.related(rng, la, lb, lc),
                  ac.planted(rng, la, lb, lc, 10)):
            assert tuple(len(s) for s in t) == (la, lb, lc)
            assert all(s.dtype == np.uint8 and (len(s) == 0 or s.max() < 4) for s in t)
    a, b, c = ac.identical(np.random.default_rng(2), 20, 18, 10, shift=5)
    assert np.array_equal(a[:18], b) and np.array_equal(a[5:15], c)
    again = ac.planted(np.random.default_rng(3), 30, 30, 30, 10)
    assert all(np.array_equal(u, v) for u, v in zip(again, ac.planted(np.random.default_rng(3), 30, 30, 30, 10)))


def test_path_geometry_counts():
    """A hand-made path over 2 x 2 tiles of 3 x 2: from (0,0,0) M to (1,1,1), Iy
    to y = 4 (a y seam at 3 -> 4), Iyz to (1,5,2), Iyz to (1,6,3) (a z seam),
    Iz to z = 4; and a diagonal from (0,1,0) that takes the corner (3,2) -> (4,3)."""
    tiles, ny, nz, nc = ac.path_geometry((0, 0, 0), [0, 2, 2, 2, 5, 5, 3], 3, 2)
    assert (tiles, ny, nz, nc) == ({(0, 0), (1, 0), (1, 1)}, 1, 1, 0)
    tiles, ny, nz, nc = ac.path_geometry((0, 1, 0), [0, 0, 0, 0], 3, 2)
    assert (tiles, ny, nz, nc) == ({(0, 0), (1, 1)}, 0, 0, 1)
    assert ac.path_cells((2, 0, 1), [0, 1, 6]) == [(3, 1, 2), (4, 1, 2), (5, 1, 3)]
    assert ac.move_pairs([0, 0, 1, 0]) == {(0, 0), (0, 1), (1, 0)}


# ---- CPU: the conditions on the reference ------------------------------------

def _list_geometry(tsa, orc, name):
    """Per case (tiles, ny, nz, ncorner) of the oracle's path over the tile grid
    tsa.describe_align_plan gives, which must be the list's expected one."""
    ov, _, _ = LISTS[name]
    cases, refs = _list_cases(name), _list_refs(orc, name)
    out = []
    with tsa.overrides(align_mode="tiled", **ov):
        for (kind, shape, tile, _), ref in zip(cases, refs):
            assert ac.plan_tiles(tsa, len(cases), *shape) == tile, (name, kind, shape)
            out.append(ac.path_geometry(ref[1], ref[2], tile[0], tile[1]))
    return out


@pytest.mark.parametrize("name", sorted(LISTS))
def test_real_tile_lists_cross_seams_and_corners(tsa, orc, name):
    cases = _list_cases(name)
    geo = _list_geometry(tsa, orc, name)
    ny, nz, nc = (sum(g[k] for g in geo) for k in (1, 2, 3))
    most = max(len(g[0]) for g in geo)
    print("%s: y seams %d, z seams %d, corners %d, most tiles on a path %d" % (name, ny, nz, nc, most))
    assert ny >= 1 and nz >= 2 and nc >= 1 and most >= 3, (name, ny, nz, nc, most)
    # the corner is the pure diagonal's: identical on square tiles, the shifted one elsewhere
    corner_kinds = {kind for (kind, _, tile, _), g in zip(cases, geo) if g[3]}
    want = "identical" if all(t[0] == t[1] for _, _, t, _ in cases) else "identical+%d" % LISTS[name][2][0][1]
    assert want in corner_kinds, (name, corner_kinds)
    # the instantiation of every call of the list
    for k, only in CALLS[name]:
        pos = max(t[0] * t[1] for _, _, t, _ in cases if only is None or t[:2] == only)
        assert (pos + TILED_NT - 1) // TILED_NT == k, (name, only, pos)


def test_real_tile_lists_use_all_states(orc):
    states = set()
    for name in LISTS:
        for ref in _list_refs(orc, name):
            states |= {int(m) for m in ref[2]}
    assert states == set(range(7))
    assert sorted(k for name in LISTS for k, _ in CALLS[name]) == [1, 2, 2, 3]


@pytest.mark.parametrize("ki", range(len(KWS)))
def test_tiny_planted_cross_seams_and_corners(tsa, orc, ki):
    trips, refs = _tiny(orc, ki)
    ny = nz = nc = 0
    states, pairs = set(), set()
    with tsa.overrides(align_mode="tiled", align_tile="5x7"):
        for (a, b, c), ref in zip(trips, refs):
            assert min(len(a), len(b), len(c)) >= 8 and max(len(a), len(b), len(c)) <= 40
            TY, TZ, nty, ntz = ac.plan_tiles(tsa, 24, len(a), len(b), len(c))
            assert TY <= 5 and TZ <= 7 and nty >= 2 and ntz >= 2
            g = ac.path_geometry(ref[1], ref[2], TY, TZ)
            ny, nz, nc = ny + g[1], nz + g[2], nc + g[3]
            states |= {int(m) for m in ref[2]}
            pairs |= ac.move_pairs(ref[2])
    print("tiny %s: y seams %d, z seams %d, corners %d, pairs %d" % (KWS[ki], ny, nz, nc, len(pairs)))
    assert ny >= 20 and nz >= 20 and nc >= 3, (ny, nz, nc)
    assert states == set(range(7))
    assert len(pairs) >= 30, len(pairs)


def test_resident_lists_have_long_paths(orc):
    """No seams in the resident kernel; what the long inputs add is a path that
    spans the (y,z) plane the workgroup holds -- at least max(lb,lc) moves, from
    y or z at most 2 -- and all 7 states. The three shapes are the three
    instantiations (1024 positions per K, no K = 3)."""
    states = set()
    for k, shape in RESIDENT:
        pos = shape[1] * shape[2]
        assert (1 if pos <= 1024 else 2 if pos <= 2048 else 4) == k and pos <= 4096
        for a, b, c in _resident_cases(shape):
            ref = orc.align(a, b, c)
            assert len(ref[2]) >= max(shape[1:]) and min(ref[1][1:]) <= 2, (shape, ref[1], len(ref[2]))
            states |= {int(m) for m in ref[2]}
    assert states == set(range(7))


def test_unstaged_a_cases_sit_on_the_lds_edge(tsa, orc):
    """(163710,1,1) fills LDS to the last byte with A staged, (163711,1,1) and
    (163900,3,4) cannot stage it; and A moved by one symbol either way gives
    another alignment, so an A index that is off by one shows."""
    for (la, lb, lc), staged in zip(UNSTAGED, (True, False, False)):
        need = 32 * (lb + 1) * (lc + 1) + lb + lc + la
        assert (need <= LDS_MAX) == staged, (la, lb, lc)
        with tsa.overrides(align_mode="resident"):
            txt = tsa.describe_align_plan(4, la, lb, lc)
        assert txt == "resident lds=%d" % (LDS_MAX if staged else (need - la + 15) // 16 * 16), txt
    assert 32 * 2 * 2 + 2 + 163710 == LDS_MAX
    with tsa.overrides(align_mode="tiled", align_tile="2x2"):
        plans = [tsa.describe_align_plan(4, *s).split()[0] for s in UNSTAGED + [(20, 16, 16)]]
        assert plans == ["resident", "resident", "tiled", "tiled"]
        assert ac.plan_tiles(tsa, 4, 163900, 3, 4) == (2, 2, 2, 2)
    # A as a lookup that is one off would see it, the index clamped as align_sym_a clamps it. With
    # lb = lc = 1 the path is one move at x = la, where a_{la+1} clamps to a_la: only the
    # lookup that is one behind can show there; (163900,3,4) shows both.
    for (a, b, c), ref in zip(_unstaged_cases()[:3], _unstaged_refs(orc)):
        assert b[-1] == a[-1] and c[-1] == a[-2] and a[-1] != a[-2]
        behind, ahead = np.concatenate([a[:1], a[:-1]]), np.concatenate([a[1:], a[-1:]])
        assert not _same(orc.align(behind, b, c), ref), len(a)
        if len(b) > 1:
            assert not _same(orc.align(ahead, b, c), ref), len(a)


def _op_args(op):
    return op.match, op.mismatch, op.gap_open, op.gap_extend, bool(op.s3_mode), op.score_bits


def test_schedules_emulated_on_planted_paths(orc):
    """tools/align_emu.py and tools/align_tiled_emu.py on 6 planted triples of
    lengths 8..14, one per parameter set, against the oracle move for move."""
    import align_emu
    import align_tiled_emu
    rng = np.random.default_rng(950)
    for kw in KWS:
        op = orc.default_params(**kw)
        a, b, c = ac.planted(rng, *(int(v) for v in rng.integers(8, 15, 3)), 10)
        ref = orc.align(a, b, c, op)
        shape = (len(a), len(b), len(c))
        assert len(ref[2]) >= 8, (kw, shape)
        assert _same(align_emu.align(a, b, c, *_op_args(op)), ref), (kw, shape)
        for tile in ((4, 4), (5, 7)):
            assert _same(align_tiled_emu.align(a, b, c, *_op_args(op), tile), ref), (kw, shape, tile)


# ---- GPU ---------------------------------------------------------------------

def _ok(gpu, what, call):
    """The call's result; a refusal (a 160 KiB launch, say) fails here with its code."""
    try:
        return call()
    except gpu.TsaError as e:
        pytest.fail("%s: rc=%d, expected TSA_OK (%s)" % (what, e.rc, e))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(LISTS))
def test_gpu_tiled_long_paths(gpu, orc, name):
    """A list of real tile sizes through the tiled kernel, call by call
    (CALLS): every triple tiled with the expected tile, equal to the oracle
    and to the plane sweep."""
    ov = LISTS[name][0]
    cases, refs = _list_cases(name), _list_refs(orc, name)
    for _, only in CALLS[name]:
        pick = [i for i, (_, _, tile, _) in enumerate(cases) if only is None or tile[:2] == only]
        trips = [cases[i][3] for i in pick]
        with gpu.overrides(align_mode="tiled", **ov):
            for i in pick:
                assert ac.plan_tiles(gpu, len(pick), *cases[i][1]) == cases[i][2], cases[i][:2]
                assert gpu.describe_align_plan(len(pick), *cases[i][1]).startswith("tiled "), cases[i][:2]
            before = gpu.kernel_launch_count()
            got = gpu.align_batch(trips)
            assert gpu.kernel_launch_count() - before == 1
        with gpu.overrides(align_mode="plane"):
            pla = gpu.align_batch(trips)
        for j, i in enumerate(pick):
            assert _same(got[j], refs[i]), (name, only, cases[i][:2])
            assert _same(got[j], pla[j]), (name, only, cases[i][:2])


@pytest.mark.gpu
def test_gpu_tiled_mixed_tile_sizes(gpu, orc):
    """The related cases of K1 and K3 interleaved in one call: triples of
    33 x 25 and 49 x 35 tiles inside the K = 3 launch that 64 x 48 asks for."""
    pick = lambda name: [(c, r) for c, r in zip(_list_cases(name), _list_refs(orc, name)) if c[0] == "related"]
    both = [cr for pair in zip(pick("K1"), pick("K3")) for cr in pair]
    assert len(both) == 4
    with gpu.overrides(align_mode="tiled", align_tile="64x48"):
        for (kind, shape, tile, _), _ in both:
            assert ac.plan_tiles(gpu, len(both), *shape) == tile
        before = gpu.kernel_launch_count()
        got = gpu.align_batch([c[3] for c, _ in both])
        assert gpu.kernel_launch_count() - before == 1
    for g, (c, r) in zip(got, both):
        assert _same(g, r), c[:2]


@pytest.mark.gpu
@pytest.mark.parametrize("tile", ["5x7", "3x16"])
@pytest.mark.parametrize("ki", range(len(KWS)))
def test_gpu_tiled_planted_tiny(gpu, orc, ki, tile):
    trips, refs = _tiny(orc, ki)
    with gpu.overrides(align_mode="tiled", align_tile=tile):
        got = gpu.align_batch(trips, gpu.TsaParams.default(**KWS[ki]))
    assert len(got) == 24
    for i, t in enumerate(trips):
        assert _same(got[i], refs[i]), (i, tuple(len(s) for s in t))


@pytest.mark.gpu
def test_gpu_resident_long_paths(gpu, orc):
    """identical, related and planted through align_kernel.hip's K = 1, 2 and 4,
    a call each; the K = 2 call under every parameter set."""
    for k, shape in RESIDENT:
        trips = _resident_cases(shape)
        for kw in (KWS if k == 2 else KWS[:1]):
            with gpu.overrides(align_mode="resident"):
                assert gpu.describe_align_plan(3, *shape).startswith("resident")
                before = gpu.kernel_launch_count()
                got = gpu.align_batch(trips, gpu.TsaParams.default(**kw))
                assert gpu.kernel_launch_count() - before == 1
            for g, (a, b, c) in zip(got, trips):
                assert _same(g, orc.align(a, b, c, orc.default_params(**kw))), (shape, kw)


@pytest.mark.gpu
def test_gpu_align_unstaged_a(gpu, orc):
    """A staged up to the last byte of LDS, and read from global memory beyond
    that, in both kernels and next to a small triple that stages it."""
    trips, refs = _unstaged_cases(), _unstaged_refs(orc)
    shapes = [tuple(len(s) for s in t) for t in trips]
    assert shapes == UNSTAGED + [(20, 16, 16)]
    for ov in (dict(align_mode="resident"), dict(align_mode="tiled", align_tile="2x2")):
        with gpu.overrides(**ov):
            got = _ok(gpu, "align_batch under %s" % ov, lambda: gpu.align_batch(trips))
        for g, r, s in zip(got, refs, shapes):
            assert _same(g, r), (ov, s, g[:2], r[:2])


@pytest.mark.gpu
def test_gpu_align_chunk_cap(gpu, orc):
    """65535 + 70 triples: two chunks whatever the budget, the second one of 70.
    Period 7 against chunks of 65535 = 7 * 9362 + 1: a triple placed one off
    is another triple."""
    seven = _seven()
    refs = [orc.align(*t) for t in seven]
    assert len({(r[0], r[1], tuple(r[2].tolist())) for r in refs}) == 7      # a neighbour's result is another one
    n = 65535 + 70
    lens = np.array([[len(s) for s in seven[i % 7]] for i in range(n)], np.int64).ravel()
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    seqs = np.concatenate([np.concatenate(seven[i % 7]) for i in range(n)]).astype(np.uint8)
    for ov, launches in ((dict(align_mode="resident"), 2), (dict(align_mode="plane"), 0),
                         (dict(align_mode="tiled", align_tile="1x1"), 2)):
        with gpu.overrides(**ov):
            assert all(gpu.describe_align_plan(n, *(len(s) for s in t)).split()[0] == ov["align_mode"] for t in seven)
            before = gpu.kernel_launch_count()
            got = gpu.align_batch(seqs=seqs, offsets=offsets)
            assert gpu.kernel_launch_count() - before == launches, ov
        assert len(got) == n
        bad = [i for i in range(n) if not _same(got[i], refs[i % 7])]
        assert not bad, (ov, len(bad), bad[:5])


@pytest.mark.gpu
def test_gpu_align_default_rule_per_chunk(gpu, orc):
    """No mode override, 300 triples of (1,65,65) under a budget of 256 cubes:
    the chunk of 256 takes the tiled kernel (one counted launch), the chunk of
    44 the plane sweep (none)."""
    rng = np.random.default_rng(500)
    trips = [ac.related(rng, 1, 65, 65) for _ in range(300)]
    refs = [orc.align(*t) for t in trips]
    with gpu.overrides(align_tb_bytes=256 * _cube_bytes(1, 65, 65)):
        assert gpu.describe_align_plan(256, 1, 65, 65).startswith("tiled ")
        assert gpu.describe_align_plan(44, 1, 65, 65) == "plane"
        before = gpu.kernel_launch_count()
        got = gpu.align_batch(trips)
        assert gpu.kernel_launch_count() - before == 1
    bad = [i for i in range(300) if not _same(got[i], refs[i])]
    assert not bad, bad[:5]


@pytest.mark.gpu
def test_gpu_align_batch_offset_base(gpu, orc):
    """include/trialign.h: triple i's moves start at moves[offsets[3i] - offsets[0]].
    5 bytes that are no symbols stand in front of the sequences."""
    rng = np.random.default_rng(600)
    trips = [ac.planted(rng, *s, 4) for s in ((9, 4, 7), (3, 12, 5), (6, 6, 11))]
    refs = [orc.align(*t) for t in trips]
    packed, offs = gpu.pack_batch(trips)
    seqs = np.concatenate([np.full(5, 7, np.uint8), packed])
    offsets = (offs + 5).astype(np.int64)
    total, tail = len(packed), 8
    u8, i32, i64 = (ctypes.POINTER(t) for t in (ctypes.c_uint8, ctypes.c_int32, ctypes.c_int64))
    scores, n_moves, starts = np.zeros(3, np.int32), np.zeros(3, np.int32), np.zeros(9, np.int32)
    moves = np.full(total + tail, 0xEE, np.uint8)
    p = gpu.TsaParams.default()

    def call(device):
        return gpu.lib().tsa_align_batch(seqs.ctypes.data_as(u8), offsets.ctypes.data_as(i64), 3, ctypes.byref(p),
                                         scores.ctypes.data_as(i32), moves.ctypes.data_as(u8),
                                         n_moves.ctypes.data_as(i32), starts.ctypes.data_as(i32), device)

    assert call(gpu.device_count()) == gpu.TSA_ENODEV
    assert (moves == 0xEE).all() and not scores.any()
    assert call(0) == gpu.TSA_OK
    for i, (ref, t) in enumerate(zip(refs, trips)):
        at, slot, nm = int(offsets[3 * i]) - 5, sum(len(s) for s in t), int(n_moves[i])
        assert at == int(offs[3 * i])
        got = (int(scores[i]), tuple(int(v) for v in starts[3 * i:3 * i + 3]), moves[at:at + nm])
        assert _same(got, ref), i
        assert 1 <= nm < slot and (moves[at + nm:at + slot] == 0xEE).all(), i
    assert (moves[total:] == 0xEE).all()
