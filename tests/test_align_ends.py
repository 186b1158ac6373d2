"""tsa_align_batch_ends: the traceback with a free end. TSA_END_FACE lets the
path stop on a far face, TSA_END_ANY at any cell; the resident and the tiled
kernel search the end cell as they sweep (csrc/align_step.h) and tb_walk_ends
walks from it.

Reference for every test, with the oracle as it is: the recurrence is causal,
so the MAX7 of cell (x, y, z) is oracle.score(a[:x], b[:y], c[:z]). Brute force
over all prefixes gives v[x, y, z]; the end cell is the first maximum among the
candidates in (x, y, z) order; score, start and moves are oracle.align of those
prefixes. Every test first asserts on the reference alone that its inputs say
something: the end differs from the corner in at least three quarters of the
triples, and at least one triple has a tied maximum.

The shapes are the smallest that reach each instantiation:
  resident K=1   12 triples of 5..12 a side, mixed lengths in one call
  resident K=2   (5, 40, 30): 1200 positions
  resident K=4   (6, 48, 44): 2112 positions
  tiled K=1      (13, 11, 16) under align_tile=5x7 (3 x 3 tiles of 4 x 6),
                 11x4 (1 x 4 tiles) and 3x16 (4 x 1 tiles)
  tiled K=2      (3, 70, 60) under align_tile=35x30: 2 x 2 tiles of 1050
                 positions (a (3, 70, 50) cube would give tiles of 35 x 25 = 875
                 positions, which the tiled launch runs with K=1)
  tiled K=3      (3, 96, 44) under align_tile=48x44: 2 x 1 tiles of 2112
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG_DIR, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))

# tests/test_align_batch.py::KWS and the set whose maxima tie in every triple
KWS = [dict(), dict(s3_mode=1), dict(score_bits=0), dict(score_bits=6),
       dict(match=3, mismatch=-1, gap_open=2, gap_extend=2, score_bits=16), dict(score_bits=4)]
BIG_KWS = [dict(), dict(score_bits=4)]
MODES = ["face", "any"]
CONSUMES = ((1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1))
LDS_MAX = 160 * 1024


# ---- inputs --------------------------------------------------------------------

def _uniform(rng, la, lb, lc):
    return tuple(rng.integers(0, 5, n).astype(np.uint8) for n in (la, lb, lc))


def _core_tails(rng):
    """A shared core of 6 symbols; every sequence has a private head of 0..2 and
    a private tail of 1..5 symbols."""
    core = rng.integers(0, 5, 6).astype(np.uint8)
    return tuple(np.concatenate([rng.integers(0, 5, int(rng.integers(0, 3))).astype(np.uint8), core,
                                 rng.integers(0, 5, int(rng.integers(1, 6))).astype(np.uint8)]) for _ in range(3))


def _small_batch():
    rng = np.random.default_rng(11)
    uni = [_uniform(rng, *(int(v) for v in rng.integers(5, 13, 3))) for _ in range(6)]
    return uni + [_core_tails(rng) for _ in range(6)]


def _shape(seed, la, lb, lc):
    """One uniform triple. The seeds below are the first from 100 on whose
    reference meets the conditions of refs_of under every parameter set of the
    case and in both modes (the end off the corner, a tied maximum)."""
    return [_uniform(np.random.default_rng(seed), la, lb, lc)]


# name -> (overrides of the GPU call, triples, parameter sets)
CASES = {
    "resident_k1": (dict(), _small_batch(), KWS),
    "resident_k2": (dict(), _shape(100, 5, 40, 30), BIG_KWS),
    "resident_k4": (dict(), _shape(101, 6, 48, 44), BIG_KWS),
    "tiled_k1_3x3": (dict(align_mode="tiled", align_tile="5x7"), _shape(114, 13, 11, 16), KWS),
    "tiled_k1_1x4": (dict(align_mode="tiled", align_tile="11x4"), _shape(114, 13, 11, 16), BIG_KWS),
    "tiled_k1_4x1": (dict(align_mode="tiled", align_tile="3x16"), _shape(114, 13, 11, 16), BIG_KWS),
    "tiled_k2": (dict(align_mode="tiled", align_tile="35x30"), _shape(100, 3, 70, 60), BIG_KWS),
    "tiled_k3": (dict(align_mode="tiled", align_tile="48x44"), _shape(100, 3, 96, 44), BIG_KWS),
}
CASE_PARAMS = [(name, k) for name, (_, _, kws) in CASES.items() for k in range(len(kws))]


# ---- the reference ---------------------------------------------------------------

_V = {}


def prefix_scores(orc, a, b, c, kw):
    """v[x, y, z] = oracle.score(a[:x], b[:y], c[:z]) for 1 <= x, y, z, in one
    oracle.score_batch call over all the prefix triples; computed once."""
    key = (a.tobytes(), b.tobytes(), c.tobytes(), tuple(sorted(kw.items())))
    if key not in _V:
        la, lb, lc = len(a), len(b), len(c)
        parts, offs = [], [0]
        for x in range(1, la + 1):
            for y in range(1, lb + 1):
                for z in range(1, lc + 1):
                    parts += [a[:x], b[:y], c[:z]]
                    offs += [offs[-1] + x, offs[-1] + x + y, offs[-1] + x + y + z]
        v = orc.score_batch(np.concatenate(parts), np.asarray(offs, np.int64), orc.default_params(**kw),
                            nthreads=min(8, os.cpu_count() or 1))
        _V[key] = np.asarray(v, np.int64).reshape(la, lb, lc)
    return _V[key]


def ref_end(orc, a, b, c, kw, mode):
    """((score, start, moves, end), tied): the oracle's end-free alignment."""
    v = prefix_scores(orc, a, b, c, kw)
    la, lb, lc = v.shape
    cand = np.ones(v.shape, bool)
    if mode == "face":
        cand[:la - 1, :lb - 1, :lc - 1] = False
    masked = np.where(cand, v, np.iinfo(np.int64).min)
    best = int(masked.max())
    x1, y1, z1 = (int(i) + 1 for i in np.unravel_index(int(np.argmax(masked)), v.shape))  # the first in (x, y, z) order
    s, st, mv = orc.align(a[:x1], b[:y1], c[:z1], orc.default_params(**kw))
    assert s == best
    return (s, st, mv, (x1, y1, z1)), int((masked == best).sum()) > 1


def refs_of(orc, name, k, mode):
    """The references of a case under its k-th parameter set, after the
    conditions on the reference alone."""
    _, trips, kws = CASES[name]
    out = [ref_end(orc, a, b, c, kws[k], mode) for a, b, c in trips]
    off_corner = sum(r[3] != tuple(len(s) for s in t) for (r, _), t in zip(out, trips))
    assert 4 * off_corner >= 3 * len(trips), (name, kws[k], mode, off_corner)
    assert any(tied for _, tied in out), (name, kws[k], mode)
    return [r for r, _ in out]


def same(got, ref):
    return (got[0] == ref[0] and tuple(got[1]) == tuple(ref[1]) and np.array_equal(got[2], ref[2]) and
            tuple(got[3]) == tuple(ref[3]))


def check_path(tsa, a, b, c, got, params=None, rescore=True):
    score, start, moves, end = got
    assert min(start) == 0 and all(v >= 0 for v in start) and len(moves) >= 1
    used = np.sum([CONSUMES[int(t)] for t in moves], axis=0)
    assert tuple(int(v) for v in np.asarray(start) + used) == tuple(end)
    assert all(1 <= e <= len(s) for e, s in zip(end, (a, b, c)))
    if rescore:
        assert tsa.path_score(a, b, c, start, moves, params) == score


def _emu_args(op):
    return op.match, op.mismatch, op.gap_open, op.gap_extend, bool(op.s3_mode), op.score_bits


def _tile(ov):
    return tuple(int(v) for v in ov["align_tile"].split("x")) if "align_tile" in ov else None


# ---- CPU: the interface ---------------------------------------------------------

def _raw_call(tsa, seqs, offsets, n, p, end_mode, null=None):
    u8, i32, i64 = (ctypes.POINTER(t) for t in (ctypes.c_uint8, ctypes.c_int32, ctypes.c_int64))
    seqs = np.ascontiguousarray(seqs, np.uint8)
    offsets = np.ascontiguousarray(offsets, np.int64)
    m = max(abs(n), 1)
    out = dict(scores=np.zeros(m, np.int32), moves=np.zeros(max(len(seqs), 1), np.uint8),
               n_moves=np.zeros(m, np.int32), starts=np.zeros(3 * m, np.int32), ends=np.zeros(3 * m, np.int32))
    arg = lambda k, t: None if k == null else out[k].ctypes.data_as(t)
    return tsa.lib().tsa_align_batch_ends(seqs.ctypes.data_as(u8), offsets.ctypes.data_as(i64), n, ctypes.byref(p),
                                          end_mode, arg("scores", i32), arg("moves", u8), arg("n_moves", i32),
                                          arg("starts", i32), arg("ends", i32), 0)


def test_ends_is_exported(tsa):
    assert "tsa_align_batch_ends" in tsa.EXPORTS
    assert hasattr(tsa.lib(), "tsa_align_batch_ends") and callable(tsa.align_batch_ends)
    assert (tsa.END_CORNER, tsa.END_FACE, tsa.END_ANY) == (0, 1, 2)


def test_ends_argument_checks(tsa):
    """Validation comes before any device work: TSA_EINVAL on any host."""
    p = tsa.TsaParams.default()
    seqs, offs = tsa.pack_batch([([0, 1], [1, 2], [2, 3]), ([0], [1], [2])])
    for mode in (tsa.END_CORNER, tsa.END_FACE, tsa.END_ANY):
        for null in ("scores", "moves", "n_moves", "starts", "ends"):
            assert _raw_call(tsa, seqs, offs, 2, p, mode, null=null) == tsa.TSA_EINVAL, (mode, null)
        assert _raw_call(tsa, seqs, offs, -1, p, mode) == tsa.TSA_EINVAL
        assert _raw_call(tsa, np.zeros(6, np.uint8), np.array([0, 3, 2, 6], np.int64), 1, p, mode) == tsa.TSA_EINVAL
        bad = seqs.copy()
        bad[1] = 9                                                 # a symbol > 4
        assert _raw_call(tsa, bad, offs, 2, p, mode) == tsa.TSA_EINVAL
        assert _raw_call(tsa, seqs, offs, 2, tsa.TsaParams.default(score_bits=3), mode) == tsa.TSA_EINVAL
    for mode in (3, -1):
        assert _raw_call(tsa, seqs, offs, 2, p, mode) == tsa.TSA_EINVAL
    for end in ("corner", "any"):
        with pytest.raises(tsa.TsaError) as e:
            tsa.align_batch_ends([([0, 7], [1], [2])], end=end)
        assert e.value.rc == tsa.TSA_EINVAL
    for end in ("middle", 3, None):
        with pytest.raises(tsa.TsaError) as e:
            tsa.align_batch_ends([([0], [1], [2])], end=end)
        assert e.value.rc == tsa.TSA_EINVAL


def test_ends_empty_is_ok(tsa):
    for mode in (0, 1, 2):
        assert _raw_call(tsa, np.zeros(1, np.uint8), np.zeros(1, np.int64), 0, tsa.TsaParams.default(), mode) == tsa.TSA_OK
    assert tsa.align_batch_ends([], end="face") == []


def test_ends_no_cpu_fallback(tsa):
    if tsa.device_count() > 0:
        pytest.skip("a HIP device is visible")
    for end in ("corner", "face", "any", 2):
        with pytest.raises(tsa.TsaError) as e:
            tsa.align_batch_ends([([0, 1], [0, 1], [0, 1])], end=end)
        assert e.value.rc == tsa.TSA_ENODEV


def test_ends_refuses_the_paths_without_an_end_search(tsa):
    """align_mode = plane, strip or grid: TSA_EINVAL under face and any, found
    without a device; under corner the call is tsa_align_batch's and goes on."""
    p = tsa.TsaParams.default()
    seqs, offs = tsa.pack_batch([([0, 1], [1, 2], [2, 3])])
    beyond = (tsa.TSA_OK,) if tsa.device_count() > 0 else (tsa.TSA_ENODEV,)
    for mode in ("plane", "strip", "grid"):
        with tsa.overrides(align_mode=mode):
            assert _raw_call(tsa, seqs, offs, 1, p, tsa.END_ANY) == tsa.TSA_EINVAL, mode
            assert _raw_call(tsa, seqs, offs, 1, p, tsa.END_FACE) == tsa.TSA_EINVAL, mode
            assert _raw_call(tsa, seqs, offs, 1, p, tsa.END_CORNER) in beyond, mode
    for mode in ("resident", "tiled"):
        with tsa.overrides(align_mode=mode):
            assert _raw_call(tsa, seqs, offs, 1, p, tsa.END_ANY) in beyond, mode


def test_cli_end_option():
    """--end is parsed: a bad value or --end without --align is a usage error
    (exit 2); a good one gets as far as the device."""
    cli = os.path.join(PKG_DIR, "bin", "tsa")
    dat = os.path.join(ROOT, "tests", "golden", "dat")
    files = [f"{dat}/A_seq.dat", f"{dat}/B_seq.dat", f"{dat}/C_seq.dat"]
    run = lambda *extra: subprocess.run([cli, *files, *extra], capture_output=True, text=True)
    assert run("--align", "--end", "middle").returncode == 2
    assert run("--align", "--end").returncode == 2
    assert run("--end", "any").returncode == 2
    for end in ("corner", "face", "any"):
        r = run("--align", "--end", end)
        if r.returncode == 0:
            assert "alignment start" in r.stdout
            assert ("alignment end (x1,y1,z1) = (" in r.stdout) == (end != "corner")
        else:
            assert r.returncode == 1 and "no HIP device" in r.stderr and "usage" not in r.stderr
    plain, corner = run("--align"), run("--align", "--end", "corner")
    assert (plain.returncode, plain.stdout) == (corner.returncode, corner.stdout)


# ---- CPU: the reference's conditions and the replay ------------------------------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,k", CASE_PARAMS)
def test_reference_conditions(orc, name, k, mode):
    """Every GPU case says something on the reference alone: the end is off
    the corner in three quarters of its triples and a maximum is tied."""
    _, trips, _ = CASES[name]
    for (s, st, mv, end), (a, b, c) in zip(refs_of(orc, name, k, mode), trips):
        assert len(mv) >= 1 and min(st) == 0
        if mode == "face":
            assert any(e == len(q) for e, q in zip(end, (a, b, c)))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", range(len(KWS)))
def test_resident_replay_matches_oracle(orc, mode, k):
    """tools/align_ends_emu.py on the resident schedule: the key folded at each
    cell in schedule order, the reduction and the walk from the end record."""
    import align_ends_emu as emu
    op = orc.default_params(**KWS[k])
    _, trips, _ = CASES["resident_k1"]
    for (a, b, c), ref in zip(trips, refs_of(orc, "resident_k1", k, mode)):
        got = emu.align(a, b, c, emu.END_MODES[mode], *_emu_args(op))
        assert same(got, ref), (KWS[k], mode, got[3], ref[3])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["tiled_k1_3x3", "tiled_k1_1x4", "tiled_k1_4x1"])
def test_tiled_replay_matches_oracle(orc, name, mode):
    """The tiled schedule on the (13, 11, 16) cube: the running best of a
    thread lives across the tiles."""
    import align_ends_emu as emu
    ov, trips, kws = CASES[name]
    for k, kw in enumerate(kws):
        op = orc.default_params(**kw)
        for (a, b, c), ref in zip(trips, refs_of(orc, name, k, mode)):
            got = emu.align(a, b, c, emu.END_MODES[mode], *_emu_args(op), tile=_tile(ov))
            assert same(got, ref), (name, kw, mode, got[3], ref[3])


def _early_cube():
    """B and C are A's first symbols and unrelated tails: the best cell lies in
    the first tile of 3 x 3."""
    rng = np.random.default_rng(31)
    a = rng.integers(0, 4, 4).astype(np.uint8)
    tail = lambda n: ((a[-1] + 1 + rng.integers(0, 2, n)) % 4).astype(np.uint8)
    return a, np.concatenate([a, tail(7)]), np.concatenate([a, tail(12)])


@pytest.mark.parametrize("mode", MODES)
def test_replay_best_cell_in_a_tile_that_is_not_the_last(orc, mode):
    import align_ends_emu as emu
    import align_tiled_emu
    a, b, c = _early_cube()
    ref, _ = ref_end(orc, a, b, c, {}, mode)
    TY, TZ, nty, ntz = align_tiled_emu.tile_geom(len(b), len(c), 5, 7)
    assert (nty, ntz) == (3, 3)
    if mode == "any":
        assert ref[3] == (4, 4, 4) and ref[0] == 12
    assert ((ref[3][1] - 1) // TY, (ref[3][2] - 1) // TZ) != (nty - 1, ntz - 1)
    got = emu.align(a, b, c, emu.END_MODES[mode], tile=(5, 7))
    assert same(got, ref), (got, ref)


def test_replay_key_is_order_free(orc):
    """A plain max is the whole rule: the thread count and the order in which
    the cells are folded change nothing, ties included (score_bits = 4)."""
    import align_ends_emu as emu
    op = orc.default_params(score_bits=4)
    _, trips, _ = CASES["resident_k1"]
    for mode in MODES:
        for (a, b, c), ref in zip(trips[:4], refs_of(orc, "resident_k1", len(KWS) - 1, mode)[:4]):
            for nt, shuffle, tile in ((64, 5, None), (128, 6, None), (64, 7, (5, 7)), (192, None, (3, 4))):
                got = emu.align(a, b, c, emu.END_MODES[mode], *_emu_args(op), tile=tile, nt=nt, shuffle=shuffle)
                assert same(got, ref), (mode, nt, shuffle, tile)
    # the key: score first, then the smaller x, y, z, then the lower state
    k = lambda S, x, y, z: emu.cell_key(S, x, y, z, 9, 11)
    lo = (-5,) * 7
    assert k((3,) + lo[1:], 2, 9, 11) > k((2,) * 7, 1, 1, 1)
    assert k((3,) * 7, 1, 9, 11) > k((3,) * 7, 2, 1, 1) and k((3,) * 7, 2, 3, 11) > k((3,) * 7, 2, 4, 1)
    assert k((3,) * 7, 2, 3, 4) > k((3,) * 7, 2, 3, 5)
    assert emu.decode(k((-7, 3, 3, -2, 3, 0, 1), 5, 9, 11), 9, 11) == (5, 9, 11, 1, 3)
    assert emu.decode(k((-2048,) * 7, 1, 1, 1), 9, 11) == (1, 1, 1, 0, -2048)
    assert emu.key_fits(2 ** 15, 2 ** 15, 2 ** 15) and not emu.key_fits(2 ** 16, 2 ** 15, 2 ** 15)


def test_replay_corner_is_the_batch_replay(orc):
    import align_emu
    import align_ends_emu as emu
    _, trips, _ = CASES["resident_k1"]
    for a, b, c in trips[:3]:
        s, st, mv, end = emu.align(a, b, c, emu.END_CORNER)
        r = align_emu.align(a, b, c)
        assert (s, st) == r[:2] and np.array_equal(mv, r[2]) and end == (len(a), len(b), len(c))


def _unstaged():
    """(163711, 1, 1): A is one symbol too long to be staged in LDS. Every cell
    has y == lb, so face and any name the same cells. A avoids b's symbol but at
    x = la-2 and x = la: a tied maximum whose first cell is not the corner, and
    both lie where only an unstaged lookup reaches."""
    la = LDS_MAX - (32 * 2 * 2 + 2) + 1
    rng = np.random.default_rng(41)
    a = rng.integers(1, 4, la).astype(np.uint8)
    a[la - 3] = a[la - 1] = 0
    return a, np.zeros(1, np.uint8), np.zeros(1, np.uint8)


def test_unstaged_reference(tsa, orc):
    """The reference of the unstaged triple is the oracle's best_range -- the
    first cell in (x, y, z) order of the largest MAX7 without the wrap, which is
    the rule of TSA_END_ANY wherever nothing wraps -- since brute force over
    163711 prefixes is out of reach. On the small triples it is checked against
    the brute force first (score_bits = 0: no wrap); the long triple runs under
    the default 12 bits, which its states stay far inside (a cube that long is
    TSA_ERANGE without a wrap)."""
    kw = dict(score_bits=0)
    _, trips, _ = CASES["resident_k1"]
    for a, b, c in trips:
        r, _ = ref_end(orc, a, b, c, kw, "any")
        br = orc.best_range(a, b, c, orc.default_params(**kw))
        assert (br.bmax, br.at_max) == (r[0], r[3])
    a, b, c = _unstaged()
    la = len(a)
    with tsa.overrides(align_mode="resident"):
        assert tsa.describe_align_plan(1, la, 1, 1) == "resident lds=%d" % ((32 * 4 + 2 + 15) // 16 * 16)
        assert tsa.describe_align_plan(1, la - 1, 1, 1) == "resident lds=%d" % LDS_MAX
    lo, hi = orc.state_range(a, b, c)
    assert -2048 < lo and hi < 2047                                  # nothing wraps in 12 bits
    br = orc.best_range(a, b, c)
    assert (br.bmax, br.at_max) == (3, (la - 2, 1, 1))
    assert orc.score(a, b, c) == 3                                   # tied with the corner


# ---- GPU -------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,k", CASE_PARAMS)
def test_gpu_ends_match_oracle(gpu, orc, name, k, mode):
    """Every instantiation of both kernels, in both modes: score, start, moves
    and end as the oracle gives them on the prefixes."""
    ov, trips, kws = CASES[name]
    refs = refs_of(orc, name, k, mode)
    p = gpu.TsaParams.default(**kws[k])
    with gpu.overrides(**ov):
        tiles = _tile(ov)
        if tiles:
            la, lb, lc = (len(s) for s in trips[0])
            assert gpu.describe_align_plan(1, la, lb, lc).startswith("tiled ")
        got = gpu.align_batch_ends(trips, p, end=mode)
    wraps = kws[k].get("score_bits", 12) in (4, 6)
    for (a, b, c), g, r in zip(trips, got, refs):
        assert same(g, r), (name, kws[k], mode, g[0], g[1], g[3], r[0], r[1], r[3])
        check_path(gpu, a, b, c, g, p, rescore=not wraps)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_gpu_ends_unstaged_a(gpu, orc, mode):
    """A resident triple whose A is read from global memory (163711, 1, 1), next
    to a small one that stages it; reference: test_unstaged_reference."""
    kw = dict()
    a, b, c = _unstaged()
    small = CASES["resident_k1"][1][0]
    p, op = gpu.TsaParams.default(**kw), orc.default_params(**kw)
    x1 = len(a) - 2
    s, st, mv = orc.align(a[:x1], b, c, op)
    want = [(s, st, mv, (x1, 1, 1)), ref_end(orc, *small, kw, mode)[0]]
    assert s == 3
    got = gpu.align_batch_ends([(a, b, c), small], p, end=mode)
    for t, g, r in zip([(a, b, c), small], got, want):
        assert same(g, r), (mode, g[0], g[1], g[3], r[0], r[1], r[3])
        check_path(gpu, *t, g, p)


@pytest.mark.gpu
def test_gpu_ends_corner_is_align_batch(gpu):
    """TSA_END_CORNER: tsa_align_batch output for output, under every plan, and
    ends = the lengths."""
    rng = np.random.default_rng(51)
    trips = _small_batch() + [_uniform(rng, 4, 70, 9), _uniform(rng, 9, 20, 66)]
    for ov in (dict(), dict(align_mode="plane"), dict(align_mode="tiled", align_tile="5x7"),
               dict(align_mode="strip", align_tile="5x7"), dict(align_mode="grid", align_tile="5x7")):
        with gpu.overrides(**ov):
            want = gpu.align_batch(trips)
            got = gpu.align_batch_ends(trips, end="corner")
        for t, g, w in zip(trips, got, want):
            assert g[0] == w[0] and g[1] == w[1] and np.array_equal(g[2], w[2]), ov
            assert g[3] == tuple(len(s) for s in t)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_gpu_ends_mixed_chunks_and_launch_count(gpu, orc, mode):
    """Resident and tiled triples interleaved in one call that spans three
    chunks under align_tb_bytes: results in the caller's order, and every chunk
    queues the counted launches of tsa_align_batch under align_mode = tiled,
    [resident] + [tiled]."""
    big = _shape(114, 13, 11, 16)[0]                       # over the 5x7 tile: tiled
    rng = np.random.default_rng(61)
    tiny = [_uniform(rng, 6, 5, 7), _uniform(rng, 7, 4, 6), _uniform(rng, 5, 5, 5)]
    trips = [tiny[0], big, tiny[1], big, big, tiny[2]]
    cube = lambda t: 4 * len(t[1]) * (len(t[0]) + len(t[2]) - 1) * len(t[2])
    budget = cube(big) + cube(tiny[0]) + cube(tiny[1])     # chunks: [tiny, big, tiny] [big] [big, tiny]
    refs = [ref_end(orc, a, b, c, {}, mode)[0] for a, b, c in trips]
    with gpu.overrides(align_mode="tiled", align_tile="5x7", align_tb_bytes=budget):
        plans = [gpu.describe_align_plan(1, *(len(s) for s in t)).split()[0] for t in trips]
        assert plans == ["resident", "tiled", "resident", "tiled", "tiled", "resident"]
        before = gpu.kernel_launch_count()
        want_batch = gpu.align_batch(trips)
        batch_launches = gpu.kernel_launch_count() - before
        before = gpu.kernel_launch_count()
        got = gpu.align_batch_ends(trips, end=mode)
        assert gpu.kernel_launch_count() - before == batch_launches == 2 + 1 + 2
    assert len(want_batch) == len(got) == 6
    for t, g, r in zip(trips, got, refs):
        assert same(g, r), (mode, g[3], r[3])
        check_path(gpu, *t, g)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_gpu_ends_rows(gpu, orc, mode):
    """tsa_align_rows_async on the uploaded moves of an end-free result renders
    the rows render_alignment gives: both work from start and moves."""
    import torch
    trips = _small_batch()
    got = gpu.align_batch_ends(trips, end=mode)
    seqs, offs = gpu.pack_batch(trips)
    n, total = len(trips), len(seqs)
    mv = np.zeros(total, np.uint8)
    for i, g in enumerate(got):
        mv[int(offs[3 * i]):int(offs[3 * i]) + len(g[2])] = g[2]
    nm = np.array([len(g[2]) for g in got], np.int32)
    st = np.array([v for g in got for v in g[1]], np.int32)
    d = [torch.from_numpy(x).cuda() for x in (seqs, offs, mv, nm, st)]
    rows = torch.full((3 * total,), 0xEE, dtype=torch.uint8, device="cuda")
    gpu.align_rows_async(d[0].data_ptr(), d[1].data_ptr(), n, d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(),
                         rows.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    rows = rows.cpu().numpy()
    for i, (t, g) in enumerate(zip(trips, got)):
        at, ln = 3 * int(offs[3 * i]), sum(len(s) for s in t)
        text = tuple("".join(gpu.ROW_LETTERS[v] for v in rows[at + r * ln:at + r * ln + len(g[2])]) for r in range(3))
        assert text == gpu.render_alignment(*t, g[1], g[2]), i
        # the rows hold the symbols between start and end, and nothing beyond the end
        for r, (seq, x0, x1) in enumerate(zip(t, g[1], g[3])):
            assert text[r].replace("-", "") == "".join("ATCGN"[int(v)] for v in seq[x0:x1])
