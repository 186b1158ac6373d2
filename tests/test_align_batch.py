"""tsa_align_batch: batched traceback. A triple whose (y,z) planes fit one
workgroup is swept by the resident kernel (csrc/align_kernel.hip, one launch
per chunk of pointer cubes), the others by the batched plane sweep; either way
every triple must come out as tsa_align_gpu and the oracle's independent
traceback give it -- score, start and moves. The resident schedule itself is
replayed on the CPU by tools/align_emu.py (no GPU needed)."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

# the parameter sets of test_align.py::test_gpu_align_random
KWS = [dict(), dict(s3_mode=1), dict(score_bits=0), dict(score_bits=6),
       dict(match=3, mismatch=-1, gap_open=2, gap_extend=2, score_bits=16)]


def _rand_triple(rng, la, lb, lc, hi=5):
    return tuple(rng.integers(0, hi, n).astype(np.uint8) for n in (la, lb, lc))


def _same(got, ref):
    return got[0] == ref[0] and tuple(got[1]) == tuple(ref[1]) and np.array_equal(got[2], ref[2])


def _check_path(tsa, a, b, c, score, start, moves, params=None, rescore=True):
    la, lb, lc = len(a), len(b), len(c)
    assert min(start) == 0 and all(v >= 0 for v in start)          # leaves a zero face
    used = np.sum([tsa.MOVE_CONSUMES[t] for t in moves], axis=0)
    assert tuple(int(v) for v in np.asarray(start) + used) == (la, lb, lc)  # ends at (LA,LB,LC)
    if rescore:
        assert tsa.path_score(a, b, c, start, moves, params) == score


def _raw_call(tsa, seqs, offsets, n, p, null=None):
    """tsa_align_batch through ctypes with outputs sized for the batch; the
    output named by `null` is passed as NULL."""
    u8, i32, i64 = (ctypes.POINTER(t) for t in (ctypes.c_uint8, ctypes.c_int32, ctypes.c_int64))
    seqs = np.ascontiguousarray(seqs, np.uint8)
    offsets = np.ascontiguousarray(offsets, np.int64)
    m = max(abs(n), 1)
    out = dict(scores=np.zeros(m, np.int32), moves=np.zeros(max(len(seqs), 1), np.uint8),
               n_moves=np.zeros(m, np.int32), starts=np.zeros(3 * m, np.int32))
    arg = lambda k, t: None if k == null else out[k].ctypes.data_as(t)
    return tsa.lib().tsa_align_batch(seqs.ctypes.data_as(u8), offsets.ctypes.data_as(i64), n, ctypes.byref(p),
                                     arg("scores", i32), arg("moves", u8), arg("n_moves", i32),
                                     arg("starts", i32), 0)


# ---- CPU ---------------------------------------------------------------------

def test_align_batch_is_exported(tsa):
    assert "tsa_align_batch" in tsa.EXPORTS
    assert hasattr(tsa.lib(), "tsa_align_batch") and callable(tsa.align_batch)


def test_align_batch_argument_checks(tsa):
    """Validation comes before any device work: TSA_EINVAL on any host."""
    p = tsa.TsaParams.default()
    seqs, offs = tsa.pack_batch([([0, 1], [1, 2], [2, 3]), ([0], [1], [2])])
    for null in ("scores", "moves", "n_moves", "starts"):
        assert _raw_call(tsa, seqs, offs, 2, p, null=null) == tsa.TSA_EINVAL, null
    assert _raw_call(tsa, seqs, offs, -1, p) == tsa.TSA_EINVAL
    assert _raw_call(tsa, np.zeros(6, np.uint8), np.array([0, 3, 2, 6], np.int64), 1, p) == tsa.TSA_EINVAL
    bad = seqs.copy()
    bad[1] = 9                                                     # a symbol > 4
    assert _raw_call(tsa, bad, offs, 2, p) == tsa.TSA_EINVAL
    assert _raw_call(tsa, seqs, offs, 2, tsa.TsaParams.default(score_bits=3)) == tsa.TSA_EINVAL
    with pytest.raises(tsa.TsaError) as e:
        tsa.align_batch([([0, 7], [1], [2])])
    assert e.value.rc == tsa.TSA_EINVAL


def test_align_batch_empty_is_ok(tsa):
    assert _raw_call(tsa, np.zeros(1, np.uint8), np.zeros(1, np.int64), 0, tsa.TsaParams.default()) == tsa.TSA_OK
    assert tsa.align_batch([]) == []


def test_align_batch_no_cpu_fallback(tsa):
    if tsa.device_count() > 0:
        pytest.skip("a HIP device is visible")
    with pytest.raises(tsa.TsaError) as e:
        tsa.align_batch([([0, 1], [0, 1], [0, 1])])
    assert e.value.rc == tsa.TSA_ENODEV


def test_align_overrides_are_accepted_and_reported(tsa):
    assert "align_mode" in tsa.OVERRIDES and "align_tb_bytes" in tsa.OVERRIDES
    L = tsa.lib()
    assert L.tsa_set_override(b"align_mode", b"plane") == tsa.TSA_OK
    assert L.tsa_set_override(b"align_tb_bytes", b"4096") == tsa.TSA_OK
    assert tsa.get_overrides() == {"align_mode": "plane", "align_tb_bytes": "4096"}
    tsa.clear_overrides()
    with tsa.overrides(align_mode="resident"):
        assert tsa.get_overrides() == {"align_mode": "resident"}
    assert tsa.get_overrides() == {}


def _emu_align(a, b, c, op):
    import align_emu
    return align_emu.align(a, b, c, op.match, op.mismatch, op.gap_open, op.gap_extend, bool(op.s3_mode),
                           op.score_bits)


@pytest.mark.parametrize("kw", KWS)
def test_resident_schedule_emulated_matches_oracle(orc, kw):
    """tools/align_emu.py -- two zeroed buffers, publication only while the
    cell is real, the register history -- against the oracle, move for move."""
    rng = np.random.default_rng(7 + len(kw) + kw.get("score_bits", 1))
    op = orc.default_params(**kw)
    shapes = [tuple(int(v) for v in rng.integers(1, 13, 3)) for _ in range(6)]
    for la, lb, lc in shapes + [(1, 1, 1), (1, 9, 9), (9, 1, 9), (9, 9, 1)]:
        a, b, c = _rand_triple(rng, la, lb, lc)
        assert _same(_emu_align(a, b, c, op), orc.align(a, b, c, op)), (kw, la, lb, lc)


def test_resident_schedule_emulated_all_a(orc):
    for n in (1, 2, 7):
        z = np.zeros(n, np.uint8)
        s, st, mv = _emu_align(z, z, z, orc.default_params())
        assert s == 3 * n and st == (0, 0, 0) and list(mv) == [0] * n


# ---- GPU ---------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("kw", KWS)
def test_gpu_align_batch_mixed(gpu, orc, kw):
    """24 triples of independent random lengths 1..40: the resident kernel and
    the batched plane sweep agree with each other and with the oracle."""
    rng = np.random.default_rng(300 + len(kw) + kw.get("score_bits", 1))
    p, op = gpu.TsaParams.default(**kw), orc.default_params(**kw)
    trips = [_rand_triple(rng, *(int(v) for v in rng.integers(1, 41, 3))) for _ in range(24)]
    ref = [orc.align(a, b, c, op) for a, b, c in trips]
    with gpu.overrides(align_mode="resident"):
        res = gpu.align_batch(trips, p)
    with gpu.overrides(align_mode="plane"):
        pla = gpu.align_batch(trips, p)
    assert len(res) == len(pla) == 24
    for i, t in enumerate(trips):
        shape = tuple(len(s) for s in t)
        assert _same(res[i], pla[i]), (i, shape)
        assert _same(res[i], ref[i]), (i, shape)


EDGES = [(1, 1, 1), (40, 1, 1), (1, 64, 64), (8, 64, 64), (8, 1, 64), (8, 64, 1), (8, 7, 63), (8, 7, 65),
         (8, 3, 130), (8, 64, 72), (8, 72, 64), (150, 5, 5)]


@pytest.mark.gpu
def test_gpu_align_batch_geometry_edges(gpu, orc):
    """One batch, caller order kept: a full-capacity resident triple (64 x 64
    positions), rows that straddle a wave along z (lc = 63, 65, 130), single
    rows and columns, two triples over the resident capacity (64 x 72,
    72 x 64: the plane sweep inside a resident batch) and LA far beyond
    lb + lc."""
    rng = np.random.default_rng(41)
    trips = [_rand_triple(rng, *s) for s in EDGES]
    with gpu.overrides(align_mode="resident"):
        got = gpu.align_batch(trips)
    for (a, b, c), g, shape in zip(trips, got, EDGES):
        assert _same(g, orc.align(a, b, c)), shape
        assert _same(g, gpu.align(a, b, c)), shape


@pytest.mark.gpu
def test_gpu_align_batch_golden(gpu, orc, golden):
    groups = {}
    for c in golden:
        if len(c["a"]) * len(c["b"]) * len(c["c"]) <= 64 ** 3:
            groups.setdefault(tuple(sorted(c["params"].items())), []).append(c)
    used = 0
    for key, cases in groups.items():
        kw = dict(key)
        got = gpu.align_batch([(c["a"], c["b"], c["c"]) for c in cases], gpu.TsaParams.default(**kw))
        for c, g in zip(cases, got):
            ref = orc.align(c["a"], c["b"], c["c"], orc.default_params(**kw))
            assert g[0] == c["score"], c["name"]
            assert _same(g, ref), c["name"]
            used += 1
    assert used >= 10


@pytest.mark.gpu
def test_gpu_align_batch_chunks(gpu, orc, synth):
    """12 triples of 24^3 under a budget of 5 cubes (4*24*47*24 bytes each):
    three chunks, so three resident launches whatever la+lb+lc is."""
    trips = [synth.triple(500 + i, 24) for i in range(12)]
    ref = [orc.align(a, b, c) for a, b, c in trips]
    cube = 4 * 24 * 47 * 24
    with gpu.overrides(align_mode="resident", align_tb_bytes=5 * cube):
        before = gpu.kernel_launch_count()
        got = gpu.align_batch(trips)
        assert gpu.kernel_launch_count() - before == 3
    assert all(_same(g, r) for g, r in zip(got, ref))
    with gpu.overrides(align_mode="plane", align_tb_bytes=5 * cube):
        assert all(_same(g, r) for g, r in zip(gpu.align_batch(trips), ref))
    with gpu.overrides(align_tb_bytes=cube - 1):
        with pytest.raises(gpu.TsaError) as e:
            gpu.align_batch(trips)
        assert e.value.rc == gpu.TSA_ENOMEM
    assert all(_same(g, r) for g, r in zip(gpu.align_batch(trips), ref))


@pytest.mark.gpu
def test_gpu_align_batch_64_cubes(gpu, orc, synth):
    """64 x 64^3 in one call: every workgroup at the resident capacity."""
    z = np.zeros(64, np.uint8)
    trips = ([synth.triple(i, 64) for i in range(32)] + [synth.related_triple(900 + i, 64) for i in range(16)] +
             [(z, z, z)] * 16)
    got = gpu.align_batch(trips)
    assert [g[0] for g in got] == [int(s) for s in gpu.score_batch(trips)]
    for (a, b, c), (s, st, mv) in zip(trips, got):
        _check_path(gpu, a, b, c, s, st, mv)
    for s, st, mv in got[48:]:
        assert s == 192 and st == (0, 0, 0) and len(mv) == 64 and not mv.any()
    for (a, b, c), g in zip(trips[:8], got[:8]):
        assert _same(g, orc.align(a, b, c))


@pytest.mark.gpu
def test_gpu_align_batch_wrapping_bits(gpu, orc):
    """SCORE_BITS 6 wraps: both paths take the literal wrapped candidates, so
    their argmaxes -- not only their scores -- match the oracle's."""
    rng = np.random.default_rng(66)
    p, op = gpu.TsaParams.default(score_bits=6), orc.default_params(score_bits=6)
    trips = [_rand_triple(rng, *(int(v) for v in rng.integers(33, 38, 3)), hi=4) for _ in range(8)]
    ref = [orc.align(a, b, c, op) for a, b, c in trips]
    for mode in ("resident", "plane"):
        with gpu.overrides(align_mode=mode):
            got = gpu.align_batch(trips, p)
        for g, r, t in zip(got, ref, trips):
            assert _same(g, r), (mode, tuple(len(s) for s in t))
            _check_path(gpu, *t, g[0], g[1], g[2], p, rescore=False)
