"""The device-resident traceback entry points: tsa_align_workspace_size,
tsa_align_batch_async and tsa_align_rows_async (include/trialign.h), and
align_batch_device over them.

CPU tests: the exports, every argument check (validation comes before any
device work, so fake device addresses never reach a device), and the sizes of
the workspace against the needs tsa_describe_align_plan prints. GPU tests:
results against oracle.align and against the synchronous align_batch of the
same path, the caller's order and layout, the chunks of a small workspace with
their counted launches, stream order, and the gapped rows against
render_alignment. Shapes are the smallest at which each mechanism can go wrong:
tiles of 5x7 put cubes of a dozen symbols through several tiles, (8,65,64) is
the smallest triple that does not fit a workgroup (65*64 > 4096)."""
import ctypes
import functools
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _align_cases as ac  # noqa: E402

PATHS = ("tiled", "strip", "grid")
KWS = [dict(), dict(score_bits=6), dict(match=3, mismatch=-1, gap_open=2, gap_extend=2, score_bits=16)]
SHAPES = [(9, 11, 13), (3, 4, 5), (14, 6, 15), (6, 5, 7), (1, 1, 1)]  # under align_tile=5x7: larger, resident, ...
TILE = "5x7"
FAKE = 0x1000  # a non-null, 256-byte aligned address that is never dereferenced: validation fails first


def _same(got, ref):
    return got[0] == ref[0] and tuple(got[1]) == tuple(ref[1]) and np.array_equal(got[2], ref[2])


@functools.lru_cache(maxsize=None)
def _batch():
    """The interleaved batch of test 1: the larger triples run through the cube."""
    rng = np.random.default_rng(7100)
    return tuple(ac.identical(rng, *s) if s[1] > 5 or s[2] > 7 else ac.planted(rng, *s, 3) for s in SHAPES)


@functools.lru_cache(maxsize=None)
def _refs(ki):
    import oracle
    return [oracle.align(a, b, c, oracle.default_params(**KWS[ki])) for a, b, c in _batch()]


def _raw(tsa, args):
    """tsa_align_batch_async with integer addresses; returns the rc."""
    (d_seqs, d_off, h_off, n, p, path, d_sc, d_mv, d_nm, d_st, d_ws, ws) = args
    h = None if h_off is None else np.ascontiguousarray(h_off, np.int64)
    hp = None if h is None else h.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    pp = None if p is None else ctypes.byref(p)
    return tsa.lib().tsa_align_batch_async(d_seqs, d_off, hp, n, pp, path, d_sc, d_mv, d_nm, d_st, d_ws, ws, None)


# ---------------------------------------------------------------- CPU ------

def test_exports(tsa):
    for name in ("tsa_align_workspace_size", "tsa_align_batch_async", "tsa_align_rows_async"):
        assert name in tsa.EXPORTS and hasattr(tsa.lib(), name)
    assert tsa.ALIGN_PATHS == {"tiled": 0, "strip": 1, "grid": 2} and tsa.ROW_LETTERS[tsa.ROW_GAP] == "-"


def test_async_argument_checks(tsa):
    p = tsa.TsaParams.default()
    offs = np.array([0, 3, 7, 12, 14, 15, 19], np.int64)
    good = [FAKE, FAKE, offs, 2, p, 0, FAKE, FAKE, FAKE, FAKE, FAKE, 1 << 20]
    before = tsa.kernel_launch_count()

    def rc(**kw):
        names = ("d_seqs", "d_off", "h_off", "n", "p", "path", "d_sc", "d_mv", "d_nm", "d_st", "d_ws", "ws")
        a = list(good)
        for k, v in kw.items():
            a[names.index(k)] = v
        return _raw(tsa, a)

    for name in ("d_seqs", "d_off", "h_off", "p", "d_sc", "d_mv", "d_nm", "d_st", "d_ws"):
        assert rc(**{name: None}) == tsa.TSA_EINVAL, name
    assert rc(n=-1) == tsa.TSA_EINVAL
    assert rc(h_off=np.array([0, 3, 2, 12, 14, 15, 19])) == tsa.TSA_EINVAL      # not monotone
    assert rc(h_off=np.array([0, 3, 3, 12, 14, 15, 19])) == tsa.TSA_EINVAL      # a length below 1
    assert rc(p=tsa.TsaParams.default(score_bits=3)) == tsa.TSA_EINVAL
    assert rc(path=3) == tsa.TSA_EINVAL and rc(path=-1) == tsa.TSA_EINVAL
    assert rc(d_ws=FAKE + 128) == tsa.TSA_EINVAL                                # not 256-byte aligned
    for mode in ("plane", "resident"):
        with tsa.overrides(align_mode=mode):
            assert rc() == tsa.TSA_EINVAL, mode
            with pytest.raises(tsa.TsaError) as e:
                tsa.align_workspace_size(offs)
            assert e.value.rc == tsa.TSA_EINVAL
    with tsa.overrides(align_tile="0x4"):
        assert rc() == tsa.TSA_EINVAL
    assert rc(n=0) == tsa.TSA_OK
    if tsa.device_count() == 0:  # with a device a valid call would use the fake addresses
        assert rc() == tsa.TSA_ENODEV
        for path in (1, 2):
            assert rc(path=path) == tsa.TSA_ENODEV
    assert tsa.kernel_launch_count() == before


def test_rows_argument_checks(tsa):
    f = tsa.lib().tsa_align_rows_async
    good = [FAKE, FAKE, 2, FAKE, FAKE, FAKE, FAKE, None]
    for k in (0, 1, 3, 4, 5, 6):
        a = list(good)
        a[k] = None
        assert f(*a) == tsa.TSA_EINVAL, k
    assert f(FAKE, FAKE, -1, FAKE, FAKE, FAKE, FAKE, None) == tsa.TSA_EINVAL
    assert f(FAKE, FAKE, 0, FAKE, FAKE, FAKE, FAKE, None) == tsa.TSA_OK
    if tsa.device_count() == 0:
        assert f(*good) == tsa.TSA_ENODEV


def test_workspace_size_argument_checks(tsa):
    f = tsa.lib().tsa_align_workspace_size
    p = tsa.TsaParams.default()
    offs = np.array([0, 3, 7, 12], np.int64)
    op = offs.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    lo, hi = ctypes.c_size_t(7), ctypes.c_size_t(7)
    assert f(None, 1, ctypes.byref(p), 0, ctypes.byref(lo), ctypes.byref(hi)) == tsa.TSA_EINVAL
    assert f(op, 1, None, 0, ctypes.byref(lo), ctypes.byref(hi)) == tsa.TSA_EINVAL
    assert f(op, 1, ctypes.byref(p), 0, None, ctypes.byref(hi)) == tsa.TSA_EINVAL
    assert f(op, 1, ctypes.byref(p), 0, ctypes.byref(lo), None) == tsa.TSA_EINVAL
    assert f(op, -1, ctypes.byref(p), 0, ctypes.byref(lo), ctypes.byref(hi)) == tsa.TSA_EINVAL
    assert f(op, 1, ctypes.byref(p), 7, ctypes.byref(lo), ctypes.byref(hi)) == tsa.TSA_EINVAL
    bad = np.array([0, 3, 3, 12], np.int64)
    assert f(bad.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), 1, ctypes.byref(p), 0, ctypes.byref(lo),
             ctypes.byref(hi)) == tsa.TSA_EINVAL
    assert f(op, 0, ctypes.byref(p), 0, ctypes.byref(lo), ctypes.byref(hi)) == tsa.TSA_OK
    assert f(op, 1, ctypes.byref(p), 0, ctypes.byref(lo), ctypes.byref(hi)) == tsa.TSA_OK and lo.value > 0


def _offsets(shapes, base=0):
    return np.concatenate([[base], base + np.cumsum(np.array(shapes, np.int64).ravel())]).astype(np.int64)


def test_workspace_size_grows_with_the_batch(tsa):
    shapes = [(7, 6, 5), (8, 65, 64), (3, 3, 3), (20, 70, 66), (1, 1, 1)]
    for path in PATHS:
        prev = (0, 0)
        for k in range(1, len(shapes) + 1):
            lo, hi = tsa.align_workspace_size(_offsets(shapes[:k]), path=path)
            assert lo <= hi and lo >= prev[0] and hi >= prev[1] and lo % 4 == 0, (path, k)
            if k == 1:
                assert lo == hi                       # one triple, one chunk
            prev = (lo, hi)
        # full_bytes prices one chunk for all: it exceeds min_bytes by the other triples' needs
        assert hi > lo
    # the cube of a resident triple is its need on every path
    one = [tsa.align_workspace_size(_offsets([(7, 6, 5)]), path=path)[0] for path in PATHS]
    two = [tsa.align_workspace_size(_offsets([(7, 6, 5), (7, 6, 5)]), path=path)[1] for path in PATHS]
    fixed2 = [tsa.align_workspace_size(_offsets([(7, 6, 5), (7, 6, 5)]), path=path)[0] - 4 * 6 * 11 * 5
              for path in PATHS]
    assert all(t - f == 2 * 4 * 6 * 11 * 5 for t, f in zip(two, fixed2)) and len(set(one[1:])) == 1


def test_workspace_min_is_the_need_the_plan_prints(tsa):
    """One larger triple under align_tile=7x7: min_bytes for strip and for grid,
    each less the min_bytes of a batch of 1x1x1 triples with as many symbols
    (whose needs are equal on both paths), differ by exactly the difference of
    cube + faces tsa_describe_align_plan prints for strip and for grid."""
    shape = (10, 20, 18)
    ones = [(1, 1, 1)] * (sum(shape) // 3)
    need, net = {}, {}
    for path in ("strip", "grid"):
        with tsa.overrides(align_tile="7x7"):
            lo, hi = tsa.align_workspace_size(_offsets([shape]), path=path)
            base = tsa.align_workspace_size(_offsets(ones), path=path)[0]
            with tsa.overrides(align_mode=path):
                txt = tsa.describe_align_plan(1, *shape)
        m = re.match(rf"{path} tile=7x6 tiles=3x3 lds=\d+ cube=(\d+) faces=(\d+)$", txt)
        assert m, txt
        need[path], net[path] = int(m.group(1)) + int(m.group(2)), lo - base
        assert lo == hi
    assert need["strip"] != need["grid"]
    assert net["strip"] - net["grid"] == need["strip"] - need["grid"]
    # tiled: the whole cube and the tiled kernel's faces
    with tsa.overrides(align_tile="7x7"):
        lo_t = tsa.align_workspace_size(_offsets([shape]), path="tiled")[0]
        lo_s = tsa.align_workspace_size(_offsets([shape]), path="strip")[0]
        with tsa.overrides(align_mode="tiled"):
            faces = int(re.search(r"faces=(\d+)$", tsa.describe_align_plan(1, *shape)).group(1))
    walk = 256  # the walker records of one strip triple, one 256-byte region, are the fixed parts' difference
    assert (lo_t + walk) - lo_s == 4 * 20 * 27 * 18 + faces - need["strip"]
    # align_tb_bytes caps the budget: below the need no size works
    with tsa.overrides(align_tile="7x7", align_tb_bytes=need["grid"] - 1):
        with pytest.raises(tsa.TsaError) as e:
            tsa.align_workspace_size(_offsets([shape]), path="grid")
        assert e.value.rc == tsa.TSA_ENOMEM


# ---------------------------------------------------------------- GPU ------

class Dev:
    """A batch on the device as torch tensors, and one queued async call."""

    def __init__(self, tsa, trips, base=0, tail=0, fill=0):
        import torch
        self.tsa, self.torch, self.trips = tsa, torch, trips
        packed, offs = tsa.pack_batch(trips)
        self.seqs = np.concatenate([np.full(base, 7, np.uint8), packed])
        self.offsets = (offs + base).astype(np.int64)
        self.n, self.total = len(trips), len(packed)
        self.d_seqs, self.d_off = torch.from_numpy(self.seqs).cuda(), torch.from_numpy(self.offsets).cuda()
        self.d_sc = torch.zeros(self.n, dtype=torch.int32, device="cuda")
        self.d_nm = torch.full((self.n,), -1, dtype=torch.int32, device="cuda")
        self.d_st = torch.zeros(3 * self.n, dtype=torch.int32, device="cuda")
        self.d_mv = torch.full((self.total + tail,), fill, dtype=torch.uint8, device="cuda")
        self.d_rows = torch.full((3 * self.total + tail,), fill, dtype=torch.uint8, device="cuda")
        self.ws = None

    def sizes(self, path, params=None):
        return self.tsa.align_workspace_size(self.offsets, params, path)

    def queue(self, path="tiled", params=None, ws_bytes=None, stream=None):
        torch = self.torch
        if ws_bytes is None:
            ws_bytes = self.sizes(path, params)[1]
        self.ws = torch.empty(max(ws_bytes, 256), dtype=torch.uint8, device="cuda")
        s = (stream or torch.cuda.current_stream()).cuda_stream
        self.tsa.align_batch_async(self.d_seqs.data_ptr(), self.d_off.data_ptr(), self.offsets, self.d_sc.data_ptr(),
                                   self.d_mv.data_ptr(), self.d_nm.data_ptr(), self.d_st.data_ptr(),
                                   self.ws.data_ptr(), ws_bytes, s, params, path)

    def queue_rows(self, stream=None, moves=None):
        s = (stream or self.torch.cuda.current_stream()).cuda_stream
        d_mv, d_nm, d_st = moves or (self.d_mv, self.d_nm, self.d_st)
        self.tsa.align_rows_async(self.d_seqs.data_ptr(), self.d_off.data_ptr(), self.n, d_mv.data_ptr(),
                                  d_nm.data_ptr(), d_st.data_ptr(), self.d_rows.data_ptr(), s)

    def results(self):
        """After a synchronise: [(score, start, moves)] as align_batch returns them."""
        sc, nm, st, mv = (t.cpu().numpy() for t in (self.d_sc, self.d_nm, self.d_st, self.d_mv))
        out = []
        for i in range(self.n):
            at = int(self.offsets[3 * i] - self.offsets[0])
            out.append((int(sc[i]), tuple(int(v) for v in st[3 * i:3 * i + 3]), mv[at:at + max(int(nm[i]), 0)].copy()))
        return out

    def rows(self):
        """After a synchronise: per triple the three rows as text, n_moves columns each."""
        nm, rows = self.d_nm.cpu().numpy(), self.d_rows.cpu().numpy()
        out = []
        for i, t in enumerate(self.trips):
            at, ln = 3 * int(self.offsets[3 * i] - self.offsets[0]), sum(len(s) for s in t)
            out.append(tuple("".join(self.tsa.ROW_LETTERS[v] if v < 6 else "?"
                                     for v in rows[at + r * ln: at + r * ln + int(nm[i])]) for r in range(3)))
        return out


def _run(tsa, trips, path, params=None, ws_bytes=None):
    import torch
    d = Dev(tsa, trips)
    d.queue(path, params, ws_bytes)
    torch.cuda.synchronize()
    return d.results()


@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS)
def test_gpu_async_order_and_paths(gpu, orc, path):
    """Test 1: larger and resident triples interleaved, three parameter sets."""
    trips = list(_batch())
    with gpu.overrides(align_mode="tiled", align_tile=TILE):
        assert [gpu.describe_align_plan(1, *s).split()[0] for s in SHAPES] == \
            ["tiled", "resident", "tiled", "resident", "resident"]
        geo = [ac.plan_tiles(gpu, 1, *s) for s in SHAPES]
    for i in (0, 2):  # the reference's path crosses a y seam and a z seam: a condition on the oracle alone
        _, ny, nz, _ = ac.path_geometry(_refs(0)[i][1], _refs(0)[i][2], geo[i][0], geo[i][1])
        assert ny >= 1 and nz >= 1, (i, ny, nz)
    for ki, kw in enumerate(KWS):
        p = gpu.TsaParams.default(**kw)
        with gpu.overrides(align_tile=TILE):
            got = _run(gpu, trips, path, p)
        with gpu.overrides(align_mode=path, align_tile=TILE):
            sync = gpu.align_batch(trips, p)
        for i, ref in enumerate(_refs(ki)):
            assert _same(got[i], ref), (path, kw, i, got[i], ref)
            assert _same(got[i], sync[i]), (path, kw, i)


@pytest.mark.gpu
def test_gpu_async_mode_override_replaces_path(gpu):
    """A set align_mode holds: path = tiled under align_mode = grid queues the grid launches."""
    trips = list(_batch())
    with gpu.overrides(align_mode="grid", align_tile=TILE):
        before = gpu.kernel_launch_count()
        got = _run(gpu, trips, "tiled")
        # [resident] + max (nty+ntz-2) + max (nty+ntz-1): tiles 3x2 and 2x3
        assert gpu.kernel_launch_count() - before == 1 + 3 + 4
    assert all(_same(g, r) for g, r in zip(got, _refs(0)))


@pytest.mark.gpu
def test_gpu_async_natural_plan(gpu, orc):
    """Test 2: (8,65,64), the smallest triple that does not fit a workgroup, no override."""
    rng = np.random.default_rng(7200)
    t = ac.related(rng, 8, 65, 64)
    ref = orc.align(*t)
    assert gpu.describe_align_plan(1, 8, 64, 64).startswith("resident")
    with gpu.overrides(align_mode="tiled"):
        assert gpu.describe_align_plan(1, 8, 65, 64).startswith("tiled tile=33x32 tiles=2x2")
    sync = {"tiled": gpu.align_batch([t])[0], "strip": gpu.align_batch([t], lowmem=True)[0],
            "grid": gpu.align_batch([t], grid=True)[0]}
    for path in PATHS:
        got = _run(gpu, [t], path)[0]
        assert _same(got, ref), (path, got, ref)
        assert _same(got, sync[path]), path


@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS)
def test_gpu_async_layout(gpu, path):
    """Test 3: offsets[0] = 5; beyond n_moves no byte of a slot is written, in moves and in rows."""
    import torch
    trips = list(_batch())
    d = Dev(gpu, trips, base=5, tail=8, fill=0xEE)
    with gpu.overrides(align_tile=TILE):
        d.queue(path)
    d.queue_rows()
    torch.cuda.synchronize()
    got, nm = d.results(), d.d_nm.cpu().numpy()
    mv, rows = d.d_mv.cpu().numpy(), d.d_rows.cpu().numpy()
    for i, (t, ref) in enumerate(zip(trips, _refs(0))):
        assert _same(got[i], ref), i
        at, ln = int(d.offsets[3 * i]) - 5, sum(len(s) for s in t)
        assert 1 <= nm[i] <= ln
        assert (mv[at + nm[i]:at + ln] == 0xEE).all(), i
        for r in range(3):
            row = rows[3 * at + r * ln:3 * at + (r + 1) * ln]
            assert (row[:nm[i]] <= gpu.ROW_GAP).all() and (row[nm[i]:] == 0xEE).all(), (i, r)
        assert d.rows()[i] == gpu.render_alignment(*t, ref[1], ref[2]), i
    assert nm.sum() < d.total                      # some slot has unwritten bytes
    assert (mv[d.total:] == 0xEE).all() and (rows[3 * d.total:] == 0xEE).all()


@pytest.mark.gpu
def test_gpu_async_chunks_resident(gpu, orc):
    """Test 4: six resident triples; min_bytes runs six chunks, full_bytes one."""
    rng = np.random.default_rng(7300)
    trips = [ac.planted(rng, 7, 6, 5, 3) for _ in range(6)]
    refs = [orc.align(*t) for t in trips]
    lo, hi = gpu.align_workspace_size(_offsets([(7, 6, 5)] * 6))
    assert hi - lo == 5 * 4 * 6 * 11 * 5
    for ws, launches in ((lo, 6), (hi, 1), (lo + 2 * 4 * 6 * 11 * 5 + 100, 2)):
        before = gpu.kernel_launch_count()
        got = _run(gpu, trips, "tiled", ws_bytes=ws)
        assert gpu.kernel_launch_count() - before == launches, ws
        assert all(_same(g, r) for g, r in zip(got, refs)), ws
    before = gpu.kernel_launch_count()
    with pytest.raises(gpu.TsaError) as e:
        _run(gpu, trips, "tiled", ws_bytes=lo - 256)
    assert e.value.rc == gpu.TSA_ENOMEM and gpu.kernel_launch_count() == before


@pytest.mark.gpu
def test_gpu_async_chunks_grid(gpu):
    """Test 4 on the grid path: the two larger triples of the batch, min_bytes
    (a chunk each) against full_bytes (one chunk)."""
    trips = [_batch()[0], _batch()[2]]
    refs = [_refs(0)[0], _refs(0)[2]]
    with gpu.overrides(align_tile=TILE):
        lo, hi = gpu.align_workspace_size(_offsets([SHAPES[0], SHAPES[2]]), path="grid")
        assert lo < hi
        for ws, launches in ((lo, 2 * (3 + 4)), (hi, 3 + 4)):   # tiles 3x2 and 2x3: 3 forward + 4 backward
            before = gpu.kernel_launch_count()
            got = _run(gpu, trips, "grid", ws_bytes=ws)
            assert gpu.kernel_launch_count() - before == launches, ws
            assert all(_same(g, r) for g, r in zip(got, refs)), ws
        before = gpu.kernel_launch_count()
        with pytest.raises(gpu.TsaError) as e:
            _run(gpu, trips, "grid", ws_bytes=lo - 256)
        assert e.value.rc == gpu.TSA_ENOMEM and gpu.kernel_launch_count() == before


@pytest.mark.gpu
def test_gpu_async_stream_order(gpu, orc):
    """Test 5: two batches with their own workspaces and their rows, back to
    back on one non-default stream, one synchronise at the end."""
    import torch
    rng = np.random.default_rng(7400)
    one = list(_batch())
    two = [ac.planted(rng, 12, 9, 10, 4), ac.related(rng, 5, 13, 8), ac.planted(rng, 4, 4, 16, 2)]
    refs2 = [orc.align(*t) for t in two]
    d1, d2 = Dev(gpu, one), Dev(gpu, two)
    torch.cuda.synchronize()                        # the uploads were made on the default stream
    s = torch.cuda.Stream()
    with gpu.overrides(align_tile=TILE):
        d1.queue("strip", stream=s)
        d1.queue_rows(stream=s)
        d2.queue("grid", stream=s)
        d2.queue_rows(stream=s)
    s.synchronize()
    for d, refs in ((d1, _refs(0)), (d2, refs2)):
        got, rows = d.results(), d.rows()
        for i, (t, ref) in enumerate(zip(d.trips, refs)):
            assert _same(got[i], ref), i
            assert rows[i] == gpu.render_alignment(*t, ref[1], ref[2]), i


@pytest.mark.gpu
def test_gpu_rows(gpu, orc):
    """Test 6: 1, 64, 65 and 70 columns (the wave's block boundary inside a
    path), gaps in all three rows, N kept as 4; on the async call's moves and on
    the synchronous tsa_align_batch's, uploaded."""
    import torch
    rng = np.random.default_rng(7500)
    trips = [ac.identical(rng, L, L, L) for L in (1, 64, 65, 70)] + [ac.planted(rng, 40, 40, 40, run=4)]
    withn = [s.copy() for s in ac.identical(rng, 12, 12, 12)]
    for s in withn:
        s[5] = 4
    trips.append(tuple(withn))
    refs = [orc.align(*t) for t in trips]
    assert [len(r[2]) for r in refs[:4]] == [1, 64, 65, 70]
    want = [gpu.render_alignment(*t, r[1], r[2]) for t, r in zip(trips, refs)]
    assert all("-" in row for row in want[4]) and all(row[5] == "N" for row in want[5])
    d = Dev(gpu, trips)
    d.queue("tiled")
    d.queue_rows()
    torch.cuda.synchronize()
    assert all(_same(g, r) for g, r in zip(d.results(), refs))
    assert d.rows() == want
    # the rows of the synchronous entry point's output
    sync = gpu.align_batch(trips)
    mv, nm, st = np.zeros(d.total, np.uint8), np.zeros(d.n, np.int32), np.zeros(3 * d.n, np.int32)
    for i, (sc, start, moves) in enumerate(sync):
        at = int(d.offsets[3 * i])
        mv[at:at + len(moves)], nm[i], st[3 * i:3 * i + 3] = moves, len(moves), start
    e = Dev(gpu, trips)
    e.d_nm = torch.from_numpy(nm).cuda()
    up = (torch.from_numpy(mv).cuda(), e.d_nm, torch.from_numpy(st).cuda())
    e.queue_rows(moves=up)
    torch.cuda.synchronize()
    assert e.rows() == want


@pytest.mark.gpu
def test_gpu_rows_inconsistent_moves_stay_in_bounds(gpu):
    """Moves that consume more than the sequences hold, a move code out of
    range, n_moves beyond the slot and n_moves = 0: gaps where nothing can be
    read, nothing written outside the slot."""
    import torch
    trips = [(np.array([0, 1], np.uint8), np.array([2], np.uint8), np.array([3, 3, 1], np.uint8))] * 3
    d = Dev(gpu, trips, tail=4, fill=0xEE)
    mv = np.zeros(d.total + 4, np.uint8)            # M everywhere: A, B, C run out after 2, 1, 3 columns
    mv[3] = 9
    d.d_mv = torch.from_numpy(mv).cuda()
    d.d_nm = torch.tensor([6, 99, 0], dtype=torch.int32, device="cuda")
    d.queue_rows()
    torch.cuda.synchronize()
    rows = d.d_rows.cpu().numpy()
    assert "".join(gpu.ROW_LETTERS[v] for v in rows[:18]) == "AT----" "C-----" "GGT---"
    assert (rows[18:36] <= gpu.ROW_GAP).all()       # clamped to the slot
    assert (rows[36:] == 0xEE).all()


@pytest.mark.gpu
def test_gpu_align_batch_device(gpu):
    """Test 7: the torch convenience returns test 1's results, with and without rows."""
    import torch
    trips = list(_batch())
    packed, offs = gpu.pack_batch(trips)
    d_seqs = torch.from_numpy(packed).cuda()
    for path in PATHS:
        with gpu.overrides(align_tile=TILE):
            out = gpu.align_batch_device(d_seqs, offs, path=path)
            outr = gpu.align_batch_device(d_seqs, offs, path=path, rows=True, stream=torch.cuda.Stream())
        torch.cuda.synchronize()
        assert len(out) == 4 and len(outr) == 5 and all(t.is_cuda for t in outr)
        for o in (out, outr):
            sc, mv, nm, st = (t.cpu().numpy() for t in o[:4])
            for i, ref in enumerate(_refs(0)):
                at = int(offs[3 * i])
                assert _same((int(sc[i]), st[3 * i:3 * i + 3], mv[at:at + nm[i]]), ref), (path, i)
        rows, nm = outr[4].cpu().numpy(), outr[2].cpu().numpy()
        for i, (t, ref) in enumerate(zip(trips, _refs(0))):
            at, ln = 3 * int(offs[3 * i]), sum(len(s) for s in t)
            got = tuple("".join(gpu.ROW_LETTERS[v] for v in rows[at + r * ln:at + r * ln + nm[i]]) for r in range(3))
            assert got == gpu.render_alignment(*t, ref[1], ref[2]), (path, i)
