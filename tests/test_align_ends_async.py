"""tsa_align_ends_workspace_size and tsa_align_batch_ends_async: the end-free
traceback (TSA_END_FACE, TSA_END_ANY) under tsa_align_batch_async's calling
convention, and align_batch_ends_device over them. Results are those of
tsa_align_batch_ends / tsa_align_batch_grid_ends; the traceback kernels are
theirs, what is new is the device-side plumbing: the key slot offsets of a
chunk (align_meta_kernel), the end cells scattered to the caller's index
(align_finish_kernel) and the key slots in the workspace.

Reference, as in tests/test_align_ends.py: the oracle brute-forced over the
prefixes (ref_end / refs_of; tests/test_align_grid_ends.py's _ref_big where all
prefixes are too many), and output for output the synchronous entry point of the
same path in the same process. Every parity test first asserts on the reference
alone that the end lies off the corner in at least three quarters of its
triples and, where the reference can tell, that a maximum is tied.

The mixed batch is test_align_ends._small_batch(), 12 triples of 5..13 a side.
Under align_tile=5x7 every one of them is over capacity (the plan text says
so: none has lb <= 5 and lc <= 7), so it runs there as a batch of tiled or grid
triples alone, and again under align_tile=9x10, where the plan text shows four
resident triples between eight over-capacity ones: that is the batch the chunk,
dirty-workspace and layout tests use.

Without the feature every test below fails on the missing symbols."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _align_cases as ac  # noqa: E402
import test_align_async as ta  # noqa: E402
import test_align_ends as te  # noqa: E402
import test_align_grid_ends as tge  # noqa: E402

KWS, MODES, CASES = te.KWS, te.MODES, te.CASES
FAKE = ta.FAKE
SIZE_FN, FN = "tsa_align_ends_workspace_size", "tsa_align_batch_ends_async"
MIXED_TILE = "9x10"
PATH_ID = {"tiled": 0, "strip": 1, "grid": 2}


def _shapes(trips):
    return [tuple(len(s) for s in t) for t in trips]


def _up256(v):
    return (v + 255) & ~255


def _kinds(tsa, shapes, path, tile):
    """The first word of the plan text of every triple, and S = the tiles of the
    over-capacity ones, from the tiles=AxB text."""
    kinds, tiles = [], 0
    with tsa.overrides(align_mode=path, align_tile=tile):
        for s in shapes:
            txt = tsa.describe_align_plan(len(shapes), *s)
            kinds.append(txt.split()[0])
            m = re.search(r" tiles=(\d+)x(\d+) ", txt)
            if m:
                tiles += int(m.group(1)) * int(m.group(2))
    return kinds, tiles


# ---------------------------------------------------------------- CPU ------

def test_ends_async_exports(tsa):
    for name in (SIZE_FN, FN):
        assert name in tsa.EXPORTS and hasattr(tsa.lib(), name), name
    with open(os.path.join(ROOT, "include", "trialign.h")) as f:
        text = f.read()
    for name in (SIZE_FN, FN):
        assert re.search(rf"\bint {name}\(", text), name
    for name in ("align_ends_workspace_size", "align_batch_ends_async", "align_batch_ends_device"):
        assert callable(getattr(tsa, name)), name


def _raw(tsa, args):
    """tsa_align_batch_ends_async with integer addresses; returns the rc."""
    (d_seqs, d_off, h_off, n, p, path, end, d_sc, d_mv, d_nm, d_st, d_en, d_ws, ws) = args
    h = None if h_off is None else np.ascontiguousarray(h_off, np.int64)
    hp = None if h is None else h.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    pp = None if p is None else ctypes.byref(p)
    return getattr(tsa.lib(), FN)(d_seqs, d_off, hp, n, pp, path, end, d_sc, d_mv, d_nm, d_st, d_en, d_ws, ws, None)


def _size_rc(tsa, offs, n, path, end, p=None):
    p = p or tsa.TsaParams.default()
    offs = np.ascontiguousarray(offs, np.int64)
    lo, hi = ctypes.c_size_t(7), ctypes.c_size_t(7)
    return getattr(tsa.lib(), SIZE_FN)(offs.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), n, ctypes.byref(p), path,
                                       end, ctypes.byref(lo), ctypes.byref(hi))


def test_ends_async_argument_checks(tsa):
    """Validation comes before any device work, in the header's order: the fake
    addresses never reach a device, and the size function returns the same
    TSA_EINVALs."""
    p = tsa.TsaParams.default()
    offs = np.array([0, 3, 7, 12, 14, 15, 19], np.int64)
    names = ("d_seqs", "d_off", "h_off", "n", "p", "path", "end", "d_sc", "d_mv", "d_nm", "d_st", "d_en", "d_ws", "ws")
    before = tsa.kernel_launch_count()
    nodev = tsa.device_count() == 0  # with a device a valid call would use the fake addresses

    def rc(**kw):
        a = [FAKE, FAKE, offs, 2, p, 0, tsa.END_ANY, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 1 << 20]
        for k, v in kw.items():
            a[names.index(k)] = v
        return _raw(tsa, a)

    for end in (tsa.END_CORNER, tsa.END_FACE, tsa.END_ANY):
        for name in ("d_seqs", "d_off", "h_off", "p", "d_sc", "d_mv", "d_nm", "d_st", "d_en", "d_ws"):
            assert rc(end=end, **{name: None}) == tsa.TSA_EINVAL, (end, name)
        assert rc(end=end, d_ws=FAKE + 128) == tsa.TSA_EINVAL                       # not 256-byte aligned
        assert rc(end=end, path=3) == tsa.TSA_EINVAL and rc(end=end, path=-1) == tsa.TSA_EINVAL
        assert rc(end=end, n=-1) == tsa.TSA_EINVAL
        assert rc(end=end, h_off=np.array([0, 3, 3, 12, 14, 15, 19])) == tsa.TSA_EINVAL  # a length below 1
        assert rc(end=end, p=tsa.TsaParams.default(score_bits=3)) == tsa.TSA_EINVAL
        assert _size_rc(tsa, offs, 2, 3, end) == tsa.TSA_EINVAL
        for mode in ("resident", "plane"):
            with tsa.overrides(align_mode=mode):
                assert rc(end=end) == tsa.TSA_EINVAL, (end, mode)
                assert _size_rc(tsa, offs, 2, 0, end) == tsa.TSA_EINVAL
    for end in (3, -1):
        assert rc(end=end) == tsa.TSA_EINVAL
        assert rc(end=end, n=0) == tsa.TSA_EINVAL                                   # before the empty batch
        assert _size_rc(tsa, offs, 2, 0, end) == tsa.TSA_EINVAL
    for end in (tsa.END_FACE, tsa.END_ANY):
        assert rc(end=end, path=PATH_ID["strip"]) == tsa.TSA_EINVAL                 # no end search on the strips
        assert rc(end=end, path=PATH_ID["strip"], n=0) == tsa.TSA_EINVAL
        assert _size_rc(tsa, offs, 2, PATH_ID["strip"], end) == tsa.TSA_EINVAL
        with tsa.overrides(align_mode="strip"):
            for path in (0, 2):
                assert rc(end=end, path=path) == tsa.TSA_EINVAL
                assert _size_rc(tsa, offs, 2, path, end) == tsa.TSA_EINVAL
        with pytest.raises(tsa.TsaError) as e:
            tsa.align_ends_workspace_size(offs, path="strip", end=end)
        assert e.value.rc == tsa.TSA_EINVAL
        for mode in ("tiled", "grid"):                                              # these replace the path
            with tsa.overrides(align_mode=mode):
                assert _size_rc(tsa, offs, 2, 0, end) == tsa.TSA_OK
                if nodev:
                    assert rc(end=end) == tsa.TSA_ENODEV
    with pytest.raises(tsa.TsaError) as e:
        tsa.align_ends_workspace_size(offs, end="middle")
    assert e.value.rc == tsa.TSA_EINVAL
    for end in (tsa.END_CORNER, tsa.END_FACE, tsa.END_ANY):
        for path in (0, 2):
            assert rc(end=end, path=path, n=0) == tsa.TSA_OK
            assert _size_rc(tsa, offs, 0, path, end) == tsa.TSA_OK
    assert rc(end=tsa.END_CORNER, path=PATH_ID["strip"], n=0) == tsa.TSA_OK
    assert _size_rc(tsa, offs, 2, PATH_ID["strip"], tsa.END_CORNER) == tsa.TSA_OK   # corner + strip is accepted
    with tsa.overrides(align_mode="strip"):
        assert _size_rc(tsa, offs, 2, 0, tsa.END_CORNER) == tsa.TSA_OK
    if nodev:
        assert rc(end=tsa.END_CORNER, path=PATH_ID["strip"]) == tsa.TSA_ENODEV
        for end in (tsa.END_CORNER, tsa.END_FACE, tsa.END_ANY):
            for path in (0, 2):
                assert rc(end=end, path=path) == tsa.TSA_ENODEV
                assert rc(end=end, path=path, ws=0) == tsa.TSA_ENODEV              # before TSA_ENOMEM
    assert tsa.kernel_launch_count() == before


def test_ends_workspace_size_null_outputs(tsa):
    f = getattr(tsa.lib(), SIZE_FN)
    p = tsa.TsaParams.default()
    offs = np.array([0, 3, 7, 12], np.int64)
    op = offs.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    lo, hi = ctypes.c_size_t(7), ctypes.c_size_t(7)
    assert f(op, 1, ctypes.byref(p), 0, 2, None, ctypes.byref(hi)) == tsa.TSA_EINVAL
    assert f(op, 1, ctypes.byref(p), 0, 2, ctypes.byref(lo), None) == tsa.TSA_EINVAL
    assert f(None, 1, ctypes.byref(p), 0, 2, ctypes.byref(lo), ctypes.byref(hi)) == tsa.TSA_EINVAL
    assert f(op, 1, None, 0, 2, ctypes.byref(lo), ctypes.byref(hi)) == tsa.TSA_EINVAL
    assert f(op, 1, ctypes.byref(p), 0, 2, ctypes.byref(lo), ctypes.byref(hi)) == tsa.TSA_OK and lo.value > 0


def test_ends_workspace_relations(tsa):
    """A mixed batch under align_tile=5x7: the sizes are tsa_align_workspace_size's
    under corner (every path) and under face/any with tiled; under face/any with
    grid they exceed the grid sizes by exactly up256(8n) + up256(8S), S from the
    tiles=AxB text of the plan; min <= full, and both grow with the batch."""
    shapes = list(ta.SHAPES) + [(12, 17, 9), (5, 5, 8)]
    kinds, S = _kinds(tsa, shapes, "grid", "5x7")
    assert kinds.count("resident") >= 2 and kinds.count("grid") >= 2 and kinds[0] == "grid" and kinds[1] == "resident"
    assert S == 3 * 2 + 2 * 3 + 4 * 2 + 1 * 2                                       # (11,13) (6,15) (17,9) (5,8)
    prev = {}
    for k in range(1, len(shapes) + 1):
        offs = ta._offsets(shapes[:k], base=3)
        Sk = _kinds(tsa, shapes[:k], "grid", "5x7")[1]
        with tsa.overrides(align_tile="5x7"):
            for path in ("tiled", "strip", "grid"):
                assert tsa.align_ends_workspace_size(offs, path=path, end="corner") == \
                    tsa.align_workspace_size(offs, path=path), (k, path)
            for end in ("face", "any"):
                assert tsa.align_ends_workspace_size(offs, path="tiled", end=end) == \
                    tsa.align_workspace_size(offs, path="tiled"), (k, end)
                lo, hi = tsa.align_ends_workspace_size(offs, path="grid", end=end)
                glo, ghi = tsa.align_workspace_size(offs, path="grid")
                extra = _up256(8 * k) + _up256(8 * Sk)
                assert (lo - glo, hi - ghi) == (extra, extra), (k, end)
                assert lo <= hi and lo % 4 == 0
                plo, phi = prev.get(end, (0, 0))
                assert lo >= plo and hi >= phi and (k == 1 or hi > phi), (k, end)
                prev[end] = (lo, hi)
                with tsa.overrides(align_mode="grid"):                              # the override replaces the path
                    assert tsa.align_ends_workspace_size(offs, path="tiled", end=end) == (lo, hi)
    assert prev["any"][1] > prev["any"][0]
    # no over-capacity triple, no slots: the slot offsets alone
    offs = ta._offsets([(3, 4, 5), (6, 5, 7)])
    with tsa.overrides(align_tile="5x7"):
        assert tsa.align_ends_workspace_size(offs, path="grid", end="any")[0] - \
            tsa.align_workspace_size(offs, path="grid")[0] == 256


# ---------------------------------------------------------------- GPU ------

class EDev(ta.Dev):
    """ta.Dev with the end cells and tsa_align_batch_ends_async."""

    def __init__(self, tsa, trips, base=0, tail=0, fill=0):
        super().__init__(tsa, trips, base, tail, fill)
        self.d_en = self.torch.full((3 * self.n,), -7, dtype=self.torch.int32, device="cuda")

    def sizes(self, path, params=None, end="any"):
        return self.tsa.align_ends_workspace_size(self.offsets, params, path, end)

    def queue(self, path="tiled", end="any", params=None, ws_bytes=None, stream=None, ws=None):
        torch = self.torch
        if ws_bytes is None:
            ws_bytes = self.sizes(path, params, end)[1]
        self.ws = ws if ws is not None else torch.full((max(ws_bytes, 256),), 0xFF, dtype=torch.uint8, device="cuda")
        assert self.ws.numel() >= ws_bytes and self.ws.data_ptr() % 256 == 0
        s = (stream or torch.cuda.current_stream()).cuda_stream
        self.tsa.align_batch_ends_async(self.d_seqs.data_ptr(), self.d_off.data_ptr(), self.offsets,
                                        self.d_sc.data_ptr(), self.d_mv.data_ptr(), self.d_nm.data_ptr(),
                                        self.d_st.data_ptr(), self.d_en.data_ptr(), self.ws.data_ptr(), ws_bytes, s,
                                        params, path, end)

    def results(self):
        """After a synchronise: [(score, start, moves, end)] as align_batch_ends returns them."""
        en = self.d_en.cpu().numpy()
        return [r + (tuple(int(v) for v in en[3 * i:3 * i + 3]),) for i, r in enumerate(super().results())]


def _run(tsa, trips, path, end, params=None, ws_bytes=None, **ov):
    """One call under the overrides, every workspace byte 0xFF on entry:
    (results, counted launches)."""
    import torch
    d = EDev(tsa, trips)
    with tsa.overrides(**ov):
        before = tsa.kernel_launch_count()
        d.queue(path, end, params, ws_bytes)
        launches = tsa.kernel_launch_count() - before
    torch.cuda.synchronize()
    return d.results(), launches


def _sync(tsa, trips, path, end, params=None, **ov):
    """The synchronous entry point of the path: (results, counted launches)."""
    if path == "tiled":
        ov = dict(ov, align_mode="tiled") if "align_tile" in ov else ov
    with tsa.overrides(**ov):
        before = tsa.kernel_launch_count()
        got = tsa.align_batch_ends(trips, params, end=end, grid=(path == "grid"))
        return got, tsa.kernel_launch_count() - before


def _assert_same(gpu, trips, got, refs, params=None, rescore=True, what=None):
    assert len(got) == len(trips) == len(refs)
    for i, (t, g, r) in enumerate(zip(trips, got, refs)):
        assert te.same(g, r), (what, i, g[0], g[1], g[3], r[0], r[1], r[3])
        te.check_path(gpu, *t, g, params, rescore=rescore)


# id -> (path, case of test_align_ends.CASES, align_tile or None, what the plan text must show)
PARITY = {
    "tiled_all_over_5x7": ("tiled", "resident_k1", "5x7", {"tiled"}),
    "tiled_mixed_9x10": ("tiled", "resident_k1", MIXED_TILE, {"resident", "tiled"}),
    "tiled_k1": ("tiled", "tiled_k1_3x3", "5x7", {"tiled"}),
    "tiled_k2": ("tiled", "tiled_k2", "35x30", {"tiled"}),
    "tiled_k3": ("tiled", "tiled_k3", "48x44", {"tiled"}),
    "resident_k2": ("tiled", "resident_k2", None, {"resident"}),
    "resident_k4": ("tiled", "resident_k4", None, {"resident"}),
    "grid_all_over_5x7": ("grid", "resident_k1", "5x7", {"grid"}),
    "grid_mixed_9x10": ("grid", "resident_k1", MIXED_TILE, {"resident", "grid"}),
    "grid_seed114_5x7": ("grid", "tiled_k1_3x3", "5x7", {"grid"}),
}
PARITY_PARAMS = [(pid, k) for pid, (_, name, _, _) in PARITY.items() for k in range(len(CASES[name][2]))]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("pid,k", PARITY_PARAMS)
def test_gpu_ends_async_parity(gpu, orc, pid, k, mode):
    """Every END instantiation the call reaches, both modes, every parameter set
    of the case: the oracle's result on the prefixes, the synchronous entry
    point's output for output, and its counted launches."""
    path, name, tile, want_kinds = PARITY[pid]
    _, trips, kws = CASES[name]
    refs = te.refs_of(orc, name, k, mode)                  # the end off the corner, a tied maximum
    ov = dict(align_tile=tile) if tile else {}
    kinds = set(_kinds(gpu, _shapes(trips), path, tile)[0]) if tile else \
        {gpu.describe_align_plan(len(trips), *s).split()[0] for s in _shapes(trips)}
    assert kinds == want_kinds, (pid, kinds)
    p = gpu.TsaParams.default(**kws[k])
    got, launches = _run(gpu, trips, path, mode, p, **ov)
    sync, sync_launches = _sync(gpu, trips, path, mode, p, **ov)
    _assert_same(gpu, trips, got, refs, p, rescore=kws[k].get("score_bits", 12) not in (4, 6), what=(pid, kws[k], mode))
    for g, w in zip(got, sync):
        assert te.same(g, w), (pid, kws[k], mode)
    assert launches == sync_launches >= 1
    if pid == "grid_seed114_5x7":
        assert launches == 5 + 5
        want = {(0, "face"): ((5, 11, 14), (2, 2)), (0, "any"): ((4, 9, 12), (2, 1)),    # the last tile, early tiles
                (5, "face"): ((2, 11, 4), (2, 0)), (5, "any"): ((2, 2, 3), (0, 0))}.get((k, mode))
        if want:
            assert (refs[0][3], tge._tile_of(refs[0][3], 4, 6)) == want


@pytest.mark.gpu
def test_gpu_ends_async_grid_corner_write_trap(gpu, orc):
    """Uniform seed 184 (13, 11, 16) under 5x7, face: the end (13, 11, 14) lies in
    the last tile with x1 == la, so backward launch 0 sweeps the corner too; the
    corner's score must not replace the end's. One triple, so the condition on
    the reference is the end off the corner; its maximum is not tied."""
    a, b, c = tge._uniform(184, 13, 11, 16)
    ref, _ = te.ref_end(orc, a, b, c, {}, "face")
    assert ref[3] == (13, 11, 14) and tge._tile_of(ref[3], 4, 6) == (2, 2) and ref[0] != orc.score(a, b, c)
    got, launches = _run(gpu, [(a, b, c)], "grid", "face", align_tile="5x7")
    sync, _ = _sync(gpu, [(a, b, c)], "grid", "face", align_tile="5x7")
    assert launches == 5 + 5
    _assert_same(gpu, [(a, b, c)], got, [ref])
    assert te.same(got[0], sync[0])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["k2", "k3_2x1"])
def test_gpu_ends_async_grid_two_and_three_positions_a_thread(gpu, orc, name, mode):
    """The planted cores of tests/test_align_grid_ends.py: (12, 70, 60) under 35x30
    (K = 2, 2 x 2 tiles) and (12, 96, 44) under 48x44 (K = 3, 2 x 1 tiles)."""
    shape, offb, offc, tile, grid, pos, end, path_tiles, seams, corner = tge.PLANTED[name]
    a, b, c = tge._planted(7, *shape, offb, offc)
    TY, TZ, nty, ntz = tge._geom(shape[1], shape[2], *(int(v) for v in tile.split("x")))
    assert (nty, ntz) == grid and TY * TZ == pos
    ref, _ = tge._ref_big(orc, a, b, c, {}, mode)
    assert ref[0] == 36 and ref[3] == end != shape and orc.score(a, b, c) == corner
    got, launches = _run(gpu, [(a, b, c)], "grid", mode, align_tile=tile)
    sync, _ = _sync(gpu, [(a, b, c)], "grid", mode, align_tile=tile)
    assert launches == 2 * (nty + ntz - 1)
    _assert_same(gpu, [(a, b, c)], got, [ref], what=(name, mode))
    assert te.same(got[0], sync[0])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_gpu_ends_async_grid_every_cell_a_tile(gpu, orc, mode):
    """identical (5, 6, 6) under 1x1: 36 tiles, 36 slots, 11 + 11 launches."""
    a, b, c = ac.identical(np.random.default_rng(900), 5, 6, 6)
    ref, _ = te.ref_end(orc, a, b, c, {}, mode)
    assert tge._tile_of(ref[3], 1, 1) != (5, 5)
    assert _kinds(gpu, [(5, 6, 6)], "grid", "1x1") == (["grid"], 36)
    d = EDev(gpu, [(a, b, c)])
    with gpu.overrides(align_tile="1x1"):
        assert d.sizes("grid", None, mode)[0] - gpu.align_workspace_size(d.offsets, path="grid")[0] == 256 + _up256(8 * 36)
    got, launches = _run(gpu, [(a, b, c)], "grid", mode, align_tile="1x1")
    sync, _ = _sync(gpu, [(a, b, c)], "grid", mode, align_tile="1x1")
    assert launches == 11 + 11
    _assert_same(gpu, [(a, b, c)], got, [ref])
    assert te.same(got[0], sync[0])


def _need(shape, path, tymax, tzmax):
    la, lb, lc = shape
    if lb <= tymax and lc <= tzmax:
        return tge._cube_bytes(la, lb, lc)
    if path == "grid":
        return sum(tge._grid_need(la, lb, lc, tymax, tzmax))
    TY = tge._geom(lb, lc, tymax, tzmax)[0]
    return tge._cube_bytes(la, lb, lc) + 32 * la * (lc + 1) + 32 * la * TY       # include/trialign.h: tiled


def _chunk_launches(shapes, path, budget, tymax, tzmax):
    """(sum over the chunks of the header's rule, chunks): [resident] + [tiled],
    or [resident] + 2 * max (nty+ntz-1) on the grid path with a free end."""
    total, chunks, i = 0, 0, 0
    while i < len(shapes):
        used, res, diag = 0, False, []
        while i < len(shapes):
            need = _need(shapes[i], path, tymax, tzmax)
            assert need <= budget
            if used + need > budget:
                break
            used += need
            if shapes[i][1] > tymax or shapes[i][2] > tzmax:
                g = tge._geom(shapes[i][1], shapes[i][2], tymax, tzmax)
                diag.append(g[2] + g[3] - 1)
            else:
                res = True
            i += 1
        total += int(res) + ((2 * max(diag) if path == "grid" else 1) if diag else 0)
        chunks += 1
    return total, chunks


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("path,tile", [("grid", MIXED_TILE), ("tiled", MIXED_TILE), ("tiled", None)])
def test_gpu_ends_async_chunks(gpu, orc, path, tile, mode):
    """The mixed batch on the grid and the tiled path and the all-resident batch
    with workspace_bytes = min_bytes: a chunk budget of the largest need, so
    several chunks; results equal the full_bytes run, and the counted launches
    are the per-chunk rule summed over the chunks of the host plan."""
    trips = CASES["resident_k1"][1]
    shapes = _shapes(trips)
    refs = te.refs_of(orc, "resident_k1", 0, mode)
    ty, tz = (int(v) for v in tile.split("x")) if tile else (1 << 20, 1 << 20)
    ov = dict(align_tile=tile) if tile else {}
    if tile:
        kinds = _kinds(gpu, shapes, path, tile)[0]
        assert kinds.count("resident") == 4 and kinds.count(path) == 8
    d = EDev(gpu, trips)
    with gpu.overrides(**ov):
        lo, hi = d.sizes(path, None, mode)
    needs = [_need(s, path, ty, tz) for s in shapes]
    assert hi - lo == sum(needs) - max(needs)               # the fixed part, then one chunk's needs
    want_lo, chunks = _chunk_launches(shapes, path, max(needs), ty, tz)
    want_hi, one = _chunk_launches(shapes, path, sum(needs), ty, tz)
    assert chunks >= 3 and one == 1
    full, launches_hi = _run(gpu, trips, path, mode, ws_bytes=hi, **ov)
    small, launches_lo = _run(gpu, trips, path, mode, ws_bytes=lo, **ov)
    assert (launches_lo, launches_hi) == (want_lo, want_hi)
    _assert_same(gpu, trips, full, refs, what=(path, mode, "full"))
    _assert_same(gpu, trips, small, refs, what=(path, mode, "min"))
    before = gpu.kernel_launch_count()
    with pytest.raises(gpu.TsaError) as e:
        _run(gpu, trips, path, mode, ws_bytes=lo - 256, **ov)
    assert e.value.rc == gpu.TSA_ENOMEM and gpu.kernel_launch_count() == before


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("path", ["grid", "tiled"])
def test_gpu_ends_async_dirty_workspace_and_stream_order(gpu, orc, path, mode):
    """One workspace of 0xFF bytes; the mixed batch, the (13, 11, 16) triple and
    the mixed batch again (over the first call's slots and records) back to back
    on one non-default stream, no synchronisation between them."""
    import torch
    one, two = CASES["resident_k1"][1], CASES["tiled_k1_3x3"][1]
    refs1, refs2 = te.refs_of(orc, "resident_k1", 0, mode), te.refs_of(orc, "tiled_k1_3x3", 0, mode)
    d1, d2, d3 = EDev(gpu, one), EDev(gpu, two), EDev(gpu, one)
    with gpu.overrides(align_tile=MIXED_TILE):
        size = max(d.sizes(path, None, mode)[1] for d in (d1, d2))
        ws = torch.full((size,), 0xFF, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()                            # the uploads were made on the default stream
        s = torch.cuda.Stream()
        for d in (d1, d2, d3):
            d.queue(path, mode, ws_bytes=size, stream=s, ws=ws)
    s.synchronize()
    _assert_same(gpu, one, d1.results(), refs1, what=(path, mode, 1))
    _assert_same(gpu, two, d2.results(), refs2, what=(path, mode, 2))
    _assert_same(gpu, one, d3.results(), refs1, what=(path, mode, 3))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("path", ["grid", "tiled"])
def test_gpu_ends_async_layout(gpu, orc, path, mode):
    """offsets[0] = 5; d_moves prefilled with 0xEE: beyond n_moves no byte of a
    slot is written, nor any beyond the batch."""
    import torch
    trips = CASES["resident_k1"][1]
    refs = te.refs_of(orc, "resident_k1", 0, mode)
    d = EDev(gpu, trips, base=5, tail=8, fill=0xEE)
    with gpu.overrides(align_tile=MIXED_TILE):
        d.queue(path, mode)
    torch.cuda.synchronize()
    got, nm, mv = d.results(), d.d_nm.cpu().numpy(), d.d_mv.cpu().numpy()
    _assert_same(gpu, trips, got, refs, what=(path, mode))
    for i, t in enumerate(trips):
        at, ln = int(d.offsets[3 * i]) - 5, sum(len(s) for s in t)
        assert 1 <= nm[i] == len(refs[i][2]) <= ln
        assert (mv[at + nm[i]:at + ln] == 0xEE).all(), i
    assert nm.sum() < d.total and (mv[d.total:] == 0xEE).all()


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["tiled", "strip", "grid"])
def test_gpu_ends_async_corner_is_align_batch_async(gpu, path):
    """TSA_END_CORNER: tsa_align_batch_async's outputs and counted launches on
    every path, strip included, and d_ends = the lengths."""
    import torch
    trips = list(ta._batch())
    with gpu.overrides(align_tile=ta.TILE):
        before = gpu.kernel_launch_count()
        want = ta._run(gpu, trips, path)
        mid = gpu.kernel_launch_count()
        got, launches = _run(gpu, trips, path, "corner")
    torch.cuda.synchronize()
    assert launches == mid - before >= 1
    for t, g, w, r in zip(trips, got, want, ta._refs(0)):
        assert ta._same(g, w) and ta._same(g, r), path
        assert g[3] == tuple(len(s) for s in t)


@pytest.mark.gpu
def test_gpu_ends_async_mode_override_replaces_path(gpu, orc):
    """A set align_mode holds: path = tiled under align_mode = grid queues the grid END launches."""
    trips = CASES["tiled_k1_3x3"][1]
    refs = te.refs_of(orc, "tiled_k1_3x3", 0, "any")
    got, launches = _run(gpu, trips, "tiled", "any", align_mode="grid", align_tile="5x7")
    assert launches == 5 + 5                                # 3 x 3 tiles: 5 forward + 5 backward
    _assert_same(gpu, trips, got, refs)
    got, launches = _run(gpu, trips, "grid", "any", align_mode="tiled", align_tile="5x7")
    assert launches == 1
    _assert_same(gpu, trips, got, refs)


def _rows_text(tsa, rows, offsets, trips, nm):
    out = []
    for i, t in enumerate(trips):
        at, ln = 3 * int(offsets[3 * i] - offsets[0]), sum(len(s) for s in t)
        out.append(tuple("".join(tsa.ROW_LETTERS[v] if v < 6 else "?" for v in rows[at + r * ln:at + r * ln + int(nm[i])])
                         for r in range(3)))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_gpu_ends_async_rows(gpu, orc, mode):
    """tsa_align_rows_async, queued behind the call, renders the prefixes'
    alignment: n_moves and starts define the columns."""
    import torch
    trips = CASES["resident_k1"][1]
    refs = te.refs_of(orc, "resident_k1", 0, mode)
    d = EDev(gpu, trips)
    with gpu.overrides(align_tile=MIXED_TILE):
        d.queue("grid", mode)
    d.queue_rows()
    torch.cuda.synchronize()
    _assert_same(gpu, trips, d.results(), refs)
    for i, ((a, b, c), r) in enumerate(zip(trips, refs)):
        x1, y1, z1 = r[3]
        assert d.rows()[i] == gpu.render_alignment(a[:x1], b[:y1], c[:z1], r[1], r[2]), i


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["tiled", "grid"])
def test_gpu_align_batch_ends_device(gpu, orc, path):
    """The torch convenience: the mixed batch, with and without rows, on a stream of its own."""
    import torch
    trips = CASES["resident_k1"][1]
    refs = te.refs_of(orc, "resident_k1", 0, "any")
    packed, offs = gpu.pack_batch(trips)
    d_seqs = torch.from_numpy(packed).cuda()
    with gpu.overrides(align_tile=MIXED_TILE):
        out = gpu.align_batch_ends_device(d_seqs, offs, end="any", path=path)
        torch.cuda.synchronize()
        outr = gpu.align_batch_ends_device(d_seqs, offs, end="any", path=path, rows=True, stream=torch.cuda.Stream())
    torch.cuda.synchronize()
    assert len(out) == 5 and len(outr) == 6 and all(t.is_cuda for t in outr)
    for o in (out, outr):
        sc, mv, nm, st, en = (t.cpu().numpy() for t in o[:5])
        for i, r in enumerate(refs):
            at = int(offs[3 * i])
            assert te.same((int(sc[i]), st[3 * i:3 * i + 3], mv[at:at + nm[i]], en[3 * i:3 * i + 3]), r), (path, i)
    rows = _rows_text(gpu, outr[5].cpu().numpy(), offs, trips, outr[2].cpu().numpy())
    for i, ((a, b, c), r) in enumerate(zip(trips, refs)):
        x1, y1, z1 = r[3]
        assert rows[i] == gpu.render_alignment(a[:x1], b[:y1], c[:z1], r[1], r[2]), (path, i)
    corner = gpu.align_batch_ends_device(d_seqs, offs, end="corner", path="strip")
    torch.cuda.synchronize()
    assert corner[4].cpu().numpy().reshape(-1, 3).tolist() == [list(s) for s in _shapes(trips)]
