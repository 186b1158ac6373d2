"""tsa_score_batch_ends_lap: end-free scores and end cells on the lap schedule.

The semantics are tsa_align_batch_ends' (tests/test_score_ends.py): the best
MAX7 over the candidate cells of the mode, at the cell with the smallest x,
then y, then z. References:
  any   oracle.best_range(a, b, c): bmax and at_max;
  face  the prefix brute force on the small inputs, the recorded references
        (tests/golden/score_ends_face.json) on the planted cubes;
  both  on the GPU also tsa_align_batch_ends, the literal traceback kernels.
The certified path uses the recipes of tests/_checked_cases.py: a peak of
exactly hi (certified) or hi + 1 (refused) at one chosen cell of (72, 50, 270)
in 8-bit words.
"""
import ctypes
import functools
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG_DIR, ROOT
import _checked_cases as cc
from test_score_ends import (EMU_INPUTS, MODES, PLANTED, RAGGED_MAX, SHAPES, SMALL, SMALL_ANY, _repeat, any_ref,
                             emu_face_ref, face_ref, planted, planted_face_ref, planted_name, ragged_batch, small_ref)

NEW = ("tsa_score_batch_ends_lap", "tsa_score_ends_workspace_size_lap", "tsa_score_batch_ends_async_lap",
       "tsa_describe_score_ends_plan_lap")
BUILT = tuple((m, nw) for m in (1, 2) for nw in (4, 8))     # the END instantiations (no M = 4)
# a small triple the lap schedule takes: 3 laps at NW = 4, 2 tiles at M = 1
LAPPED = ([0, 1, 2, 3], [1, 2] * 10, [2, 3] * 35)


def _emu():
    tools = os.path.join(ROOT, "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import lap_emu
    return lap_emu


def _plan(text):
    """The plan text without the overrides' suffix."""
    return text.split(" overrides=")[0]


def _kv(text):
    return dict(t.split("=", 1) for t in _plan(text).split() if "=" in t)


# ---- CPU: the interface ---------------------------------------------------------------

def test_exports(tsa):
    for name in NEW:
        assert name in tsa.EXPORTS and hasattr(tsa.lib(), name), name
    with open(os.path.join(ROOT, "include", "trialign.h")) as f:
        header = f.read()
    for name in NEW:
        assert f"int {name}(" in header


def _raw(tsa, seqs, offsets, n, p, end_mode, null=None):
    u8, i32, i64 = (ctypes.POINTER(t) for t in (ctypes.c_uint8, ctypes.c_int32, ctypes.c_int64))
    seqs = np.ascontiguousarray(seqs, np.uint8)
    offsets = np.ascontiguousarray(offsets, np.int64)
    m = max(abs(n), 1)
    out = dict(scores=np.zeros(m, np.int32), ends=np.zeros(3 * m, np.int32))
    arg = lambda k: None if k == null else out[k].ctypes.data_as(i32)
    return tsa.lib().tsa_score_batch_ends_lap(seqs.ctypes.data_as(u8), offsets.ctypes.data_as(i64), n,
                                              ctypes.byref(p), end_mode, arg("scores"), arg("ends"), 0)


def test_argument_errors(tsa):
    """TSA_EINVAL, TSA_OK for n = 0, then TSA_ERANGE, then TSA_ENODEV, all before any device work."""
    p = tsa.TsaParams.default()
    seqs, offs = tsa.pack_batch([LAPPED, LAPPED])
    tiny = tsa.pack_batch([([0, 1], [1, 2], [2, 3])])
    beyond = tsa.TSA_OK if tsa.device_count() > 0 else tsa.TSA_ENODEV
    for mode in (0, 1, 2):
        for null in ("scores", "ends"):
            assert _raw(tsa, seqs, offs, 2, p, mode, null=null) == tsa.TSA_EINVAL, (mode, null)
        assert _raw(tsa, seqs, offs, -1, p, mode) == tsa.TSA_EINVAL
        assert _raw(tsa, np.zeros(6, np.uint8), np.array([0, 3, 2, 6], np.int64), 1, p, mode) == tsa.TSA_EINVAL
        bad = seqs.copy()
        bad[1] = 9
        assert _raw(tsa, bad, offs, 2, p, mode) == tsa.TSA_EINVAL
        assert _raw(tsa, seqs, offs, 2, tsa.TsaParams.default(score_bits=3), mode) == tsa.TSA_EINVAL
        assert _raw(tsa, np.zeros(1, np.uint8), np.zeros(1, np.int64), 0, p, mode) == tsa.TSA_OK     # n = 0
        assert _raw(tsa, seqs, offs, 2, p, mode) == beyond                                        # admitted
    for mode in (3, -1):
        assert _raw(tsa, seqs, offs, 2, p, mode) == tsa.TSA_EINVAL
        assert _raw(tsa, seqs, offs, 2, p, mode, null="ends") == tsa.TSA_EINVAL
    lit = tsa.TsaParams.default(gap_open=1, gap_extend=2)
    wide0 = tsa.TsaParams.default(score_bits=0, match=1000, mismatch=-1000)
    for mode in (1, 2):
        assert _raw(tsa, seqs, offs, 2, lit, mode) == tsa.TSA_ERANGE          # literal-only parameters
        assert _raw(tsa, seqs, offs, 2, wide0, mode) == tsa.TSA_ERANGE        # no wrap, but beyond int16
        assert _raw(tsa, *tiny, 1, p, mode) == tsa.TSA_ERANGE                 # one workgroup: no lap plan
        with tsa.overrides(pencil_mode="helix"):
            assert _raw(tsa, seqs, offs, 2, p, mode) == tsa.TSA_EINVAL
            # an argument error like the others: before the n = 0 return
            assert _raw(tsa, np.zeros(1, np.uint8), np.zeros(1, np.int64), 0, p, mode) == tsa.TSA_EINVAL
            assert _raw(tsa, np.zeros(1, np.uint8), np.zeros(1, np.int64), 0, p, 0) == tsa.TSA_OK   # corner: the score plan's
        with tsa.overrides(pencil_mode="lap"):
            assert _raw(tsa, seqs, offs, 2, p, mode) == beyond
        with tsa.overrides(lap_m=4):                                          # no M = 4 end search
            assert _raw(tsa, seqs, offs, 2, p, mode) == tsa.TSA_ERANGE
    for end in ("middle", 3, None):
        with pytest.raises(tsa.TsaError) as e:
            tsa.score_batch_ends([LAPPED], end=end, kernel="lap")
        assert e.value.rc == tsa.TSA_EINVAL
    assert tsa.score_batch_ends([], end="face", kernel="lap") == []


def test_admission(tsa):
    d = lambda *a, **kw: tsa.describe_score_ends_plan(*a, kernel="lap", **kw)
    p8, p12 = tsa.TsaParams.default(score_bits=cc.BITS), tsa.TsaParams.default()
    for mode in MODES:
        # checkable, not exact: the certificate runs
        text = d(1, *cc.SHAPE, p8, end=mode)
        assert text.startswith("pencil lap i16 rtl M=") and text.endswith(f" checked ends={mode}"), text
        # exact a priori: no certificate; LC = 513, where the helix families stop
        text = d(1, 64, 64, 513, p12, end=mode)
        assert text.startswith("pencil lap i16 rtl M=") and text.endswith(f" ends={mode}") and "checked" not in text
        assert int(_kv(text)["M"]) <= 2
        # the RTL's 1024^3 in 12-bit words
        text = d(1, 1024, 1024, 1024, p12, end=mode)
        assert text.startswith("pencil lap i16 rtl M=") and text.endswith(f" checked ends={mode}"), text
        for kw in (dict(gap_open=1, gap_extend=2), dict(score_bits=0, match=1000, mismatch=-1000)):
            with pytest.raises(tsa.TsaError) as e:
                d(1, *cc.SHAPE, tsa.TsaParams.default(**kw), end=mode)
            assert e.value.rc == tsa.TSA_ERANGE, kw
            with pytest.raises(tsa.TsaError) as e:
                tsa.score_ends_workspace_size(1, *cc.SHAPE, tsa.TsaParams.default(**kw), end=mode, kernel="lap")
            assert e.value.rc == tsa.TSA_ERANGE, kw
        with tsa.overrides(pencil_mode="helix"):
            with pytest.raises(tsa.TsaError) as e:
                d(1, *cc.SHAPE, p8, end=mode)
            assert e.value.rc == tsa.TSA_EINVAL
    assert d(3, *cc.SHAPE, p8, end="corner") == tsa.describe_plan(3, *cc.SHAPE, p8)
    # the sibling families keep refusing: TSA_KERNEL_CHECKED, and AUTO beyond LC = 256
    for kernel, shape in (("checked", (64, 64, 64)), ("auto", (64, 64, 257)), ("auto", (64, 64, 513))):
        with pytest.raises(tsa.TsaError) as e:
            tsa.describe_score_ends_plan(1, *shape, end="any", kernel=kernel)
        assert e.value.rc == tsa.TSA_ERANGE


@pytest.mark.parametrize("m,nw", BUILT)
def test_plan_text_and_workspace_against_the_checked_lap(tsa, m, nw):
    """Under a forced geometry the plan is the checked lap plan of that
    geometry (the END kernels hold as many workgroups per CU as the checked
    ones), its text with the end mode in place of the estimate, its workspace
    plus 8 bytes per compute wave of every logical workgroup of a launch."""
    p8 = tsa.TsaParams.default(score_bits=cc.BITS)
    for n, shape in ((1, cc.SHAPE), (cc.BATCH_N, cc.SHAPE), (cc.BATCH_N, (cc.BATCH_LA, cc.BATCH_LB, 128))):
        with tsa.overrides(lap_m=m, lap_nw=nw):
            chk = tsa.describe_plan(n, *shape, p8, "checked", sync=False)
            base = tsa.workspace_size(n, *shape, p8, "checked")
            for mode in MODES:
                text = tsa.describe_score_ends_plan(n, *shape, p8, end=mode, kernel="lap")
                assert text.split(" ends=")[0] == chk.split(" est=")[0] and _plan(text).endswith(f" ends={mode}"), \
                    (text, chk)
                kv = _kv(text)
                assert (int(kv["M"]), int(kv["NW"])) == (m, nw)
                per_launch = int(kv.get("chunk", n))
                keys = 8 * per_launch * int(kv["laps"]) * int(kv["tiles"]) * nw
                assert tsa.score_ends_workspace_size(n, *shape, p8, end=mode, kernel="lap") == \
                    base + (keys + 255) // 256 * 256
    assert tsa.score_ends_workspace_size(3, *cc.SHAPE, p8, end="corner", kernel="lap") == \
        tsa.workspace_size(3, *cc.SHAPE, p8, "checked")


def test_existing_sizes_and_plans_are_the_parent_s(tsa):
    """What the size and describe functions returned before this family was
    added: 54 results of the parent commit's library, recorded on a host
    without a device (tests/golden/score_ends_lap_parent.json).

    Without a device every record is compared (32 of them plan a lap grid).
    With a device the lap plans follow its occupancy query instead of the
    host model, so every record that planned a lap grid then, or plans one
    now, is SKIPPED there and only the helix and literal entries are compared;
    `compared >= 6` keeps the test from passing empty."""
    with open(os.path.join(ROOT, "tests", "golden", "score_ends_lap_parent.json")) as f:
        rec = json.load(f)
    assert len(rec) >= 12
    dev = tsa.device_count() > 0
    compared = 0
    for r in rec:
        p = tsa.TsaParams.default(**r["params"])
        with tsa.overrides(**r["overrides"]):
            if r["fn"] == "describe_plan":
                got = tsa.describe_plan(r["n"], *r["shape"], p, r["kernel"], sync=r["sync"])
            elif r["fn"] == "workspace_size":
                got = tsa.workspace_size(r["n"], *r["shape"], p, r["kernel"])
            elif r["fn"] == "score_ends_workspace_size":
                got = tsa.score_ends_workspace_size(r["n"], *r["shape"], p, end=r["end"], kernel=r["kernel"])
            else:
                got = tsa.describe_score_ends_plan(r["n"], *r["shape"], p, end=r["end"], kernel=r["kernel"])
        if dev:     # a lap plan then, or now: it follows the device's occupancy
            k = r["kernel"] if r["kernel"] in ("auto", "plane", "pencil", "checked") else "auto"
            with tsa.overrides(**r["overrides"]):
                lap_now = any(" lap" in tsa.describe_plan(r["n"], *r["shape"], p, k, sync=sy) for sy in (False, True))
            if r["lap"] or lap_now:
                continue
        compared += 1
        assert got == r["want"], r
    assert compared >= 6


# ---- CPU: the kernel table ---------------------------------------------------------------

@pytest.fixture(scope="module")
def meta(tsa):
    sys.path.insert(0, os.path.join(PKG_DIR, "tools"))
    import kernel_meta
    objs = [o for o in sorted(glob.glob(os.path.join(PKG_DIR, "build", "*.o"))) if not o.endswith("kernel_meta.o")]
    if not objs:
        pytest.skip("no build objects (prebuilt library only)")
    return kernel_meta.object_meta_all(objs)


def test_end_kernels_are_listed_without_scratch(tsa, meta):
    from test_kernel_meta import sgpr_waves, vgpr_waves
    fn = getattr(tsa.lib(), "_ZN3tsa27lap_ends_simd_blocks_per_cuEiib")
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_bool]
    for m, nw in BUILT:
        for sop in (0, 1):
            rows = [v for k, v in meta.items() if k.startswith(f"_ZN3tsa15lap_ends_kernelILi{m}ELi{nw}ELb{sop}EE")]
            assert len(rows) == 1, (m, nw, sop)
            assert rows[0].get("scratch", 0) == 0, (m, nw, sop, rows[0])
            want = min(sgpr_waves(rows[0]["sgpr"]), vgpr_waves(rows[0]["vgpr"] + rows[0].get("agpr", 0))) // \
                ((nw + 1 + 3) // 4)
            assert fn(m, nw, bool(sop)) == want and want >= 1, (m, nw, sop)
    assert fn(4, 4, False) == 0 and fn(4, 8, True) == 0      # not instantiated
    assert not [k for k in meta if "lap_ends_kernelILi4E" in k]
    red = [v for k, v in meta.items() if k.startswith("_ZN3tsa15lap_ends_reduceE")]
    assert len(red) == 1 and red[0].get("scratch", 0) == 0


# ---- CPU: the kernel's fold, replayed (tools/lap_emu.py) ---------------------------------

EMU_GEOMETRIES = [(m, nw) for m in (1, 2) for nw in (2, 4)]


def test_key_orders_by_score_then_x_y_z():
    e = _emu()
    k = lambda s, x, y, z: e.end_key64(e.end_key(s, x - 1), y - 1, z - 1)
    assert k(5, 9, 9, 9) > k(4, 1, 1, 1) and k(-3, 9, 9, 9) > k(-4, 1, 1, 1) and k(0, 1, 1, 1) > k(-1, 1, 1, 1)
    assert k(5, 2, 9, 9) > k(5, 3, 1, 1) and k(5, 2, 3, 9) > k(5, 2, 4, 1) and k(5, 2, 3, 4) > k(5, 2, 3, 5)
    for s, cell in ((-32768, (1, 1, 1)), (32767, (4096, 4096, 1024)), (-1, (72, 50, 270))):
        assert e.end_decode(k(s, *cell)) == (s, cell) and e.end_key(s, cell[0] - 1) != 0


@pytest.mark.parametrize("m,nw", EMU_GEOMETRIES)
@pytest.mark.parametrize("name", list(EMU_INPUTS))
def test_replay_matches_the_references(orc, name, m, nw):
    """Mask, key, per-register fold, wave and triple reduction as the kernel
    does them, with garbage in best of every cell that is no candidate."""
    t = EMU_INPUTS[name]
    got_any, got_face = _emu().emulate(*t, M=m, NW=nw, end=("any", "face"))
    assert got_any == any_ref(orc, t), (name, m, nw)
    planted_face_ref(planted_name(SHAPES[0], SHAPES[0]))   # the recorded file first: the cache loads it only while empty
    assert got_face == emu_face_ref(orc, name), (name, m, nw)


@pytest.mark.parametrize("m,nw", EMU_GEOMETRIES)
@pytest.mark.parametrize("name", list(SMALL))
def test_replay_in_a_ragged_batch(orc, name, m, nw):
    """A short triple inside the geometry of a batch's maxima: the slots of the
    laps and tiles it does not have keep the neutral fill."""
    assert RAGGED_MAX == (140, 19, 140)
    t = SMALL[name]
    got_any, got_face = _emu().emulate(*t, M=m, NW=nw, end=("any", "face"), max_lens=RAGGED_MAX)
    assert got_any == any_ref(orc, t) and got_face == face_ref(orc, t), (name, m, nw)


# ---- GPU ---------------------------------------------------------------------------------

def _async(gpu, trips, p, mode, dims=None, fill=0xFF):
    """tsa_score_batch_ends_async_lap under the current overrides, on a
    workspace that holds `fill`: [(score, end)], and the launches it queued."""
    import torch
    seqs, offs = gpu.pack_batch(trips)
    n = len(trips)
    dims = dims or tuple(max(len(t[k]) for t in trips) for k in range(3))
    dev = torch.device("cuda:0")
    d_seqs, d_offs = torch.from_numpy(seqs).to(dev), torch.from_numpy(offs).to(dev)
    need = gpu.score_ends_workspace_size(n, *dims, p, end=mode, kernel="lap")
    ws = torch.full((need,), fill, dtype=torch.uint8, device=dev)
    d_scores = torch.full((n,), -7, dtype=torch.int32, device=dev)
    d_ends = torch.full((3 * n,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    before = gpu.kernel_launch_count()
    gpu.score_batch_ends_async(d_seqs.data_ptr(), d_offs.data_ptr(), n, *dims, d_scores.data_ptr(),
                               d_ends.data_ptr(), ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream,
                               p, end=mode, kernel="lap")
    launches = gpu.kernel_launch_count() - before
    torch.cuda.synchronize()
    return list(zip(d_scores.cpu().tolist(), (tuple(r) for r in d_ends.cpu().view(-1, 3).tolist()))), launches


def _lit(gpu, trips, p, mode):
    return [(l[0], tuple(l[3])) for l in gpu.align_batch_ends(trips, p, end=mode)]


@functools.lru_cache(maxsize=None)
def _recipe(cell, kind):
    return cc.plant(cc.RECIPES[cell][kind == "at"][0], cc.SHAPE, cell, *cc.RECIPES[cell][kind == "at"][1:])


def _assert_plan(gpu, n, dims, p, mode, m, nw, checked):
    text = _plan(gpu.describe_score_ends_plan(n, *dims, p, end=mode, kernel="lap"))
    assert text.startswith(f"pencil lap i16 rtl M={m} NW={nw} ") and text.endswith(f"ends={mode}"), text
    assert (" checked " in text) == checked, text
    return _kv(text)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("m,nw", BUILT)
@pytest.mark.parametrize("shape", SHAPES)
def test_gpu_planted_match_the_references(gpu, orc, shape, m, nw, mode):
    """Exact a priori (12-bit words): no certificate, every geometry."""
    trips = planted(shape)
    with gpu.overrides(lap_m=m, lap_nw=nw):
        _assert_plan(gpu, len(trips), shape, None, mode, m, nw, False)
        got = gpu.score_batch_ends(trips, end=mode, kernel="lap")
    if mode == "any":
        assert got == [any_ref(orc, t) for t in trips]
        assert [e for _, e in got] == list(PLANTED[shape])
    else:
        assert got == [planted_face_ref(planted_name(shape, cell)) for cell in PLANTED[shape]]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("m,nw", [(1, 4), (2, 8)])
def test_gpu_ties_ones_and_a_ragged_batch(gpu, orc, m, nw, mode):
    trips = ragged_batch()
    with gpu.overrides(lap_m=m, lap_nw=nw):
        _assert_plan(gpu, len(trips), RAGGED_MAX, None, mode, m, nw, False)
        got = gpu.score_batch_ends(trips, end=mode, kernel="lap")
    assert got == _lit(gpu, trips, None, mode)
    names = list(SMALL)
    for name, g in zip(names, got[1:1 + len(names)]):
        assert g == small_ref(orc, name, mode), (name, mode)
    if mode == "any":
        for name, want in SMALL_ANY.items():
            assert got[1 + names.index(name)] == want
        assert got[1 + len(names)] == (24, (8, 8, 8)) == any_ref(orc, _repeat())


@pytest.mark.gpu
@pytest.mark.parametrize("m,nw", BUILT)
def test_gpu_certified_peak_at_every_cell_class(gpu, orc, m, nw):
    """Async, 8-bit words: a peak of exactly hi at one cell is certified; any
    returns (hi, that cell), face what tsa_align_batch_ends returns."""
    p = gpu.TsaParams.default(score_bits=cc.BITS)
    hi = cc.limits(orc, cc.params(orc))[1]
    cells = [c for c in cc.TARGETS if c[0] <= cc.SHAPE[0] - cc.X_DRAIN]
    trips = [_recipe(c, "at") for c in cells]
    face = _lit(gpu, trips, p, "face")
    with gpu.overrides(lap_m=m, lap_nw=nw):
        _assert_plan(gpu, 1, cc.SHAPE, p, "any", m, nw, True)
        for cell, t, f in zip(cells, trips, face):
            assert _async(gpu, [t], p, "any")[0] == [(hi, cell)], cell
            assert _async(gpu, [t], p, "face")[0] == [f], cell


@pytest.mark.gpu
@pytest.mark.parametrize("m,nw", BUILT)
def test_gpu_uncertified_async(gpu, m, nw):
    p = gpu.TsaParams.default(score_bits=cc.BITS)
    with gpu.overrides(lap_m=m, lap_nw=nw):
        for cell in cc.TARGETS:
            for mode in MODES:
                assert _async(gpu, [_recipe(cell, "over")], p, mode)[0] == [(gpu.SCORE_UNCERTIFIED, (0, 0, 0))], cell


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_gpu_uncertified_sync_counts_fallbacks(gpu, mode):
    """The synchronous call rescores an uncertified triple through the grid
    traceback's host path: tsa_align_batch_ends' score and end, one fallback."""
    p = gpu.TsaParams.default(score_bits=cc.BITS)
    trips = [_recipe(cell, "over") for cell in cc.TARGETS]
    want = _lit(gpu, trips, p, mode)
    with gpu.overrides(lap_m=2, lap_nw=4):
        for t, w in zip(trips, want):
            before = gpu.check_fallback_count()
            assert gpu.score_batch_ends([t], p, end=mode, kernel="lap") == [w]
            assert gpu.check_fallback_count() == before + 1


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_gpu_targets_at_x_la_and_the_corner_sync(gpu, mode):
    """Targets the drain cells may push over the certificate: the synchronous
    call equals tsa_align_batch_ends whichever way the certificate goes."""
    p = gpu.TsaParams.default(score_bits=cc.BITS)
    cells = [c for c in cc.TARGETS if c[0] > cc.SHAPE[0] - cc.X_DRAIN]
    assert (72, 50, 270) in cells and len(cells) >= 2
    trips = [_recipe(c, kind) for c in cells for kind in ("over", "at")]
    want = _lit(gpu, trips, p, mode)
    with gpu.overrides(lap_m=1, lap_nw=8):
        assert gpu.score_batch_ends(trips, p, end=mode, kernel="lap") == want


@functools.lru_cache(maxsize=None)
def _rounds_batch():
    """24 triples of (64, 256, 65..128), each with a run of 12 ending at its own
    cell, in a first-round row (45) or a last-round row (250) by turns."""
    out = []
    for k in range(cc.BATCH_N):
        shape = (cc.BATCH_LA, cc.BATCH_LB, cc.batch_lc(k))
        out.append(cc.plant(100 + k, shape, (50 + k % 10, cc.BATCH_ROWS[k % 2], shape[2] - 3 - k % 7), 12))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("nw", [4, 8])
def test_gpu_attribution_across_rounds(gpu, orc, nw):
    trips = _rounds_batch()
    dims = (cc.BATCH_LA, cc.BATCH_LB, 128)
    want = [any_ref(orc, t) for t in trips]
    assert len(set(want)) > cc.BATCH_N // 2      # the answers tell the triples apart
    with gpu.overrides(lap_m=1, lap_nw=nw):
        kv = _assert_plan(gpu, len(trips), dims, None, "any", 1, nw, False)
        assert int(kv["waves"]) == 3, kv
        assert gpu.score_batch_ends(trips, end="any", kernel="lap") == want
        assert _async(gpu, trips, None, "any", dims)[0] == want


@pytest.mark.gpu
def test_gpu_attribution_across_chunks(gpu, orc):
    trips = [cc.plant(200 + k, cc.SHAPE, cc.TARGETS[k % len(cc.TARGETS)], 12) for k in range(cc.BATCH_N)]
    want = [any_ref(orc, t) for t in trips]
    assert len(set(want)) > cc.BATCH_N // 2
    with gpu.overrides(lap_m=1, lap_nw=4):
        kv = _assert_plan(gpu, len(trips), cc.SHAPE, None, "any", 1, 4, False)
        assert int(kv["chunk"]) == 12, kv
        got, launches = _async(gpu, trips, None, "any")
        assert got == want and launches == 2
        assert gpu.score_batch_ends(trips, end="any", kernel="lap") == want


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_gpu_async_equals_sync_on_a_dirty_workspace(gpu, mode):
    trips = planted(SHAPES[0])
    with gpu.overrides(lap_m=2, lap_nw=4):
        got, launches = _async(gpu, trips, None, mode, fill=0xFF)
        assert launches == 1
        assert got == gpu.score_batch_ends(trips, end=mode, kernel="lap")
        assert got == _async(gpu, trips, None, mode, fill=0x00)[0]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_gpu_prefixes_compose_with_the_traceback(gpu, mode):
    trips = planted(SHAPES[0])[:4] + ragged_batch()
    with gpu.overrides(lap_m=1, lap_nw=4):
        ends = gpu.score_batch_ends(trips, end=mode, kernel="lap")
    cut = [tuple(s[:e] for s, e in zip(t, end)) for t, (_, end) in zip(trips, ends)]
    for (s, _), (s1, _, _) in zip(ends, gpu.align_batch(cut)):
        assert s1 == s


@pytest.mark.gpu
def test_gpu_corner_is_score_batch(gpu):
    trips = ragged_batch() + planted(SHAPES[1])
    got = gpu.score_batch_ends(trips, end="corner", kernel="lap")
    assert [s for s, _ in got] == list(gpu.score_batch(trips))
    assert [e for _, e in got] == [tuple(len(s) for s in t) for t in trips]


@pytest.mark.gpu
def test_gpu_timed_out_hand_off(gpu, orc):
    """lap_spin_limit = 0 (the existing bounded wait: the first poll of every
    consumer gives up): the async call reads TSA_SCORE_INVALID with ends 0, 0, 0,
    the synchronous one rescores the chunk and counts one fallback."""
    t = planted(SHAPES[0])[0]
    want = any_ref(orc, t)
    with gpu.overrides(lap_m=1, lap_nw=4, lap_spin_limit=0):
        assert _async(gpu, [t], None, "any")[0] == [(gpu.SCORE_INVALID, (0, 0, 0))]
        before = (gpu.fallback_count(), gpu.check_fallback_count())
        assert gpu.score_batch_ends([t], end="any", kernel="lap") == [want]
        assert (gpu.fallback_count(), gpu.check_fallback_count()) == (before[0] + 1, before[1])
    with gpu.overrides(lap_m=1, lap_nw=4):
        assert _async(gpu, [t], None, "any")[0] == [want]


def test_cli_lap_option():
    """--lap is parsed: without --score-end or with --kernel a usage error; with
    --score-end it runs (one workgroup: no lap plan, out of range) or gets as far
    as the device."""
    cli = os.path.join(PKG_DIR, "bin", "tsa")
    dat = os.path.join(ROOT, "tests", "golden", "dat")
    files = [f"{dat}/A_seq.dat", f"{dat}/B_seq.dat", f"{dat}/C_seq.dat"]
    run = lambda *extra: subprocess.run([cli, *files, *extra], capture_output=True, text=True)
    assert run("--lap").returncode == 2
    assert run("--score-end", "any", "--lap", "--kernel", "plane").returncode == 2
    assert run("--align", "--lap").returncode == 2
    r = run("--score-end", "any", "--lap")
    assert r.returncode in (0, 1) and "usage" not in r.stderr
    if r.returncode == 0:
        assert r.stdout.splitlines()[1].startswith("end (x1,y1,z1) = (")
