"""tsa_score_batch_ends_ex: end-free scores in the RTL's literal wrapped arithmetic.

The end search of the literal helix (csrc/literal_kernel.hip END) returns
tsa_align_batch_ends's score and end cell -- the best MAX7 over the real cells
of the mode in the wrapped words, at the smallest x, then y, then z -- for any
parameter set. The reference is the wrapped prefix brute force
(tests/test_align_ends.py: prefix_scores, ref_end): oracle.score_batch over all
prefixes under the case's parameters, then the first maximum in (x, y, z)
order. Every test of an input first asserts the reference conditions on the
oracle alone (test_reference_conditions): the wrapped and the unwrapped tables
differ where the case is a wrap case, the end is not the corner, and the
maximum is attained as often as the table below says.

Only the M = 1 and M = 2 kernels exist (LC <= 256): with the fold the M = 4
kernel does not fit the register file without scratch. The two M = 4 rows are
therefore TSA_ERANGE assertions on the library; the emulator still replays them.
"""
import ctypes
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG_DIR, ROOT
from test_align_ends import prefix_scores, ref_end

sys.path.insert(0, os.path.join(ROOT, "tools"))
import literal_emu  # noqa: E402

MODES = ["face", "any"]
END_MODE = {"corner": 0, "face": 1, "any": 2}
AUTO, PLANE, PENCIL, CHECKED = 0, 1, 2, 3
LIT_ENDS_MAX_LC = 256   # the largest LC whose END kernel exists (M = 2)


def related(seed, la, lb, lc, core):
    rng = np.random.default_rng(seed)
    R = rng.integers(0, 4, core).astype(np.uint8)
    mk = lambda n: R[:n] if n <= core else np.concatenate([R, rng.integers(0, 4, n - core).astype(np.uint8)])
    return mk(la), mk(lb), mk(lc)


def late(seed, la, lb, lc, core, zoff):
    rng = np.random.default_rng(seed)
    R = rng.integers(0, 4, core).astype(np.uint8)
    j = lambda n: rng.integers(0, 4, n).astype(np.uint8)
    return (np.concatenate([R, j(la - core)]), np.concatenate([R, j(lb - core)]),
            np.concatenate([j(zoff), R, j(lc - core - zoff)]))


def _z(n, s=0):
    return np.full(n, s, np.uint8)


WIDE = dict(match=900, mismatch=-700, gap_open=1100, gap_extend=300, score_bits=16)
WIDE_WRAP = dict(match=1500, mismatch=-700, gap_open=1100, gap_extend=300, score_bits=16)

# name -> (triple, params, wraps, {mode: (score, end, cells at the maximum)})
TABLE = {
    "m1_bits6": (related(1, 20, 19, 70, 16), dict(score_bits=6), True,
                 {"face": (29, (14, 19, 18), 2), "any": (31, (13, 13, 13), 25)}),
    "m1_homo_bits5": ((_z(12), _z(17), _z(66)), dict(score_bits=5), True,
                      {"face": (15, (5, 5, 66), 160), "any": (15, (5, 5, 5), 1324)}),
    "m2_hi_bits5": (late(11, 10, 11, 140, 9, 125), dict(score_bits=5), True,
                    {"face": (14, (10, 8, 137), 2), "any": (15, (5, 5, 130), 8)}),
    "m2_hi_homo": ((_z(10), _z(11), np.concatenate([_z(125, 1), _z(15)])), dict(score_bits=5), True,
                   {"face": (15, (5, 5, 140), 42), "any": (15, (5, 5, 130), 162)}),
    "m4_hi_bits5": (late(12, 9, 10, 260, 8, 250), dict(score_bits=5), True,
                    {"face": (15, (8, 8, 260), 1), "any": (15, (5, 5, 190), 19)}),
    "m4_hi_homo": ((_z(9), _z(10), np.concatenate([_z(248, 1), _z(12)])), dict(score_bits=5), True,
                   {"face": (15, (5, 5, 260), 32), "any": (15, (5, 5, 253), 100)}),
    "go_lt_ge": (related(4, 14, 19, 40, 10), dict(gap_open=1, gap_extend=2), False,
                 {"face": (31, (14, 14, 15), 2), "any": (31, (14, 14, 15), 2)}),
    "go_lt_ge_sop": (related(5, 14, 9, 130, 8), dict(gap_open=1, gap_extend=2, s3_mode=1), False,
                     {"face": (25, (10, 9, 9), 2), "any": (25, (10, 9, 9), 2)}),
    "wide16": (related(6, 12, 9, 30, 7), WIDE, False,
               {"face": (19800, (12, 9, 10), None), "any": (19800, (9, 8, 9), 2)}),
    "wide16_wrap": ((_z(14), _z(9), _z(20)), WIDE_WRAP, True,
                    {"face": (32700, (8, 9, 10), 62), "any": (32700, (8, 9, 10), 90)}),
}
# the unwrapped (score_bits = 0) answer under "any" (None: only the score is recorded)
UNWRAPPED_ANY = {"m1_bits6": (48, (16, 16, 16)), "m1_homo_bits5": (36, (12, 12, 12)),
                 "m2_hi_bits5": (27, (9, 9, 134)), "m2_hi_homo": (30, None), "m4_hi_bits5": (24, (8, 8, 258)),
                 "m4_hi_homo": (27, None), "wide16_wrap": (45700, (14, 9, 14))}
NAMES = list(TABLE)
ON_DEVICE = [n for n in NAMES if len(TABLE[n][0][2]) <= LIT_ENDS_MAX_LC]
M4 = [n for n in NAMES if n not in ON_DEVICE]
SHORT = ["m1_bits6", "m1_homo_bits5", "go_lt_ge", "wide16", "wide16_wrap"]
RAGGED_GEOMS = [(140, 19, 140), (20, 19, 260)]


def brute(orc, name, mode):
    """(score, end) of the wrapped prefix brute force."""
    t, kw, _, _ = TABLE[name]
    (s, _, _, end), _ = ref_end(orc, *t, kw, mode)
    return int(s), tuple(end)


def emu_kw(kw):
    return dict(match=kw.get("match", 1), mismatch=kw.get("mismatch", -1), go=kw.get("gap_open", 2),
                ge=kw.get("gap_extend", 1), sop=kw.get("s3_mode", 0) == 1, bits=kw.get("score_bits", 12))


# ---- CPU: the reference's own conditions ------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_reference_conditions(orc, name):
    t, kw, wraps, want = TABLE[name]
    v = prefix_scores(orc, *t, kw)
    u = prefix_scores(orc, *t, dict(kw, score_bits=0))
    assert bool((v != u).any()) == wraps, name
    lens = tuple(len(s) for s in t)
    for mode in MODES:
        s, end = brute(orc, name, mode)
        ws, wend, wn = want[mode]
        assert (s, end) == (ws, wend), (name, mode)
        assert end != lens                                                   # not the corner
        cand = np.ones(v.shape, bool)
        if mode == "face":
            cand[:lens[0] - 1, :lens[1] - 1, :lens[2] - 1] = False
        if wn is not None:
            assert int(((v == s) & cand).sum()) == wn, (name, mode)
    if name in UNWRAPPED_ANY:
        us, uend = UNWRAPPED_ANY[name]
        assert int(u.max()) == us
        if uend is not None:
            assert tuple(int(i) + 1 for i in np.unravel_index(int(np.argmax(u)), u.shape)) == uend
        assert (us, uend) != want["any"][:2]
    if name == "wide16":
        assert want["any"][0] > 2047                                         # far outside 12 bits


# ---- CPU: the interface -------------------------------------------------------------------

NEW = ("tsa_score_batch_ends_ex", "tsa_score_ends_workspace_size_ex", "tsa_score_batch_ends_async_ex",
       "tsa_describe_score_ends_plan_ex")


def test_exports(tsa):
    with open(os.path.join(ROOT, "include", "trialign.h")) as f:
        header = f.read()
    for name in NEW:
        assert name in tsa.EXPORTS and hasattr(tsa.lib(), name), name
        assert f"int {name}(" in header
    for fn in ("score_batch_ends", "score_ends_workspace_size", "score_batch_ends_async", "describe_score_ends_plan"):
        assert inspect.signature(getattr(tsa, fn)).parameters["kernel"].default is None, fn


def _raw_ex(tsa, seqs, offsets, n, p, end_mode, kernel, null=None):
    u8, i32, i64 = (ctypes.POINTER(t) for t in (ctypes.c_uint8, ctypes.c_int32, ctypes.c_int64))
    seqs = np.ascontiguousarray(seqs, np.uint8)
    offsets = np.ascontiguousarray(offsets, np.int64)
    m = max(abs(n), 1)
    out = dict(scores=np.zeros(m, np.int32), ends=np.zeros(3 * m, np.int32))
    arg = lambda k: None if k == null else out[k].ctypes.data_as(i32)
    return tsa.lib().tsa_score_batch_ends_ex(seqs.ctypes.data_as(u8), offsets.ctypes.data_as(i64), n, ctypes.byref(p),
                                             end_mode, kernel, arg("scores"), arg("ends"), 0)


def _raw_old(tsa, seqs, offsets, n, p, end_mode, null=None):
    u8, i32, i64 = (ctypes.POINTER(t) for t in (ctypes.c_uint8, ctypes.c_int32, ctypes.c_int64))
    seqs = np.ascontiguousarray(seqs, np.uint8)
    offsets = np.ascontiguousarray(offsets, np.int64)
    m = max(abs(n), 1)
    out = dict(scores=np.zeros(m, np.int32), ends=np.zeros(3 * m, np.int32))
    arg = lambda k: None if k == null else out[k].ctypes.data_as(i32)
    return tsa.lib().tsa_score_batch_ends(seqs.ctypes.data_as(u8), offsets.ctypes.data_as(i64), n, ctypes.byref(p),
                                          end_mode, arg("scores"), arg("ends"), 0)


def test_argument_order(tsa):
    """TSA_EINVAL, then TSA_OK for n = 0, then TSA_ERANGE, then TSA_ENODEV: all before any device work."""
    p = tsa.TsaParams.default()
    seqs, offs = tsa.pack_batch([([0, 1], [1, 2], [2, 3]), ([0], [1], [2])])
    beyond = tsa.TSA_OK if tsa.device_count() > 0 else tsa.TSA_ENODEV
    for kernel in (-1, 4, 17):
        for mode in (0, 1, 2):
            assert _raw_ex(tsa, seqs, offs, 2, p, mode, kernel) == tsa.TSA_EINVAL
    for kernel in (AUTO, PLANE, PENCIL, CHECKED):
        for mode in (0, 1, 2):
            for null in ("scores", "ends"):
                assert _raw_ex(tsa, seqs, offs, 2, p, mode, kernel, null=null) == tsa.TSA_EINVAL
            assert _raw_ex(tsa, seqs, offs, -1, p, mode, kernel) == tsa.TSA_EINVAL
            bad = seqs.copy()
            bad[1] = 9
            assert _raw_ex(tsa, bad, offs, 2, p, mode, kernel) == tsa.TSA_EINVAL
            assert _raw_ex(tsa, seqs, offs, 2, tsa.TsaParams.default(score_bits=3), mode, kernel) == tsa.TSA_EINVAL
            assert _raw_ex(tsa, np.zeros(1, np.uint8), np.zeros(1, np.int64), 0, p, mode, kernel) == tsa.TSA_OK
        for mode in (3, -1):
            assert _raw_ex(tsa, seqs, offs, 2, p, mode, kernel) == tsa.TSA_EINVAL
    lit = tsa.TsaParams.default(gap_open=1, gap_extend=2)
    c257, c513 = (tsa.pack_batch([([0, 1], [1, 2], [2] * n)]) for n in (257, 513))
    a4096 = tsa.pack_batch([([1] * 4096, [1, 2], [2, 3])])
    for mode in (0, 1, 2):
        assert _raw_ex(tsa, seqs, offs, 2, p, mode, CHECKED) == tsa.TSA_ERANGE
    for mode in (1, 2):
        assert _raw_ex(tsa, *c513, 1, p, mode, PLANE) == tsa.TSA_ERANGE
        assert _raw_ex(tsa, *c513, 1, p, mode, AUTO) == tsa.TSA_ERANGE
        assert _raw_ex(tsa, *a4096, 1, p, mode, PLANE) == tsa.TSA_ERANGE
        assert _raw_ex(tsa, *a4096, 1, lit, mode, AUTO) == tsa.TSA_ERANGE
        # only the M = 1 and M = 2 END kernels exist: LC = 257 is past the largest one
        assert _raw_ex(tsa, *c257, 1, p, mode, PLANE) == tsa.TSA_ERANGE
        assert _raw_ex(tsa, *c257, 1, p, mode, AUTO) == tsa.TSA_ERANGE
        # literal-only parameters get past admission under AUTO and PLANE
        assert _raw_ex(tsa, seqs, offs, 2, lit, mode, AUTO) == beyond
        assert _raw_ex(tsa, seqs, offs, 2, lit, mode, PLANE) == beyond
        assert _raw_ex(tsa, seqs, offs, 2, p, mode, PLANE) == beyond
        with tsa.overrides(pencil_mode="literal"):
            assert _raw_ex(tsa, seqs, offs, 2, p, mode, AUTO) == beyond
            assert _raw_ex(tsa, seqs, offs, 2, p, mode, PLANE) == beyond
        with tsa.overrides(pencil_mode="helix"):
            assert _raw_ex(tsa, seqs, offs, 2, p, mode, AUTO) == beyond
            assert _raw_ex(tsa, seqs, offs, 2, lit, mode, AUTO) == tsa.TSA_ERANGE
            assert _raw_ex(tsa, seqs, offs, 2, p, mode, PLANE) == tsa.TSA_EINVAL
        for other in ("lap", "plane", "litlap"):
            with tsa.overrides(pencil_mode=other):
                assert _raw_ex(tsa, seqs, offs, 2, p, mode, AUTO) == tsa.TSA_EINVAL
                assert _raw_ex(tsa, seqs, offs, 2, lit, mode, PLANE) == tsa.TSA_EINVAL
    # an unwrapped range outside int16 (score_bits = 0) is refused as everywhere
    wide0 = tsa.TsaParams.default(match=1500, mismatch=-700, gap_open=1100, gap_extend=300, score_bits=0)
    with pytest.raises(tsa.TsaError) as e:
        tsa.describe_score_ends_plan(1, 64, 64, 64, params=wide0, kernel="plane")
    assert e.value.rc == tsa.TSA_ERANGE


def test_pencil_is_the_old_call(tsa):
    """TSA_KERNEL_PENCIL returns exactly what tsa_score_batch_ends returns, on
    the inputs of tests/test_score_ends.py::test_argument_errors."""
    p = tsa.TsaParams.default()
    seqs, offs = tsa.pack_batch([([0, 1], [1, 2], [2, 3]), ([0], [1], [2])])
    lit = tsa.TsaParams.default(gap_open=1, gap_extend=2)
    long_c = tsa.pack_batch([([0, 1], [1, 2], [2] * 257)])
    bad = seqs.copy()
    bad[1] = 9
    calls = []
    for mode in (0, 1, 2, 3, -1):
        calls += [(seqs, offs, 2, p, mode, None), (seqs, offs, 2, p, mode, "scores"), (seqs, offs, 2, p, mode, "ends"),
                  (seqs, offs, -1, p, mode, None), (bad, offs, 2, p, mode, None),
                  (np.zeros(6, np.uint8), np.array([0, 3, 2, 6], np.int64), 1, p, mode, None),
                  (seqs, offs, 2, tsa.TsaParams.default(score_bits=3), mode, None),
                  (np.zeros(1, np.uint8), np.zeros(1, np.int64), 0, p, mode, None),
                  (seqs, offs, 2, lit, mode, None), (*long_c, 1, p, mode, None)]
    for ov in (dict(), dict(pencil_arith="i16"), dict(pencil_mode="lap"), dict(pencil_mode="helix", pencil_two="1"),
               dict(pencil_mode="literal")):
        with tsa.overrides(**ov):
            for s, o, n, pp, mode, null in calls:
                assert _raw_ex(tsa, s, o, n, pp, mode, PENCIL, null=null) == _raw_old(tsa, s, o, n, pp, mode, null=null), \
                    (ov, n, mode, null)
    d = tsa.describe_score_ends_plan
    for mode in MODES + ["corner"]:
        assert d(512, 256, 256, 256, end=mode, kernel="pencil") == d(512, 256, 256, 256, end=mode)
        assert tsa.score_ends_workspace_size(300, 40, 19, 140, end=mode, kernel="pencil") == \
            tsa.score_ends_workspace_size(300, 40, 19, 140, end=mode)
    for kw, shape in ((dict(gap_open=1, gap_extend=2), (64, 64, 64)), (dict(), (64, 64, 257))):
        with pytest.raises(tsa.TsaError) as e:
            d(4, *shape, params=tsa.TsaParams.default(**kw), kernel="pencil")
        assert e.value.rc == tsa.TSA_ERANGE


def test_plan_text_and_workspace(tsa):
    d = tsa.describe_score_ends_plan
    lit = tsa.TsaParams.default(gap_open=1, gap_extend=2)
    for mode in MODES:
        assert d(512, 256, 256, 256, end=mode, kernel="plane") == f"plane literal-helix M=2 P=260 ends={mode}"
        assert d(4, 64, 64, 64, end=mode, kernel="plane") == f"plane literal-helix M=1 P=128 ends={mode}"
        assert d(4, 4095, 4096, 256, params=lit, end=mode, kernel="plane").startswith("plane literal-helix M=2 P=4096")
        # AUTO: the factored text where tsa_score_batch_ends admits the request, the literal one where not
        assert d(512, 256, 256, 256, end=mode, kernel="auto") == d(512, 256, 256, 256, end=mode)
        assert d(512, 256, 256, 256, end=mode, kernel="auto").startswith("pencil helix")
        for kw, shape in ((dict(gap_open=1, gap_extend=2), (64, 64, 64)), (dict(), (2000, 2000, 256)),
                          (dict(), (64, 2049, 64)), (dict(score_bits=6), (40, 19, 140))):
            pp = tsa.TsaParams.default(**kw)
            with pytest.raises(tsa.TsaError) as e:
                d(4, *shape, params=pp, end=mode)
            assert e.value.rc == tsa.TSA_ERANGE
            text = d(4, *shape, params=pp, end=mode, kernel="auto")
            assert text.startswith("plane literal-helix M=") and text.endswith(f"ends={mode}"), text
            assert text == d(4, *shape, params=pp, end=mode, kernel="plane")
        with tsa.overrides(pencil_mode="literal"):
            text = d(4, 64, 64, 64, end=mode, kernel="auto")
            assert text.startswith(f"plane literal-helix M=1 P=128 ends={mode} overrides=") and "pencil_mode=literal" in text
        with tsa.overrides(pencil_mode="helix"):
            assert d(4, 64, 64, 64, end=mode, kernel="auto").startswith("pencil helix")
        for shape in ((64, 64, 257), (64, 64, 512), (64, 64, 513), (4096, 64, 64), (64, 4097, 64)):
            for kernel in ("plane", "auto"):
                with pytest.raises(tsa.TsaError) as e:
                    d(4, *shape, params=lit, end=mode, kernel=kernel)
                assert e.value.rc == tsa.TSA_ERANGE, (shape, kernel)
        with pytest.raises(tsa.TsaError) as e:
            d(4, 64, 64, 64, end=mode, kernel="checked")
        assert e.value.rc == tsa.TSA_ERANGE
        with pytest.raises(tsa.TsaError) as e:
            d(4, 64, 64, 64, end=mode, kernel=7)
        assert e.value.rc == tsa.TSA_EINVAL
        # the workspace is the literal ring of that geometry
        for n, shape in ((512, (256, 256, 256)), (70000, (100, 40, 200)), (300, (40, 19, 140)), (3, (4095, 4096, 256))):
            with tsa.overrides(pencil_mode="literal"):
                assert "literal-helix" in tsa.describe_plan(n, *shape, kernel="plane", sync=False)
                want = tsa.workspace_size(n, *shape, kernel="plane")
                assert tsa.score_ends_workspace_size(n, *shape, end=mode, kernel="plane") == want
                assert tsa.score_ends_workspace_size(n, *shape, end=mode, kernel="auto") == want
            assert tsa.score_ends_workspace_size(n, *shape, end=mode, kernel="plane") == want
    for kernel in ("auto", "plane"):
        for shape in ((256, 256, 256), (64, 64, 64)):
            assert d(512, *shape, end="corner", kernel=kernel) == tsa.describe_plan(512, *shape, kernel=kernel)
            assert tsa.score_ends_workspace_size(8, *shape, end="corner", kernel=kernel) == \
                tsa.workspace_size(8, *shape, kernel=kernel)


def test_cli_kernel_with_score_end():
    cli = os.path.join(PKG_DIR, "bin", "tsa")
    dat = os.path.join(ROOT, "tests", "golden", "dat")
    files = [f"{dat}/A_seq.dat", f"{dat}/B_seq.dat", f"{dat}/C_seq.dat"]
    run = lambda *extra: subprocess.run([cli, *files, *extra], capture_output=True, text=True)
    assert run("--score-end", "any", "--kernel", "pencil").returncode == 2
    assert run("--score-end", "any", "--kernel", "plane", "--states").returncode == 2
    assert run("--score-end", "any", "--kernel", "plane", "--align").returncode == 2
    for kernel in ("plane", "auto"):
        for end in MODES:
            r = run("--score-end", end, "--kernel", kernel, "--go", "1", "--ge", "2")
            if r.returncode == 0:
                lines = r.stdout.splitlines()
                assert lines[0].startswith("TriAlign Score:") and lines[1].startswith("end (x1,y1,z1) = (")
            else:
                assert r.returncode == 1 and "no HIP device" in r.stderr and "usage" not in r.stderr


# ---- CPU: the kernel's fold, replayed (tools/literal_emu.py) --------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_emulator_matches_the_brute_force(orc, name):
    t, kw, _, _ = TABLE[name]
    got = literal_emu.emulate_ends(t, end=("any", "face"), **emu_kw(kw))
    for mode in MODES:
        assert got[mode] == brute(orc, name, mode), (name, mode)
    assert literal_emu.emulate_ends(t, end="any", **emu_kw(kw)) == got["any"]


@pytest.mark.parametrize("geom", RAGGED_GEOMS)
@pytest.mark.parametrize("name", SHORT)
def test_emulator_in_a_ragged_geometry(orc, name, geom):
    """A short triple in the geometry of a batch's maxima: every padding cell
    in x, y and z is computed and must be masked."""
    t, kw, _, _ = TABLE[name]
    assert all(len(s) < g for s, g in zip(t, geom)) or any(len(s) < g for s, g in zip(t, geom))
    got = literal_emu.emulate_ends(t, end=("any", "face"), max_lens=geom, **emu_kw(kw))
    for mode in MODES:
        assert got[mode] == brute(orc, name, mode), (name, geom, mode)


def test_emulator_corner_is_unchanged(orc):
    t, kw, _, _ = TABLE["go_lt_ge"]
    s, fin = literal_emu.emulate(*t, **emu_kw(kw))
    assert s == int(orc.score(*t, orc.default_params(**kw))) and len(fin) == 7


def test_emulator_key_limits():
    """The key at its field limits: encode, order and decode."""
    key, key64, dec = literal_emu.end_key, literal_emu.end_key64, literal_emu.end_decode
    scores, xs, laps, zs, ws = (-32768, -1, 0, 32767), (1, 2, 4095), (0, 1, 511), (1, 2, 512), (0, 7)
    seen = set()
    for s in scores:
        for x in xs:
            k32 = key(s & 0xFFFF, x)
            assert 0 < k32 < 2 ** 32 and k32 not in seen       # 0 is "no candidate yet"
            seen.add(k32)
            for lap in laps:
                for w in ws:
                    for z in zs:
                        k64 = key64(k32, lap, w, z - 1)
                        assert 0 < k64 < 2 ** 64
                        assert dec(k64, 0) == (s, (x, lap * literal_emu.NW + w + 1, z))
    assert dec(key64(key((-16 << 11) & 0xFFFF, 3), 2, 1, 4), 11) == (-16, (3, 18, 5))   # 5-bit words, shifted
    assert dec(key64(key((15 << 11) & 0xFFFF, 3), 2, 1, 4), 11) == (15, (3, 18, 5))
    # order: the score first, then the smaller x, then the smaller y, then the smaller z
    assert key(32767, 4095) > key(32766, 1) > key(0, 1) > key(0xFFFF, 1) > key(0x8000, 1) > key(0x8000, 4095)
    assert key(5, 1) > key(5, 2) > key(5, 4095)
    k = key(5, 7)
    assert key64(k, 0, 0, 511) > key64(k, 0, 1, 0) > key64(k, 0, 7, 0) > key64(k, 1, 0, 0) > key64(k, 511, 7, 0)
    assert key64(k, 3, 2, 0) > key64(k, 3, 2, 1) > key64(k, 3, 2, 511)
    assert key64(key(5, 8), 0, 0, 0) < key64(k, 511, 7, 511)


# ---- GPU ----------------------------------------------------------------------------------

def _params(gpu, kw):
    return gpu.TsaParams.default(**kw)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ON_DEVICE)
def test_gpu_table(gpu, orc, name, mode):
    t, kw, _, _ = TABLE[name]
    want = brute(orc, name, mode)
    p = _params(gpu, kw)
    shape = tuple(len(s) for s in t)
    assert gpu.describe_score_ends_plan(1, *shape, params=p, end=mode, kernel="plane").startswith("plane literal-helix")
    assert gpu.score_batch_ends([t], params=p, end=mode, kernel="plane") == [want]
    with gpu.overrides(pencil_mode="literal"):
        assert gpu.score_batch_ends([t], params=p, end=mode, kernel="auto") == [want]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", M4)
def test_gpu_m4_rows_are_refused(gpu, name, mode):
    """No M = 4 END kernel: LC > 256 is TSA_ERANGE under PLANE and AUTO."""
    t, kw, _, _ = TABLE[name]
    for kernel in ("plane", "auto"):
        with pytest.raises(gpu.TsaError) as e:
            gpu.score_batch_ends([t], params=_params(gpu, kw), end=mode, kernel=kernel)
        assert e.value.rc == gpu.TSA_ERANGE


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_gpu_table_as_one_ragged_batch(gpu, orc, mode):
    """The rows that share a parameter set as one batch: max_l* exceed most
    triples' own lengths (M = 2 geometry for the M = 1 rows)."""
    groups = {}
    for name in ON_DEVICE:
        groups.setdefault(tuple(sorted(TABLE[name][1].items())), []).append(name)
    assert max(len(g) for g in groups.values()) >= 3
    for kw, names in groups.items():
        trips = [TABLE[n][0] for n in names]
        got = gpu.score_batch_ends(trips, params=_params(gpu, dict(kw)), end=mode, kernel="plane")
        assert got == [brute(orc, n, mode) for n in names], names
    # every row under the table's widest geometry, per parameter set: the short rows next to a long one
    for name in SHORT:
        t, kw, _, _ = TABLE[name]
        pad = tuple(np.zeros(n, np.uint8) for n in (140, 19, 140))
        got = gpu.score_batch_ends([pad, t, pad], params=_params(gpu, kw), end=mode, kernel="plane")
        assert got[1] == brute(orc, name, mode), name


CROSS = [(40, 19, 140), (261, 11, 130)]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("bits", [6, 12, 16])
def test_gpu_cross_check_against_the_traceback(gpu, bits, mode):
    p = gpu.TsaParams.default(score_bits=bits)
    rng = np.random.default_rng(100 + bits)
    for shape in CROSS:
        trips = [tuple(rng.integers(0, 4, n).astype(np.uint8) for n in shape), related(bits, *shape, 12),
                 related(bits + 1, *shape, shape[1])]
        want = [(s, tuple(e)) for s, _, _, e in gpu.align_batch_ends(trips, params=p, end=mode)]
        assert gpu.score_batch_ends(trips, params=p, end=mode, kernel="plane") == want, (shape, bits)
        with gpu.overrides(pencil_mode="literal"):
            assert gpu.score_batch_ends(trips, params=p, end=mode, kernel="auto") == want


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_gpu_async(gpu, orc, mode):
    import torch
    names = ["m2_hi_bits5", "m2_hi_homo", "m1_homo_bits5"]
    p = _params(gpu, dict(score_bits=5))
    trips = [TABLE[n][0] for n in names]
    seqs, offs = gpu.pack_batch(trips)
    n = len(trips)
    shape = tuple(max(len(t[j]) for t in trips) for j in range(3))
    dev = torch.device("cuda:0")
    d_seqs = torch.from_numpy(seqs).to(dev)
    d_offs = torch.from_numpy(offs).to(dev)
    need = gpu.score_ends_workspace_size(n, *shape, params=p, end=mode, kernel="plane")
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=dev)
    d_scores = torch.full((n,), -7, dtype=torch.int32, device=dev)
    d_ends = torch.full((3 * n,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    before = gpu.kernel_launch_count()
    with pytest.raises(gpu.TsaError) as e:
        gpu.score_batch_ends_async(d_seqs.data_ptr(), d_offs.data_ptr(), n, *shape, d_scores.data_ptr(),
                                   d_ends.data_ptr(), ws.data_ptr(), need - 1, stream, params=p, end=mode,
                                   kernel="plane")
    assert e.value.rc == gpu.TSA_ENOMEM and gpu.kernel_launch_count() == before
    torch.cuda.synchronize()
    assert int((d_scores != -7).sum()) == 0 and int((d_ends != -7).sum()) == 0
    gpu.score_batch_ends_async(d_seqs.data_ptr(), d_offs.data_ptr(), n, *shape, d_scores.data_ptr(),
                               d_ends.data_ptr(), ws.data_ptr(), need, stream, params=p, end=mode, kernel="plane")
    assert gpu.kernel_launch_count() == before + 1
    torch.cuda.synchronize()
    got = list(zip(d_scores.cpu().tolist(), (tuple(r) for r in d_ends.cpu().view(-1, 3).tolist())))
    assert got == gpu.score_batch_ends(trips, params=p, end=mode, kernel="plane")
    assert got == [brute(orc, nm, mode) for nm in names]


@pytest.mark.gpu
def test_gpu_corner_under_each_kernel(gpu):
    import torch
    trips = [TABLE[n][0] for n in ("m1_bits6", "go_lt_ge", "m2_hi_bits5")]
    lens = [tuple(len(s) for s in t) for t in trips]
    seqs, offs = gpu.pack_batch(trips)
    n = len(trips)
    shape = tuple(max(l[j] for l in lens) for j in range(3))
    dev = torch.device("cuda:0")
    d_seqs, d_offs = torch.from_numpy(seqs).to(dev), torch.from_numpy(offs).to(dev)
    stream = torch.cuda.current_stream().cuda_stream
    for kernel in ("auto", "plane", "pencil"):
        got = gpu.score_batch_ends(trips, end="corner", kernel=kernel)
        assert [e for _, e in got] == lens
        want = [gpu.score(*t, kernel=kernel) for t in trips]
        assert [s for s, _ in got] == want, kernel
        need = gpu.score_ends_workspace_size(n, *shape, end="corner", kernel=kernel)
        assert need == gpu.workspace_size(n, *shape, kernel=kernel)
        ws = torch.zeros(max(need, 16), dtype=torch.uint8, device=dev)
        d_scores = torch.full((n,), -7, dtype=torch.int32, device=dev)
        d_ref = torch.full((n,), -7, dtype=torch.int32, device=dev)
        d_ends = torch.full((3 * n,), -7, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        gpu.score_batch_ends_async(d_seqs.data_ptr(), d_offs.data_ptr(), n, *shape, d_scores.data_ptr(),
                                   d_ends.data_ptr(), ws.data_ptr(), need, stream, end="corner", kernel=kernel)
        torch.cuda.synchronize()
        ws.zero_()
        gpu.score_batch_async(d_seqs.data_ptr(), d_offs.data_ptr(), n, *shape, d_ref.data_ptr(), ws.data_ptr(), need,
                              stream, kernel=kernel)
        torch.cuda.synchronize()
        assert d_scores.cpu().tolist() == d_ref.cpu().tolist() == want
        assert [tuple(r) for r in d_ends.cpu().view(-1, 3).tolist()] == lens


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_gpu_auto_routing(gpu, orc, mode):
    # an input the factored call admits: AUTO is tsa_score_batch_ends exactly
    rng = np.random.default_rng(3)
    trips = [related(9, 40, 19, 140, 12), tuple(rng.integers(0, 4, n).astype(np.uint8) for n in (30, 12, 70))]
    shape = (40, 19, 140)
    assert gpu.describe_score_ends_plan(2, *shape, end=mode, kernel="auto").startswith("pencil helix")
    old = gpu.score_batch_ends(trips, end=mode)
    assert gpu.score_batch_ends(trips, end=mode, kernel="auto") == old
    assert gpu.score_batch_ends(trips, end=mode, kernel="pencil") == old
    assert gpu.score_batch_ends(trips, end=mode, kernel="plane") == old      # no wrap here: the same answer
    # literal-only parameters: AUTO is PLANE
    t, kw, _, _ = TABLE["go_lt_ge"]
    p = _params(gpu, kw)
    assert gpu.describe_score_ends_plan(1, 14, 19, 40, params=p, end=mode, kernel="auto").startswith("plane literal-helix")
    got = gpu.score_batch_ends([t], params=p, end=mode, kernel="auto")
    assert got == gpu.score_batch_ends([t], params=p, end=mode, kernel="plane") == [brute(orc, "go_lt_ge", mode)]
