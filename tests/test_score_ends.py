"""tsa_score_batch_ends: end-free scores and end cells from the helix scorer.

The semantics are tsa_align_batch_ends': the best MAX7 over the real cells of
the mode, at the cell with the smallest x, then y, then z. References:
  any   oracle.best_range(a, b, c): bmax and at_max (the first cell in (x, y, z)
        order), the unwrapped sweep, which equals the wrapped one wherever the
        plan is admitted;
  face  the prefix brute force: tests/test_align_ends.py's (ref_end) on the
        small inputs, and over the face cells alone (face_brute) on the planted
        cubes, recorded in tests/golden/score_ends_face.json because it takes
        up to a minute a cube;
  both  on the GPU also tsa_align_batch_ends, an independent literal kernel
        that is itself tested against the oracle.
Every CPU test of an input first asserts the reference condition on the oracle
alone.
"""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG_DIR, ROOT
from _checked_cases import plant
from test_align_ends import prefix_scores, ref_end

MODES = ["face", "any"]

# planted peaks: shape -> {cell: (seed, r)}; the cell is best_range's at_max
# under the default parameters
PLANTED = {
    # M = 2, P = 256 > LA (padding columns), 3 laps with a ragged last one
    (40, 19, 140): {(40, 19, 140): (0, 12), (17, 8, 64): (1, 8), (18, 9, 65): (0, 9), (19, 16, 128): (0, 12),
                    (20, 17, 129): (0, 12), (40, 5, 70): (0, 5), (12, 19, 33): (0, 12), (25, 10, 140): (0, 10),
                    (30, 8, 127): (0, 8), (31, 9, 130): (0, 9)},
    # M = 1, P = LA
    (140, 19, 100): {(140, 19, 100): (0, 12), (128, 8, 64): (1, 8), (129, 9, 65): (0, 9), (139, 16, 99): (0, 12)},
    # M = 2, LA > 256, P = 264
    (261, 11, 130): {(256, 8, 128): (0, 8), (257, 9, 129): (0, 9), (261, 11, 130): (0, 11), (200, 10, 64): (0, 10)},
}
SHAPES = list(PLANTED)


def planted(shape):
    return [plant(seed, shape, cell, r) for cell, (seed, r) in PLANTED[shape].items()]


def _homo(la, lb, lc):
    return tuple(np.zeros(n, np.uint8) for n in (la, lb, lc))


def _repeat():
    """a = R + junk, b = R + junk + R, c = R + junk + R + junk, |R| = 8."""
    rng = np.random.default_rng(0)
    R = rng.integers(0, 4, 8).astype(np.uint8)
    junk = lambda n: rng.integers(0, 4, n).astype(np.uint8)
    return (np.concatenate([R, junk(30)]), np.concatenate([R, junk(3), R]),
            np.concatenate([R, junk(120), R, junk(4)]))


def _one(k, n=6):
    """An end with a coordinate of 1: one common symbol, then symbols that
    match nothing in the other two sequences; sequence k is the single symbol."""
    seqs = [np.concatenate([[0], np.full(n, s)]).astype(np.uint8) for s in (1, 2, 3)]
    seqs[k] = np.array([0], np.uint8)
    return tuple(seqs)


def _small_ragged():
    rng = np.random.default_rng(7)
    out = [tuple(np.array([s], np.uint8) for s in (2, 2, 2))]                  # 1 x 1 x 1
    for la, lb, lc in ((3, 12, 5), (12, 2, 7), (9, 9, 9), (1, 4, 11), (5, 1, 1)):
        out.append(tuple(rng.integers(0, 4, n).astype(np.uint8) for n in (la, lb, lc)))
    return out


# small inputs: the face reference is the prefix brute force
SMALL = {
    "homo_5_9_140": _homo(5, 9, 140), "homo_9_5_140": _homo(9, 5, 140), "homo_140_9_5": _homo(140, 9, 5),
    "one_x": _one(0), "one_y": _one(1), "one_z": _one(2),
}
SMALL.update({f"ragged{i}": t for i, t in enumerate(_small_ragged())})
# the answers the construction is meant to give (asserted on the oracle alone)
SMALL_ANY = {"homo_5_9_140": (15, (5, 5, 5)), "homo_9_5_140": (15, (5, 5, 5)), "homo_140_9_5": (15, (5, 5, 5)),
             "one_x": (3, (1, 1, 1)), "one_y": (3, (1, 1, 1)), "one_z": (3, (1, 1, 1))}


def any_ref(orc, t):
    r = orc.best_range(*t)
    return int(r.bmax), tuple(int(v) for v in r.at_max)


def face_ref(orc, t):
    (s, _, _, end), _ = ref_end(orc, *t, {}, "face")
    return int(s), tuple(end)


def small_ref(orc, name, mode):
    return any_ref(orc, SMALL[name]) if mode == "any" else face_ref(orc, SMALL[name])


def ragged_batch():
    """The shapes above mixed with the small triples: max_l* exceed most
    triples' own lengths."""
    return [planted(SHAPES[0])[1], *SMALL.values(), _repeat(), planted(SHAPES[0])[6]]


# ---- CPU: the references' own conditions -----------------------------------------

@pytest.mark.parametrize("shape", SHAPES)
def test_planted_peaks_are_the_oracle_s(orc, shape):
    for (cell, _), t in zip(PLANTED[shape].items(), planted(shape)):
        assert tuple(len(s) for s in t) == shape
        assert any_ref(orc, t)[1] == cell, (shape, cell)


def test_tie_inputs_are_ties(orc):
    v = prefix_scores(orc, *SMALL["homo_5_9_140"], {})
    assert int(v.max()) == 15 and int((v == 15).sum()) == 680
    for name, want in SMALL_ANY.items():
        assert any_ref(orc, SMALL[name]) == want, name
        s, end = face_ref(orc, SMALL[name])
        assert all(1 <= e <= len(q) for e, q in zip(end, SMALL[name]))
        assert any(e == len(q) for e, q in zip(end, SMALL[name]))
    a, b, c = _repeat()
    assert (len(a), len(b), len(c)) == (38, 19, 140)
    assert any_ref(orc, (a, b, c)) == (24, (8, 8, 8))
    # the copies of R further on reach 24 too: (8, 19, 136) among them
    assert int(orc.score(a[:8], b[:19], c[:136])) == 24
    # the unwrapped reference is the wrapped one: every planted cube stays inside 12 bits
    for shape in SHAPES:
        for t in planted(shape):
            r = orc.best_range(*t)
            assert -2048 <= r.bmin and r.bmax <= 2047


# ---- CPU: the interface ---------------------------------------------------------------

NEW = ("tsa_score_batch_ends", "tsa_score_ends_workspace_size", "tsa_score_batch_ends_async",
       "tsa_describe_score_ends_plan")


def test_exports(tsa):
    for name in NEW:
        assert name in tsa.EXPORTS and hasattr(tsa.lib(), name), name
    with open(os.path.join(ROOT, "include", "trialign.h")) as f:
        header = f.read()
    for name in NEW:
        assert f"int {name}(" in header
    assert all(callable(getattr(tsa, n)) for n in ("score_batch_ends", "score_ends_workspace_size",
                                                   "score_batch_ends_async", "describe_score_ends_plan"))


def _raw(tsa, seqs, offsets, n, p, end_mode, null=None):
    u8, i32, i64 = (ctypes.POINTER(t) for t in (ctypes.c_uint8, ctypes.c_int32, ctypes.c_int64))
    seqs = np.ascontiguousarray(seqs, np.uint8)
    offsets = np.ascontiguousarray(offsets, np.int64)
    m = max(abs(n), 1)
    out = dict(scores=np.zeros(m, np.int32), ends=np.zeros(3 * m, np.int32))
    arg = lambda k: None if k == null else out[k].ctypes.data_as(i32)
    return tsa.lib().tsa_score_batch_ends(seqs.ctypes.data_as(u8), offsets.ctypes.data_as(i64), n, ctypes.byref(p),
                                          end_mode, arg("scores"), arg("ends"), 0)


def test_argument_errors(tsa):
    """TSA_EINVAL, then TSA_ERANGE, then TSA_ENODEV, all before any device work."""
    p = tsa.TsaParams.default()
    seqs, offs = tsa.pack_batch([([0, 1], [1, 2], [2, 3]), ([0], [1], [2])])
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
    # refused requests are TSA_ERANGE on any host: literal-only parameters, LC = 257
    lit = tsa.TsaParams.default(gap_open=1, gap_extend=2)
    long_c = tsa.pack_batch([([0, 1], [1, 2], [2] * 257)])
    for mode in (1, 2):
        assert _raw(tsa, seqs, offs, 2, lit, mode) == tsa.TSA_ERANGE
        assert _raw(tsa, *long_c, 1, p, mode) == tsa.TSA_ERANGE
        with tsa.overrides(pencil_arith="i16"):
            assert _raw(tsa, seqs, offs, 2, p, mode) == tsa.TSA_ERANGE
        with tsa.overrides(pencil_mode="lap"):
            assert _raw(tsa, seqs, offs, 2, p, mode) == tsa.TSA_EINVAL
        with tsa.overrides(pencil_mode="helix", pencil_two="1"):
            assert _raw(tsa, seqs, offs, 2, p, mode) == beyond
    for end in ("middle", 3, None):
        with pytest.raises(tsa.TsaError) as e:
            tsa.score_batch_ends([([0], [1], [2])], end=end)
        assert e.value.rc == tsa.TSA_EINVAL
    assert tsa.score_batch_ends([], end="face") == []


def test_plan_table(tsa):
    d = tsa.describe_score_ends_plan
    for mode in MODES:
        text = d(512, 256, 256, 256, end=mode)
        assert text.startswith("pencil helix f16v") and text.endswith(f" int ends={mode}"), text
        assert " lap " not in text and " two" not in text
        # LC <= 64: still one triple per wave, whatever pencil_two says
        assert " two" not in d(512, 64, 64, 64, end=mode)
        with tsa.overrides(pencil_two="1"):
            assert " two" not in d(512, 64, 64, 64, end=mode)
        # one large cube: the score plan is the lap schedule, the end search stays on the helix
        assert d(1, 256, 256, 256, end=mode).startswith("pencil helix")
        for kw, shape in ((dict(), (256, 256, 257)), (dict(gap_open=1, gap_extend=2), (64, 64, 64)),
                          (dict(), (2000, 2000, 256)), (dict(), (64, 2049, 64)),
                          # f16-class by its range, but row 2049 is lap 256: past the key's 8 bits
                          (dict(match=0), (64, 2049, 64))):
            with pytest.raises(tsa.TsaError) as e:
                d(4, *shape, params=tsa.TsaParams.default(**kw), end=mode)
            assert e.value.rc == tsa.TSA_ERANGE, (kw, shape)
        assert d(4, 64, 2048, 64, params=tsa.TsaParams.default(match=0), end=mode).startswith("pencil helix f16")
        with tsa.overrides(pencil_arith="i16"):
            with pytest.raises(tsa.TsaError) as e:
                d(4, 64, 64, 64, end=mode)
            assert e.value.rc == tsa.TSA_ERANGE
        for arith, want in (("f16vf", "pencil helix f16v rtl M=2 NW=8 P=256 ends="),
                            ("f16", "pencil helix f16 rtl M=2 NW=8 P=256 ends=")):
            with tsa.overrides(pencil_arith=arith):
                assert d(4, 256, 256, 256, end=mode).startswith(want + mode)
        with tsa.overrides(pencil_mode="lap"):
            with pytest.raises(tsa.TsaError) as e:
                d(4, 64, 64, 64, end=mode)
            assert e.value.rc == tsa.TSA_EINVAL
        # a parameter set that leaves V-space
        assert d(4, 40, 19, 140, params=tsa.TsaParams.default(match=2, mismatch=0), end=mode).startswith(
            "pencil helix f16 rtl M=2")
    for shape in ((256, 256, 256), (64, 64, 64), (40, 19, 140)):
        assert d(512, *shape, end="corner") == tsa.describe_plan(512, *shape)
    with pytest.raises(tsa.TsaError) as e:
        d(4, 64, 64, 64, end=3)
    assert e.value.rc == tsa.TSA_EINVAL


def test_beyond_the_f16_flip_is_refused(tsa):
    """The LL256 cube at which tsa_score_batch's plan leaves the f16 class for
    int16 (tests/_range_cases.py: plan_token) is the first one refused."""
    from _range_cases import SETS, SHAPES as RSHAPES, plan_token
    p = tsa.TsaParams.default(score_bits=16, **SETS["default"])   # 16-bit words: the int16 form takes over
    lo, hi = 256, 2048                       # f16-class at lo, int16 at hi
    assert plan_token(tsa, 512, RSHAPES["LL256"](lo), p).startswith("f16")
    assert plan_token(tsa, 512, RSHAPES["LL256"](hi), p) == "i16"
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if plan_token(tsa, 512, RSHAPES["LL256"](mid), p).startswith("f16") else (lo, mid)
    for mode in MODES:
        assert tsa.describe_score_ends_plan(512, *RSHAPES["LL256"](lo), p, end=mode).startswith("pencil helix f16")
        with pytest.raises(tsa.TsaError) as e:
            tsa.describe_score_ends_plan(512, *RSHAPES["LL256"](hi), p, end=mode)
        assert e.value.rc == tsa.TSA_ERANGE


def test_workspace_size(tsa):
    for mode in MODES:
        for n, shape in ((512, (256, 256, 256)), (70000, (100, 40, 200)), (300, (40, 19, 140))):
            assert "helix" in tsa.describe_plan(n, *shape, kernel="pencil", sync=False)
            assert tsa.score_ends_workspace_size(n, *shape, end=mode) == tsa.workspace_size(n, *shape, kernel="pencil")
    assert tsa.score_ends_workspace_size(8, 64, 64, 64, end="corner") == tsa.workspace_size(8, 64, 64, 64)
    with pytest.raises(tsa.TsaError) as e:
        tsa.score_ends_workspace_size(8, 64, 64, 300)
    assert e.value.rc == tsa.TSA_ERANGE


def test_cli_score_end_option():
    """--score-end is parsed: a bad value, a missing one, or --align, --kernel or
    --states with it is a usage error (exit 2), --end without --align stays one; a good one prints the
    score and the end cell, or gets as far as the device."""
    cli = os.path.join(PKG_DIR, "bin", "tsa")
    dat = os.path.join(ROOT, "tests", "golden", "dat")
    files = [f"{dat}/A_seq.dat", f"{dat}/B_seq.dat", f"{dat}/C_seq.dat"]
    run = lambda *extra: subprocess.run([cli, *files, *extra], capture_output=True, text=True)
    assert run("--score-end", "middle").returncode == 2
    assert run("--score-end", "corner").returncode == 2
    assert run("--score-end").returncode == 2
    assert run("--align", "--score-end", "any").returncode == 2
    assert run("--score-end", "any", "--align", "--end", "any").returncode == 2
    assert run("--end", "any").returncode == 2
    assert run("--score-end", "any", "--kernel", "pencil").returncode == 2   # the plan is always the helix
    assert run("--score-end", "any", "--states").returncode == 2
    for end in ("face", "any"):
        r = run("--score-end", end)
        if r.returncode == 0:
            lines = r.stdout.splitlines()
            assert lines[0].startswith("TriAlign Score:") and lines[1].startswith("end (x1,y1,z1) = (")
            assert "alignment" not in r.stdout
        else:
            assert r.returncode == 1 and "no HIP device" in r.stderr and "usage" not in r.stderr


# ---- CPU: the kernel's fold, replayed (tools/pencil_emu.py) ---------------------------

FORMS = {"msg": dict(), "vs": dict(vs=True), "read_prev": dict(vs=True, read_prev=True),
         "int": dict(vs=True, read_prev=True, int_bits=True)}


def planted_name(shape, cell):
    return f"{'x'.join(map(str, shape))}@{'.'.join(map(str, cell))}"


PLANTED_INPUTS = {planted_name(shape, cell): t for shape in SHAPES for cell, t in zip(PLANTED[shape], planted(shape))}
EMU_INPUTS = dict(PLANTED_INPUTS)
EMU_INPUTS.update(SMALL)
EMU_INPUTS["repeat"] = _repeat()
# the integer cell is the M = 2 helix's: paired with the inputs of LC > 128 alone
EMU_CASES = [(name, form) for name, t in EMU_INPUTS.items() for form in FORMS if form != "int" or len(t[2]) > 128]
# the small triples as a ragged batch runs them: the geometry of the batch's maxima
RAGGED_MAX = tuple(max(len(t[k]) for t in ragged_batch()) for k in range(3))
RAGGED_CASES = [(name, form) for name in SMALL for form in FORMS]


def face_brute(orc, t):
    """(score, end) of the face mode by brute force over the face cells alone:
    oracle.score of the prefixes a[:x], b[:y], c[:z] with x = la or y = lb or
    z = lc, the first best one in (x, y, z) order. Seconds on 40 x 19 x 140,
    a minute on 261 x 11 x 130 (38 k prefixes), so the planted cubes' results
    are recorded in tests/golden/score_ends_face.json."""
    a, b, c = t
    la, lb, lc = len(a), len(b), len(c)
    cells = sorted({(la, y, z) for y in range(1, lb + 1) for z in range(1, lc + 1)} |
                   {(x, lb, z) for x in range(1, la + 1) for z in range(1, lc + 1)} |
                   {(x, y, lc) for x in range(1, la + 1) for y in range(1, lb + 1)})
    parts, offs = [], [0]
    for x, y, z in cells:
        parts += [a[:x], b[:y], c[:z]]
        offs += [offs[-1] + x, offs[-1] + x + y, offs[-1] + x + y + z]
    v = np.asarray(orc.score_batch(np.concatenate(parts), np.asarray(offs, np.int64), orc.default_params(),
                                   nthreads=min(8, os.cpu_count() or 1)))
    i = int(np.argmax(v))
    return int(v[i]), cells[i]


_FACE = {}


def planted_face_ref(name):
    if not _FACE:
        with open(os.path.join(ROOT, "tests", "golden", "score_ends_face.json")) as f:
            _FACE.update({k: (int(s), tuple(e)) for k, (s, e) in json.load(f).items()})
    return _FACE[name]


def emu_face_ref(orc, name):
    if name in SMALL:
        return face_ref(orc, SMALL[name])
    if name == "repeat":
        if name not in _FACE:
            _FACE[name] = face_brute(orc, EMU_INPUTS[name])
        return _FACE[name]
    return planted_face_ref(name)


def _emu():
    import sys
    tools = os.path.join(ROOT, "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import pencil_emu
    return pencil_emu


def test_recorded_face_references_are_the_brute_force(orc):
    """The recorded file names every planted cube, and the brute force gives
    the same on the cubes where it takes seconds; it agrees with the full
    prefix brute force of tests/test_align_ends.py on a small cube."""
    assert all(planted_face_ref(name) for name in PLANTED_INPUTS) and set(_FACE) >= set(PLANTED_INPUTS)
    for name in list(PLANTED_INPUTS)[:2]:
        assert face_brute(orc, PLANTED_INPUTS[name]) == planted_face_ref(name), name
    for name in ("homo_5_9_140", "ragged3"):
        assert face_brute(orc, SMALL[name]) == face_ref(orc, SMALL[name]), name
    for name, t in PLANTED_INPUTS.items():        # a face cell; never above the any score
        s, e = planted_face_ref(name)
        assert any(x == len(q) for x, q in zip(e, t)) and s <= any_ref(orc, t)[0]


@pytest.mark.parametrize("name,form", EMU_CASES)
def test_replay_matches_the_references(orc, name, form):
    """The fold as the kernel does it -- per position slot, per wave, across the
    waves -- on records and a ring that start as garbage. any: the oracle's
    (bmax, at_max). face: the prefix brute force (recorded for the planted cubes)."""
    t = EMU_INPUTS[name]
    got_any, got_face = _emu().emulate([t], end=("any", "face"), garbage_seed=3, ring_garbage_seed=4, **FORMS[form])
    assert got_any == any_ref(orc, t), (name, form)
    assert got_face == emu_face_ref(orc, name), (name, form)


@pytest.mark.parametrize("name,form", RAGGED_CASES)
def test_replay_in_a_ragged_batch(orc, name, form):
    """A short triple inside the cube of a batch's maxima (M = 2, P = 256, the
    bias of the large cube): every padding cell in x, y and z is computed and
    must be masked."""
    assert RAGGED_MAX == (140, 19, 140)
    t = SMALL[name]
    got_any, got_face = _emu().emulate([t], end=("any", "face"), garbage_seed=5, ring_garbage_seed=6,
                                       max_lens=RAGGED_MAX, **FORMS[form])
    assert got_any == any_ref(orc, t), (name, form)
    assert got_face == face_ref(orc, t), (name, form)


def test_replay_fold_is_order_free(orc):
    """Folding the same candidates in any order gives the same key: the key
    orders cells by (score, x, y, z), not by the sweep."""
    pe = _emu()
    rng = np.random.default_rng(5)
    for t in (SMALL["homo_5_9_140"], _repeat()):
        ev = {"end_cands": []}
        res = pe.emulate([t], end=("any", "face"), events=ev, vs=True)
        for mode, got in zip(("any", "face"), res):
            cands = [c for c in ev["end_cands"] if c[0] == mode]
            assert len(cands) > 1000
            for _ in range(3):
                slot = {}
                for j in rng.permutation(len(cands)):
                    _, w, i, l, h, key = cands[j]
                    slot[(w, i, l, h)] = max(slot.get((w, i, l, h), 0), key)
                M = 2 if len(t[2]) > 128 else 1
                keys = [pe.end_key64(key, w, 64 * M * h + M * l + i) for (w, i, l, h), key in slot.items()
                        if 64 * M * h + M * l + i < len(t[2]) and key]
                assert max(keys) == ev["end_key"][mode] and pe.end_decode(max(keys)) == got
    # first in time is not first in (x, y, z): the homopolymer's winner is not the first cell to reach 15
    assert any_ref(orc, SMALL["homo_140_9_5"]) == (15, (5, 5, 5))


# ---- GPU ---------------------------------------------------------------------------------

def _check_batch(gpu, orc, trips, mode, params=None):
    """Equal to the literal traceback kernels' score and end, and under any (default parameters) to the oracle."""
    got = gpu.score_batch_ends(trips, params, end=mode)
    lit = gpu.align_batch_ends(trips, params, end=mode)
    for i, (t, g, l) in enumerate(zip(trips, got, lit)):
        assert g == (l[0], tuple(l[3])), (mode, i, g, (l[0], l[3]))
        if mode == "any" and params is None:
            assert g == any_ref(orc, t), (mode, i)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES)
def test_gpu_planted_match_the_references(gpu, orc, shape, mode):
    n = len(PLANTED[shape])
    text = gpu.describe_score_ends_plan(n, *shape, end=mode)
    assert text.startswith(f"pencil helix f16v rtl M={2 if shape[2] > 128 else 1} NW=8") and text.endswith(f"ends={mode}")
    got = _check_batch(gpu, orc, planted(shape), mode)
    if mode == "any":
        assert [e for _, e in got] == list(PLANTED[shape])
    else:
        assert got == [planted_face_ref(planted_name(shape, cell)) for cell in PLANTED[shape]]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_gpu_ties_ones_and_a_ragged_batch(gpu, orc, mode):
    trips = ragged_batch()
    got = _check_batch(gpu, orc, trips, mode)
    names = list(SMALL)
    for name, g in zip(names, got[1:1 + len(names)]):
        assert g == small_ref(orc, name, mode), (name, mode)
    if mode == "any":
        for name, want in SMALL_ANY.items():
            assert got[1 + names.index(name)] == want
        assert got[1 + len(names)] == (24, (8, 8, 8))
    # every small triple alone: max_l* are its own lengths
    for name in names:
        assert gpu.score_batch_ends([SMALL[name]], end=mode) == [small_ref(orc, name, mode)], name


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("arith,word", [("f16vi", "f16v"), ("f16vf", "f16v"), ("f16", "f16")])
def test_gpu_arithmetic_forms(gpu, orc, arith, word, mode):
    for shape in SHAPES:
        if arith == "f16vi" and shape[2] <= 128:
            continue  # the integer cell is the M = 2 helix's
        with gpu.overrides(pencil_arith=arith):
            text = gpu.describe_score_ends_plan(len(PLANTED[shape]), *shape, end=mode)
            assert text.startswith(f"pencil helix {word} rtl") and ((" int " in text) == (arith == "f16vi")), text
            _check_batch(gpu, orc, planted(shape), mode)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_gpu_sop_and_outside_v_space(gpu, orc, mode):
    sop = gpu.TsaParams.default(s3_mode=1)
    flat = gpu.TsaParams.default(match=2, mismatch=0)
    for shape in SHAPES:
        n = len(PLANTED[shape])
        assert gpu.describe_score_ends_plan(n, *shape, params=sop, end=mode).startswith("pencil helix f16v sop")
        _check_batch(gpu, orc, planted(shape), mode, sop)
        assert gpu.describe_score_ends_plan(n, *shape, params=flat, end=mode).startswith("pencil helix f16 rtl")
        _check_batch(gpu, orc, planted(shape), mode, flat)
    _check_batch(gpu, orc, ragged_batch(), mode, sop)
    _check_batch(gpu, orc, ragged_batch(), mode, flat)


@pytest.mark.gpu
def test_gpu_corner_is_score_batch(gpu):
    trips = ragged_batch() + planted(SHAPES[1])
    got = gpu.score_batch_ends(trips, end="corner")
    assert [s for s, _ in got] == list(gpu.score_batch(trips))
    assert [e for _, e in got] == [tuple(len(s) for s in t) for t in trips]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_gpu_prefixes_compose_with_the_traceback(gpu, mode):
    trips = planted(SHAPES[0])[:4] + ragged_batch()
    ends = gpu.score_batch_ends(trips, end=mode)
    cut = [tuple(s[:e] for s, e in zip(t, end)) for t, (_, end) in zip(trips, ends)]
    whole = gpu.align_batch_ends(trips, end=mode)
    for (s, end), (s1, st1, mv1), (s2, st2, mv2, end2) in zip(ends, gpu.align_batch(cut), whole):
        assert (s, end) == (s2, tuple(end2)) and s1 == s
        assert tuple(st1) == tuple(st2) and np.array_equal(mv1, mv2)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_gpu_async(gpu, orc, mode):
    import torch
    trips = planted(SHAPES[0])
    seqs, offs = gpu.pack_batch(trips)
    n = len(trips)
    dev = torch.device("cuda:0")
    d_seqs = torch.from_numpy(seqs).to(dev)
    d_offs = torch.from_numpy(offs).to(dev)
    shape = SHAPES[0]
    need = gpu.score_ends_workspace_size(n, *shape, end=mode)
    ws = torch.full((need,), 0xEE, dtype=torch.uint8, device=dev)
    d_scores = torch.full((n,), -7, dtype=torch.int32, device=dev)
    d_ends = torch.full((3 * n,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    before = gpu.kernel_launch_count()
    with pytest.raises(gpu.TsaError) as e:
        gpu.score_batch_ends_async(d_seqs.data_ptr(), d_offs.data_ptr(), n, *shape, d_scores.data_ptr(),
                                   d_ends.data_ptr(), ws.data_ptr(), need - 1, stream, end=mode)
    assert e.value.rc == gpu.TSA_ENOMEM and gpu.kernel_launch_count() == before
    torch.cuda.synchronize()
    assert int((d_scores != -7).sum()) == 0 and int((d_ends != -7).sum()) == 0
    gpu.score_batch_ends_async(d_seqs.data_ptr(), d_offs.data_ptr(), n, *shape, d_scores.data_ptr(),
                               d_ends.data_ptr(), ws.data_ptr(), need, stream, end=mode)
    assert gpu.kernel_launch_count() == before + 1
    torch.cuda.synchronize()
    assert d_scores.is_cuda and d_ends.is_cuda
    got = list(zip(d_scores.cpu().tolist(), (tuple(r) for r in d_ends.cpu().view(-1, 3).tolist())))
    assert got == gpu.score_batch_ends(trips, end=mode)
    if mode == "any":
        assert got == [any_ref(orc, t) for t in trips]
