"""The range proof of DESIGN.md 1.2 at its admission edges, on the CPU.

Every fast scoring path is chosen by an a-priori argument on the host
(value_bound / bound_drops, pencil_exact, pencil_checkable and tsa_validate in
csrc/trialign_api.hip; pencil_slack, use_f16, use_vs, use_vi and lap_vs_ok in
csrc/pencil_kernel.hip). A predicate that is off by one returns a wrong score
with no error, and only at the largest shape it admits, on inputs that drive
the values to the end of the proven range. These tests go there. The library's
predicates are consulted through describe_plan and validate alone (never
through the Python copy in tools/pencil_emu.py); what the values really do
comes from the oracle's candidate_range: the 49 pre-MAX sums of every real cell,
which are what the RTL wraps, and every state, in unbounded arithmetic.

  * the flip table: the first size at which the plan's arithmetic changes, for
    every parameter set below, pinned. A change of a predicate must show as an
    edit of FLIPS (and of the rows of tests/test_range_edges_gpu.py).
  * word soundness: at the largest admitted shape no candidate leaves the word.
  * exhaustive soundness at la + lb + lc <= 6.
  * carrier soundness and tightness at the upper end: on the last size an
    arithmetic is admitted, the extreme input's range widened by the slack of
    DESIGN.md 1.2 fits the carrier; on the first size it is refused, it does
    not. The lower end of value_bound is conservative by construction (the
    all-distinct 12^3 cube reaches about 60 % of it), so only soundness is
    asserted there.
  * slack: every intermediate of the message form and of the V-space form
    (tools/pencil_emu.py) stays within the candidate range widened by the slack.
  * tsa_validate at score_bits = 0: int16 state storage.
"""
import concurrent.futures
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import pencil_emu  # noqa: E402
from _range_cases import FAMILIES, SETS, SHAPES, family, plan_token  # noqa: E402

# The first size L at which describe_plan(n, shape(L), "pencil", sync=False)
# changes its arithmetic, under pencil_mode = helix (n = 3) or lap (n = 1):
# "f16" exact f16, "f16v" the V-space f16 cell, "f16v int" the integer-pattern
# cell, "i16" int16, "refused" TSA_ERANGE. Shapes: "cube" (L, L, L), "L8L"
# (L, 8, L), "LL256" (L, L, 256). Under lap the smallest shapes have no lap
# schedule and show the helix's plan (f16v). Regenerate with _flips() below.
FLIPS = {
    ("helix", "default", "cube"): [(1, "f16v"), (129, "f16v int"), (257, "f16"), (675, "i16"), (681, "refused")],
    ("helix", "default", "L8L"): [(1, "f16v"), (129, "f16v int"), (257, "f16"), (1013, "i16"), (1020, "refused")],
    ("helix", "m2_mm0", "cube"): [(1, "f16"), (338, "i16"), (342, "refused")],
    ("helix", "m2_mm0", "L8L"): [(1, "f16"), (503, "i16"), (508, "refused")],
    ("helix", "m3_mm1_b16", "cube"): [(1, "f16"), (225, "i16")],
    ("helix", "m3_mm1_b16", "L8L"): [(1, "f16"), (333, "i16")],
    ("helix", "m40_b16", "cube"): [(1, "i16"), (271, "refused")],
    ("helix", "m40_b16", "L8L"): [(1, "i16"), (402, "refused")],
    ("helix", "m40_b0", "cube"): [(1, "i16"), (271, "refused")],
    ("helix", "m40_b0", "L8L"): [(1, "i16"), (402, "refused")],
    ("helix", "m10_mm8", "cube"): [(1, "i16"), (57, "refused")],
    ("helix", "m10_mm8", "L8L"): [(1, "i16"), (82, "refused")],
    ("helix", "lam2_b16", "cube"): [(1, "f16v"), (129, "f16v int"), (257, "f16"), (335, "i16")],
    ("helix", "lam2_b16", "L8L"): [(1, "f16v"), (129, "f16v int"), (257, "f16")],
    ("helix", "lam3_b16", "cube"): [(1, "f16v"), (129, "f16v int"), (168, "f16v"), (222, "i16")],
    ("helix", "lam3_b16", "L8L"): [(1, "f16v"), (129, "f16v int"), (257, "f16")],
    ("helix", "b9", "cube"): [(1, "f16v"), (83, "refused")],
    ("helix", "b9", "L8L"): [(1, "f16v"), (124, "refused")],
    ("helix", "b8", "cube"): [(1, "f16v"), (41, "refused")],
    ("helix", "b8", "L8L"): [(1, "f16v"), (60, "refused")],
    ("helix", "b6", "cube"): [(1, "f16v"), (9, "refused")],
    ("helix", "b6", "L8L"): [(1, "f16v"), (12, "refused")],
    ("helix", "default", "LL256"): [(1, "f16v int"), (381, "f16"), (889, "i16"), (896, "refused")],
    ("helix", "lam2_b16", "LL256"): [(1, "f16v int"), (378, "f16")],
    ("lap", "default", "cube"): [(1, "f16v"), (9, "f16"), (675, "i16"), (681, "refused")],
    ("lap", "default", "L8L"): [(1, "f16v"), (65, "f16"), (1013, "i16"), (1020, "refused")],
    ("lap", "m2_mm0", "cube"): [(1, "f16"), (338, "i16"), (342, "refused")],
    ("lap", "m2_mm0", "L8L"): [(1, "f16"), (503, "i16"), (508, "refused")],
    ("lap", "m3_mm1_b16", "cube"): [(1, "f16"), (225, "i16")],
    ("lap", "m3_mm1_b16", "L8L"): [(1, "f16"), (333, "i16")],
    ("lap", "m40_b16", "cube"): [(1, "i16"), (271, "refused")],
    ("lap", "m40_b16", "L8L"): [(1, "i16"), (402, "refused")],
    ("lap", "m40_b0", "cube"): [(1, "i16"), (271, "refused")],
    ("lap", "m40_b0", "L8L"): [(1, "i16"), (402, "refused")],
    ("lap", "m10_mm8", "cube"): [(1, "i16"), (57, "refused")],
    ("lap", "m10_mm8", "L8L"): [(1, "i16"), (82, "refused")],
    ("lap", "lam2_b16", "cube"): [(1, "f16v"), (9, "f16"), (335, "i16")],
    ("lap", "lam2_b16", "L8L"): [(1, "f16v"), (65, "f16")],
    ("lap", "lam3_b16", "cube"): [(1, "f16v"), (9, "f16"), (222, "i16")],
    ("lap", "lam3_b16", "L8L"): [(1, "f16v"), (65, "f16")],
    ("lap", "b9", "cube"): [(1, "f16v"), (9, "f16"), (83, "refused")],
    ("lap", "b9", "L8L"): [(1, "f16v"), (65, "f16"), (124, "refused")],
    ("lap", "b8", "cube"): [(1, "f16v"), (9, "f16"), (41, "refused")],
    ("lap", "b8", "L8L"): [(1, "f16v"), (60, "refused")],
    ("lap", "b6", "cube"): [(1, "f16v"), (9, "refused")],
    ("lap", "b6", "L8L"): [(1, "f16v"), (12, "refused")],
}
# the opt-in V-space cell of the lap kernel (override lap_vs = 1), cubes, n = 1
FLIPS_LAP_VS = {
    "default": [(1, "f16v"), (339, "f16"), (675, "i16"), (681, "refused")],
    "lam2_b16": [(1, "f16v"), (335, "i16")],
}
# tsa_validate at score_bits = 0, match 40, mismatch -1: the first cube side with TSA_ERANGE
VALIDATE_FLIP = 274
SCAN_MAX = {"cube": 1000, "L8L": 1024, "LL256": 1200}
def _flips(tsa, n, shape, p, lmax):
    out = []
    for L in range(1, lmax + 1):
        t = plan_token(tsa, n, shape(L), p)
        if not out or t != out[-1][1]:
            out.append((L, t))
    return out


def _first(tsa, name, shape, token, mode="helix"):
    """The first size of FLIPS' row at which the plan reads `token` (the row
    itself is checked against the library by test_flip_table)."""
    return next(L for L, t in FLIPS[(mode, name, shape)] if t == token)


def _slack(kw):
    """The slack of DESIGN.md 1.2 restated: 8 max|score| + 4 max|penalty|."""
    g = lambda k, d: kw.get(k, d)  # noqa: E731
    return 8 * max(abs(g("match", 1)), abs(g("mismatch", -1))) + 4 * max(abs(g("gap_open", 2)), abs(g("gap_extend", 1)))


def _word(bits):
    return -(1 << (bits - 1)), (1 << (bits - 1)) - 1


_POOL = concurrent.futures.ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1))
_CR = {}


def ranges(orc, jobs):
    """candidate_range of each (set name, family, dims), the large cubes side by
    side on the cores (the oracle releases the interpreter), each computed once
    for the module."""
    todo = [j for j in dict.fromkeys(jobs) if j not in _CR]

    def one(job):
        name, kind, dims = job
        return orc.candidate_range(*family(kind, dims), orc.default_params(**SETS[name]))
    for job, r in zip(todo, _POOL.map(one, todo)):
        _CR[job] = r
    return [_CR[j] for j in jobs]


@pytest.mark.parametrize("mode", ("helix", "lap"))
def test_flip_table(tsa, mode):
    """FLIPS against a fresh scan of every size up to SCAN_MAX."""
    tsa.set_override("pencil_mode", mode)
    n = 3 if mode == "helix" else 1
    seen = 0
    for (m, name, shape), want in FLIPS.items():
        if m != mode:
            continue
        got = _flips(tsa, n, SHAPES[shape], tsa.TsaParams.default(**SETS[name]), SCAN_MAX[shape])
        assert got == want, (mode, name, shape, got)
        seen += 1
    assert seen == (24 if mode == "helix" else 22)
    if mode == "lap":
        tsa.set_override("lap_vs", 1)
        for name, want in FLIPS_LAP_VS.items():
            got = _flips(tsa, 1, SHAPES["cube"], tsa.TsaParams.default(**SETS[name]), SCAN_MAX["cube"])
            assert got == want, ("lap_vs", name, got)


def test_validate_flip(tsa):
    p = tsa.TsaParams.default(**SETS["m40_b0"])
    rcs = []
    for L in range(1, 400):
        z = np.zeros(L, np.uint8)
        rcs.append(tsa.validate(z, z, z, p))
    assert rcs == [tsa.TSA_OK] * (VALIDATE_FLIP - 1) + [tsa.TSA_ERANGE] * (400 - VALIDATE_FLIP)
    # the literal kernels own the cubes between the pencil's last (270) and validate's last (273)
    assert _first(tsa, "m40_b0", "cube", "refused") == 271 < VALIDATE_FLIP


# (set, shape kinds): the largest shape of each kind at which kernel="pencil" is
# admitted. The default set's 680-cube (10^8.5 cells, seven families, three
# sweeps each) is too slow for this suite: its row has the skewed shape alone,
# (1019, 8, 1019), whose coordinate sum 2046 is the largest the 12-bit word
# admits. That reaches the PREDICATE at its edge but not the VALUE: with a
# shortest length of 8 no input comes near 2047 (the 680-cube's edge is the
# lower end, -3 * 680 - 8 = -2048, which no input reaches either, see above).
WORD_ROWS = [("b9", ("cube", "L8L")), ("b8", ("cube", "L8L")), ("b6", ("cube", "L8L")),
             ("m2_mm0", ("cube", "L8L")), ("m10_mm8", ("cube", "L8L")), ("default", ("L8L",))]


@pytest.mark.parametrize("name,shapes", WORD_ROWS, ids=[r[0] for r in WORD_ROWS])
def test_word_soundness(tsa, orc, name, shapes):
    """At the largest admitted shape, for every input family: no candidate of
    the unwrapped recurrence leaves the score_bits word, and the literal result
    at score_bits equals the one at score_bits = 0, score and final states."""
    kw = SETS[name]
    bits = kw.get("score_bits", 12)
    lo, hi = _word(bits)
    p = tsa.TsaParams.default(**kw)
    for shape in shapes:
        L = _first(tsa, name, shape, "refused") - 1
        dims = SHAPES[shape](L)
        assert plan_token(tsa, 1, dims, p) != "refused" and plan_token(tsa, 1, SHAPES[shape](L + 1), p) == "refused"
        got = ranges(orc, [(name, kind, dims) for kind in FAMILIES])

        def literal(job):
            kind, b = job
            return orc.score(*family(kind, dims), orc.default_params(**{**kw, "score_bits": b}), final_states=True)
        lit = list(_POOL.map(literal, [(kind, b) for kind in FAMILIES for b in (bits, 0)]))
        for i, (kind, r) in enumerate(zip(FAMILIES, got)):
            print(name, dims, kind, "candidates", (r.lo, r.hi), "at", r.at_lo, r.at_hi, "word", (lo, hi))
            assert lo <= r.lo and r.hi <= hi, (name, dims, kind, r)
            assert lit[2 * i] == lit[2 * i + 1], (name, dims, kind)


# (match, mismatch, GO, GE, s3_mode): scores scaled up to 40, GO = GE, zero
# penalties, negative matches, both s3 modes; GO >= GE throughout (the pencil
# is not supported otherwise)
GRID = [(1, -1, 2, 1, 0), (1, -1, 2, 1, 1), (2, 0, 2, 1, 0), (3, 1, 2, 1, 1), (40, -1, 2, 1, 0), (40, -40, 40, 20, 1),
        (10, 8, 2, 1, 0), (10, 8, 5, 5, 1), (0, -2, 3, 2, 0), (-1, -3, 4, 3, 1), (-5, -6, 7, 7, 0), (7, -3, 0, 0, 1),
        (-40, 40, 40, 1, 0)]
SMALL = [(la, lb, lc) for la in range(1, 5) for lb in range(1, 5) for lc in range(1, 5) if la + lb + lc <= 6]


@pytest.mark.parametrize("pset", GRID, ids=lambda s: "m%d_mm%d_go%d_ge%d_s%d" % s)
def test_exhaustive_small_shapes(tsa, orc, pset):
    """All 4^(la+lb+lc) triples of every shape with la + lb + lc <= 6: at the
    smallest score_bits in 4..16 that admits the pencil, no triple's candidates
    leave the word."""
    m, mm, go, ge, s3 = pset
    kw = dict(match=m, mismatch=mm, gap_open=go, gap_extend=ge, s3_mode=s3)
    admitted = 0
    for dims in SMALL:
        bits = next((b for b in range(4, 17)
                     if plan_token(tsa, 1, dims, tsa.TsaParams.default(score_bits=b, **kw)) != "refused"), None)
        if bits is None:  # the bound leaves even the 16-bit word: nothing is promised
            continue
        admitted += 1
        lo, hi, ilo, ihi = orc.candidate_range_all(*dims, orc.default_params(**kw))
        wlo, whi = _word(bits)
        assert wlo <= lo and hi <= whi, (pset, dims, bits, (lo, hi), orc.triple_number(ilo, *dims),
                                         orc.triple_number(ihi, *dims))
    assert admitted == len(SMALL), (pset, admitted)


# (set, family, arithmetic left, arithmetic entered, carrier limits, slack applies):
# the upper-end edges that a simple input reaches. f16 holds integers up to
# 2048 exactly and int16 up to 32767, both for the range widened by the slack;
# the word itself must hold the bare candidates.
TOPS = [("m2_mm0", "all-match", "f16", "i16", (-2048, 2048), True),
        ("m2_mm0", "all-match", "i16", "refused", (-2048, 2047), False),
        ("m3_mm1_b16", "all-match", "f16", "i16", (-2048, 2048), True),
        ("m40_b16", "all-match", "i16", "refused", (-32768, 32767), True),
        # RTL s3: a = b != c scores 2 (m + mm) = 36 > 3 m = 30 a cell, the quirk of src/PE_1cyc.v:162
        ("m10_mm8", "a=b", "i16", "refused", (-2048, 2047), False)]


def test_upper_end_is_sound_and_tight(tsa, orc):
    """On the last cube an arithmetic is admitted, the extreme family's
    candidates (widened by the slack where the limit is a carrier's) fit; on
    the first cube it is refused their top, widened the same way, exceeds the
    limit, so the edge the GPU rows test is not a loose one. Lower end:
    soundness only (value_bound's lower end is conservative by construction)."""
    rows = [(name, kind, _first(tsa, name, "cube", new)) for name, kind, _, new, _, _ in TOPS]
    got = ranges(orc, [(name, kind, (L + d,) * 3) for name, kind, L in rows for d in (-1, 0)])
    for i, (name, kind, old, new, limit, slacked) in enumerate(TOPS):
        L = rows[i][2]
        p = tsa.TsaParams.default(**SETS[name])
        tsa.set_override("pencil_mode", "helix")
        assert (plan_token(tsa, 3, (L - 1,) * 3, p), plan_token(tsa, 3, (L,) * 3, p)) == (old, new)
        s = _slack(SETS[name]) if slacked else 0
        last, first = got[2 * i], got[2 * i + 1]
        print(name, kind, L, "last admitted", (last.lo, last.hi), "first refused", (first.lo, first.hi), "slack", s)
        assert limit[0] <= last.lo - s and last.hi + s <= limit[1], (name, L - 1, last, s, limit)
        assert first.hi + s > limit[1], (name, L, first, s, limit)


def test_validate_int16_storage(tsa, orc):
    """score_bits = 0: TSA_OK at the last admitted cube implies every family's
    candidates fit int16 (the literal kernels' state storage); the first
    refused cube's all-match candidates do not, so neither does its bound."""
    L = VALIDATE_FLIP
    p = tsa.TsaParams.default(**SETS["m40_b0"])
    z = np.zeros(L, np.uint8)
    assert tsa.validate(z[:-1], z[:-1], z[:-1], p) == tsa.TSA_OK and tsa.validate(z, z, z, p) == tsa.TSA_ERANGE
    got = ranges(orc, [("m40_b0", kind, (L - 1,) * 3) for kind in FAMILIES] + [("m40_b0", "all-match", (L,) * 3)])
    for kind, r in zip(FAMILIES, got):
        print("validate", L - 1, kind, (r.lo, r.hi))
        assert -32768 <= r.lo and r.hi <= 32767, (kind, r)
    assert got[0].hi == 32760 and got[-1].hi == 32880 > 32767


# (match, mismatch, GO, GE, sop): the scaled sets of the slack test; the V-space
# form runs where lam = GE = -mismatch >= 1
SLACK_SETS = [(1, -1, 2, 1, True), (2, 0, 2, 1, False), (3, 1, 2, 1, True), (40, -1, 2, 1, False), (10, 8, 2, 1, False),
              (0, -2, 3, 2, False), (-1, -3, 4, 3, True), (-5, -6, 7, 6, False), (5, -4, 3, 3, True)]
# a cube through a second lap of rows (LB > 8) with the three families that reach
# the ends, and a longer shape of one lap with every family
SLACK_CASES = [((12, 12, 12), ("all-match", "all-distinct", "a=b")),
               ((20, 8, 17), ("all-match", "all-distinct", "a=b", "b=c", "a=c", "random"))]


@pytest.mark.parametrize("pset", SLACK_SETS, ids=lambda s: "m%d_mm%d_go%d_ge%d_%s" % (s[:4] + ("sop" if s[4] else "rtl",)))
def test_intermediates_within_slack(orc, pset):
    """Every intermediate the message form and the V-space form hold at a real
    cell (tools/pencil_emu.py, events["range"]) lies within the triple's
    candidate range widened by the slack; the V-space values are shifted by
    lam (x + y + z), so their upper end also gets lam (la + lb + lc)."""
    m, mm, go, ge, sop = pset
    kw = dict(match=m, mismatch=mm, gap_open=go, gap_extend=ge)
    op = orc.default_params(s3_mode=int(sop), score_bits=0, **kw)
    s = _slack(kw)
    for dims, kinds in SLACK_CASES:
        for kind in kinds:
            a, b, c = family(kind, dims)
            r = orc.candidate_range(a, b, c, op)
            want = orc.score(a, b, c, op)
            forms = [dict(vs=False)] + ([dict(vs=True, read_prev=True)] if ge == -mm and ge >= 1 else [])
            for form in forms:
                ev = {"range": {}}
                got = pencil_emu.emulate([(a, b, c)], match=m, mismatch=mm, go=go, ge=ge, sop=sop, events=ev, **form)
                assert got == [want], (pset, dims, kind, form)
                lo = min(v[0] for v in ev["range"].values())
                hi = max(v[1] for v in ev["range"].values())
                lam_q = ge * sum(dims) if form["vs"] else 0
                print(pset, dims, kind, form, ev["range"], "candidates", (r.lo, r.hi), "slack", s)
                assert r.lo - s <= lo and hi <= r.hi + s + lam_q, (pset, dims, kind, form, ev["range"], r, s)
