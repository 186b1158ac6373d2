"""CPU oracle checks: the restatement against the reference-derived known
answers, the cycle-level RTL model, its own second traversal, and the
properties SURVEY.md 4 lists. TEST INFRASTRUCTURE ONLY (no product code)."""
import numpy as np
import pytest


def test_golden_fixtures(orc, golden):
    for c in golden:
        p = orc.default_params(**c["params"])
        s, fin = orc.score(c["a"], c["b"], c["c"], p, final_states=True)
        assert s == c["score"], c["name"]
        assert list(fin) == c["final7"], c["name"]
        assert orc.score(c["a"], c["b"], c["c"], p, method="diag") == c["score"], c["name"]


def test_testbench_known_answer(orc):
    # src/TriAlign_tb.sv:423-1960 loads all-A; every M step is +3, nothing else
    # is positive, so the 64^3 score is 3*64 (KAT 1).
    z = [0] * 64
    assert orc.score(z, z, z) == 192
    for n in (8, 16, 32, 48):
        assert orc.score([0] * n, [0] * n, [0] * n) == 3 * n


def test_dat_triple_and_survey_values(golden):
    by = {c["name"]: c for c in golden}
    assert by["dat"]["score"] == 1
    assert by["dat"]["final7"] == [-1, 1, -4, -5, 1, -7, -2]
    assert by["dat_prefix8"]["score"] == -3 and by["dat_prefix16"]["score"] == -5
    assert by["homopolymers_16"]["score"] == -32
    assert by["dat"]["rtl_model"]["score"] == 1


@pytest.mark.parametrize("seed", range(6))
def test_rtl_model_matches_restatement_in_envelope(orc, seed):
    rng = np.random.default_rng(seed)
    for _ in range(4):
        la = 8 * int(rng.integers(1, 9)); lb = 8 * int(rng.integers(1, la // 8 + 1)); lc = 8 * int(rng.integers(1, 9))
        a, b, c = (rng.integers(0, 5, n).astype(np.uint8) for n in (la, lb, lc))
        r, isx, _ = orc.rtl_run(a, b, c)
        assert not isx
        assert r == orc.score(a, b, c)


def test_rtl_model_long_pencil_ring(orc):
    # 128 x 64 x 40: 8 x 5 pencils, y-face ring wraps several times
    rng = np.random.default_rng(7)
    a, b, c = (rng.integers(0, 4, n).astype(np.uint8) for n in (128, 64, 40))
    r, isx, cyc = orc.rtl_run(a, b, c)
    assert not isx and r == orc.score(a, b, c)
    # cycle model of SURVEY.md 3(c), 1cyc controller: per pencil 65 load + LA+16 compute
    assert cyc == (64 // 8) * (40 // 8) * (65 + 128 + 16) + 1


def test_rtl2_model_testbench_and_dat(orc, golden):
    """The 2-cycle variant (oracle/rtl_model_2cyc.c) on the testbench's own
    input and the reference's dat triple: the same scores as the 1-cycle
    variant and the restatement."""
    z = [0] * 64
    r, isx, cyc = orc.rtl2_run(z, z, z)
    assert (r, isx) == (192, False)
    # per pencil 65 INITIAL clocks, then a COMPUTE + WAIT pair per step for
    # A_idx + 16 steps (src/TriAlign_2cyc.v:354-355,433-482)
    assert cyc == 64 * (65 + 2 * (64 + 16)) + 1
    by = {c["name"]: c for c in golden}
    assert by["dat"]["rtl2_model"] == {"score": 1, "x": False, "cycles": cyc, "agrees": True,
                                       "source": by["dat"]["rtl2_model"]["source"]}
    assert by["dat"]["rtl2_model"]["source"].startswith("model-derived")


def test_golden_rtl2_records(orc, golden, tsa):
    """golden.json records, for every default-parameter case the 2-cycle RTL
    can take, its model's score and whether it agrees with the restatement;
    agreement is exactly the 2-cycle envelope (rtl_envelope(variant="2cyc"))."""
    seen = 0
    for c in golden:
        r = c.get("rtl2_model")
        if r is None:
            continue
        seen += 1
        la, lb, lc = len(c["a"]), len(c["b"]), len(c["c"])
        assert r["agrees"] == ((not r["x"]) and r["score"] == c["score"]), c["name"]
        assert r["agrees"] == tsa.rtl_envelope(la, lb, lc, variant="2cyc"), c["name"]
        if la * lb * lc <= 64 ** 3:
            s, isx, cyc = orc.rtl2_run(c["a"], c["b"], c["c"])
            assert (s, isx, cyc) == (r["score"], r["x"], r["cycles"]), c["name"]
    assert seen >= 30


RTL2_SHAPES = [(n, n, n) for n in range(8, 137, 8)] + [
    (64, 32, 64), (64, 64, 32), (64, 64, 8), (32, 64, 8), (128, 64, 64), (64, 64, 128),
    (48, 48, 96), (96, 96, 16), (40, 40, 80)]


def test_rtl2_envelope_is_where_the_model_agrees(orc, tsa):
    """The 2-cycle variant's y-face store (3 groups x 2 x 8 SRAMs, group and
    page from index bits shared with B_idx, src/TriAlign_2cyc.v:85-92,141-157,
    176-180) only carries every face to its reader for some shapes: LB = LA
    (or a single z pencil), and no bank shared by a pencil's write, read and
    corner slots -- 8, 16, 40, 48, 64, 128 cubes here; 24, 32, 56, 72-120,
    136 cubes and LB != LA come back X or wrong. The host-side rule
    (_rtl2_ring_ok) is checked against the clocked model on every shape."""
    for la, lb, lc in RTL2_SHAPES:
        agree = []
        for seed in range(3):
            rng = np.random.default_rng(seed)
            a, b, c = (rng.integers(0, 4, n).astype(np.uint8) for n in (la, lb, lc))
            s, isx, _ = orc.rtl2_run(a, b, c)
            agree.append((not isx) and s == orc.score(a, b, c))
        want = tsa.rtl_envelope(la, lb, lc, variant="2cyc")
        assert (all(agree) if want else not all(agree)), ((la, lb, lc), agree, want)
    assert tsa.rtl_envelope(64, 64, 64, variant="2cyc") and tsa.rtl_envelope(256, 256, 256, variant="2cyc")
    assert not tsa.rtl_envelope(96, 96, 96, variant="2cyc") and tsa.rtl_envelope(96, 96, 96)


def test_factored_form_equals_literal(orc):
    rng = np.random.default_rng(11)
    for k in range(40):
        la, lb, lc = (int(v) for v in rng.integers(1, 30, 3))
        a, b, c = (rng.integers(0, 5, n).astype(np.uint8) for n in (la, lb, lc))
        p = orc.default_params(s3_mode=k % 2, score_bits=0)
        assert orc.score(a, b, c, p, method="msg") == orc.score(a, b, c, p)


def test_ab_symmetry_rtl_s3(orc):
    # penalty table is x<->y symmetric and RTL s3 is a<->b symmetric
    rng = np.random.default_rng(3)
    for _ in range(20):
        la, lb, lc = (int(v) for v in rng.integers(1, 20, 3))
        a, b, c = (rng.integers(0, 4, n).astype(np.uint8) for n in (la, lb, lc))
        assert orc.score(a, b, c) == orc.score(b, a, c)


def test_sop_full_permutation_invariance(orc):
    import itertools
    rng = np.random.default_rng(5)
    p = orc.default_params(s3_mode=1)
    for _ in range(8):
        seqs = [rng.integers(0, 4, int(n)).astype(np.uint8) for n in rng.integers(1, 16, 3)]
        ref = orc.score(*seqs, p)
        for perm in itertools.permutations(range(3)):
            assert orc.score(*(seqs[i] for i in perm), p) == ref


def test_rtl_s3_quirk_differs_from_sop(orc):
    # a==b!=c scores 0 in the RTL (src/PE_1cyc.v:162) but -1 as sum of pairs
    a, b, c = [0], [0], [1]
    _, fin = orc.score(a, b, c, orc.default_params(score_bits=0), final_states=True)
    assert fin[0] == 0  # M = 0 + s3
    _, fin = orc.score(a, b, c, orc.default_params(s3_mode=1, score_bits=0), final_states=True)
    assert fin[0] == -1


def test_wrap_changes_result_only_when_range_exceeded(orc):
    z = [0] * 48
    assert orc.score(z, z, z, orc.default_params(score_bits=0)) == 144
    assert orc.score(z, z, z, orc.default_params(score_bits=12)) == 144
    assert orc.score(z, z, z, orc.default_params(score_bits=8)) != 144  # 144 > 127 wraps


def test_state_range_small_for_random(orc):
    rng = np.random.default_rng(9)
    a, b, c = (rng.integers(0, 4, 64).astype(np.uint8) for _ in range(3))
    lo, hi = orc.state_range(a, b, c)
    assert -40 < lo <= 0 <= hi < 40


# (match, mismatch, gap_open, gap_extend): the sets whose admission edges
# tests/test_range_proof.py and tests/test_range_edges_gpu.py visit
RANGE_SETS = [(1, -1, 2, 1), (2, 0, 2, 1), (3, 1, 2, 1), (40, -1, 2, 1), (10, 8, 2, 1), (0, -2, 3, 2),
              (-1, -3, 4, 3)]


def _py_candidate_range(orc, a, b, c, p):
    """The recurrence of DESIGN.md 1.1 written out directly from penalty_table,
    s2 and s3 in Python integers: every candidate S[s] - P[T][s] + score_T of
    every real cell, every state, and where the extremes are first attained."""
    P = orc.penalty_table(p).tolist()
    # offset (dx, dy, dz) of the predecessor each target reads: M, Ix, Iy, Iz, Ixy, Iyz, Ixz
    step = [(1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1)]
    S = {}
    lo = hi = slo = shi = 0
    at_lo = at_hi = (0, 0, 0, -1, -1)
    for x in range(1, len(a) + 1):
        for y in range(1, len(b) + 1):
            for z in range(1, len(c) + 1):
                u, v, w = int(a[x - 1]), int(b[y - 1]), int(c[z - 1])
                add = [orc.s3(u, v, w, p), 0, 0, 0, orc.s2(u, v, p), orc.s2(v, w, p), orc.s2(u, w, p)]
                out = []
                for T, (dx, dy, dz) in enumerate(step):
                    pred = S.get((x - dx, y - dy, z - dz), [0] * 7)  # a face cell: all states 0
                    cands = [pred[s] - P[T][s] + add[T] for s in range(7)]
                    for s, val in enumerate(cands):
                        if val < lo:
                            lo, at_lo = val, (x, y, z, T, s)
                        if val > hi:
                            hi, at_hi = val, (x, y, z, T, s)
                    out.append(max(cands))
                S[(x, y, z)] = out
                slo, shi = min(slo, *out), max(shi, *out)
    return (lo, hi, slo, shi, at_lo, at_hi), S[(len(a), len(b), len(c))]


@pytest.mark.parametrize("s3_mode", (0, 1))
@pytest.mark.parametrize("pset", RANGE_SETS, ids=lambda s: "m%d_mm%d_go%d_ge%d" % s)
def test_candidate_range_against_python_restatement(orc, pset, s3_mode):
    """tsao_candidate_range against the direct restatement, on cubes up to
    5 x 4 x 3: the range of the 49 pre-MAX sums of every real cell, the cells,
    targets and sources attaining it, the state part (equal to state_range),
    and, from the same Python sweep, the unwrapped score and final states."""
    m, mm, go, ge = pset
    p = orc.default_params(match=m, mismatch=mm, gap_open=go, gap_extend=ge, s3_mode=s3_mode, score_bits=0)
    rng = np.random.default_rng([s3_mode, RANGE_SETS.index(pset)])
    shapes = [(1, 1, 1), (5, 4, 3), (3, 4, 5), (4, 1, 5), (2, 3, 1)]
    fams = [lambda n, k: np.zeros(n, np.uint8), lambda n, k: np.full(n, k, np.uint8),
            lambda n, k: np.full(n, (0, 0, 1)[k], np.uint8), lambda n, k: rng.integers(0, 4, n).astype(np.uint8),
            lambda n, k: rng.integers(0, 2, n).astype(np.uint8)]
    for dims in shapes:
        for fam in fams:
            a, b, c = (fam(n, k) for k, n in enumerate(dims))
            want, fin = _py_candidate_range(orc, a, b, c, p)
            got = orc.candidate_range(a, b, c, p)
            assert tuple(got) == want, (dims, a, b, c, got, want)
            assert (got.state_lo, got.state_hi) == orc.state_range(a, b, c, p)
            assert got.lo <= got.state_lo <= 0 <= got.state_hi <= got.hi
            assert orc.score(a, b, c, p, final_states=True) == (max(fin), tuple(fin))
    # score_bits is ignored: a word the values leave does not change the range
    p8 = orc.default_params(match=m, mismatch=mm, gap_open=go, gap_extend=ge, s3_mode=s3_mode, score_bits=4)
    assert orc.candidate_range(a, b, c, p8) == got


def test_candidate_range_all_is_the_union(orc):
    """candidate_range_all on (2, 1, 2): the union of candidate_range over the
    1024 triples, enumerated here in Python, and the first triples attaining it."""
    import itertools
    la, lb, lc = 2, 1, 2
    for pset, s3_mode in ((RANGE_SETS[0], 0), (RANGE_SETS[4], 0), (RANGE_SETS[6], 1)):
        m, mm, go, ge = pset
        p = orc.default_params(match=m, mismatch=mm, gap_open=go, gap_extend=ge, s3_mode=s3_mode)
        each = []
        for i, s in enumerate(itertools.product(range(4), repeat=5)):
            s = s[::-1]  # position 0 is the lowest digit of the triple's number
            r = orc.candidate_range(s[:la], s[la:la + lb], s[la + lb:], p)
            each.append((r.lo, r.hi))
            assert [list(t) for t in orc.triple_number(i, la, lb, lc)] == [list(s[:2]), list(s[2:3]), list(s[3:])]
        los, his = [e[0] for e in each], [e[1] for e in each]
        want = (min(los), max(his), los.index(min(los)), his.index(max(his)))
        assert orc.candidate_range_all(la, lb, lc, p) == want


def test_generator_matches_python(orc, synth):
    for seed in (synth.SEED_BASE, synth.SEED_BASE + 5, 12345):
        for n in (1, 31, 32, 33, 257):
            assert np.array_equal(orc.gen_uniform(seed, n), synth.gen_uniform(seed, n))


def test_batch_threads(orc, synth):
    seqs, offs = synth.batch(0, 6, 20, 17, 23)
    s1 = orc.score_batch(seqs, offs, nthreads=1)
    s3 = orc.score_batch(seqs, offs, nthreads=3)
    assert np.array_equal(s1, s3)
    for i in range(6):
        o = offs[3 * i:3 * i + 4]
        assert s1[i] == orc.score(seqs[o[0]:o[1]], seqs[o[1]:o[2]], seqs[o[2]:o[3]])
