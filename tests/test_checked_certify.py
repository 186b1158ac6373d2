"""The checked kernel's certification at its limits.

CPU: the rule itself -- best inside the limits implies the wrapped literal
recurrence equals the unwrapped one -- on thousands of small random triples
that reach the limits; the committed planted-peak recipes re-verified through
the oracle's best-range probe; the plan text of every geometry and case.

GPU (-m gpu): per-cell planted peaks at hi and hi + 1 through every lap
geometry (the per-lane mask), both limits (the thresholds of lap_certify and
check_limits), and peaks planted into single triples of batches whose
workgroups loop over rounds or whose launches are chunked (the per-wave slots).
"""
import functools

import numpy as np
import pytest

import _checked_cases as cc

# (match, mismatch, gap_open, gap_extend); every set runs in both s3 modes
PARAM_SETS = [(1, -1, 2, 1), (2, -3, 5, 2), (3, 0, 0, 0), (1, -2, 3, 3), (5, -4, 10, 1), (2, 1, 4, 1),
              (1, -1, 1, 1)]


# ---- 1. the oracle's probe ---------------------------------------------------
def test_best_range_corner_and_all_match(orc):
    """best_range against score(..., score_bits=0): a cube whose maximum sits at
    the corner cell (all-A n^3: Bmax = 3n, first at (n, n, n)), and the corner
    cell's best bracketed by the range on random ragged cubes; the threshold
    counts against the range itself."""
    for n in (1, 5, 17):
        a = np.zeros(n, np.uint8)
        br = orc.best_range(a, a, a, orc.default_params(), hi_thr=3 * n - 1, lo_thr=0)
        assert (br.bmax, br.at_max, br.n_above) == (3 * n, (n, n, n), 1)
        assert br.bmax == orc.score(a, a, a, orc.default_params(score_bits=0))
        assert (br.bmin, br.at_min, br.n_below) == (3, (1, 1, 1), 0)   # every cell reaches 3 from a face
    rng = np.random.default_rng(12)
    for shape in ((9, 4, 13), (1, 7, 3), (12, 12, 5)):
        a, b, c = (rng.integers(0, 4, n).astype(np.uint8) for n in shape)
        for mode in (0, 1):
            op = orc.default_params(s3_mode=mode, score_bits=6)     # score_bits is ignored by the probe
            corner = orc.score(a, b, c, orc.default_params(s3_mode=mode, score_bits=0))
            br = orc.best_range(a, b, c, op, hi_thr=corner, lo_thr=corner)
            assert br.bmin <= corner <= br.bmax
            cells = shape[0] * shape[1] * shape[2]
            assert br.n_above + br.n_below <= cells - 1           # the corner cell is in neither count
            assert (br.n_above == 0) == (br.bmax == corner) and (br.n_below == 0) == (br.bmin == corner)
            # the sub-cube ending at at_max has its corner there: score = Bmax
            x, y, z = br.at_max
            assert orc.score(a[:x], b[:y], c[:z], orc.default_params(s3_mode=mode, score_bits=0)) == br.bmax
            x, y, z = br.at_min
            assert orc.score(a[:x], b[:y], c[:z], orc.default_params(s3_mode=mode, score_bits=0)) == br.bmin


# ---- 2. the rule is sound ----------------------------------------------------
def test_certification_rule_is_sound(orc):
    """DESIGN.md 1.3's claim, checked on the reference alone: whenever every
    real cell's best lies inside the limits (derived in _checked_cases.limits
    from the oracle's penalty table and score minima, not from the library),
    the literal recurrence wrapped at SCORE_BITS has the same score and the
    same final 7-tuple as the unwrapped one. 6000 triples of lengths 1..13,
    SCORE_BITS 4..8, 70 % copies of a shared base over 1..4 letters so the
    ranges reach the limits: at least 40 % must be inside and at least 50
    exactly on a limit, so the sweep cannot pass by leaving cases out (this
    seed: 3785 inside, 87 on a limit)."""
    rng = np.random.default_rng(20261020)
    n_in = n_edge = 0
    N = 6000
    for i in range(N):
        m, mm, go, ge = PARAM_SETS[i % len(PARAM_SETS)]
        kw = dict(match=m, mismatch=mm, gap_open=go, gap_extend=ge, s3_mode=(i // len(PARAM_SETS)) % 2)
        bits = int(rng.integers(4, 9))
        letters = int(rng.integers(1, 5))
        base = rng.integers(0, letters, 13)
        seqs = []
        for _ in range(3):
            n = int(rng.integers(1, 14))
            own = rng.integers(0, letters, n)
            seqs.append(np.where(rng.random(n) < 0.7, base[:n], own).astype(np.uint8))
        op = orc.default_params(score_bits=bits, **kw)
        lo, hi = cc.limits(orc, op)
        br = orc.best_range(*seqs, op)
        if not cc.inside(br, (lo, hi)):
            continue
        n_in += 1
        n_edge += br.bmax == hi or br.bmin == lo
        wrapped = orc.score(*seqs, op, final_states=True)
        plain = orc.score(*seqs, orc.default_params(score_bits=0, **kw), final_states=True)
        assert wrapped == plain, (kw, bits, [s.tolist() for s in seqs], br, (lo, hi))
    assert n_in >= 0.4 * N and n_edge >= 50, (n_in, n_edge)


def test_limits_for_the_rtl_constants(orc):
    """The derivation's value for the RTL constants, by hand: the largest
    penalty is 2 GO = 4 into Ix/Iy/Iz (score 0), M drops 3 (s3 = -3), the pair
    states GO + 1 = 3; so drop = cdrop = 4 and 8-bit words certify [-120, 127]."""
    op = cc.params(orc)
    assert cc.drops(orc, op) == (4, 4)
    assert cc.limits(orc, op) == (-120, 127)
    assert cc.limits(orc, cc.params(orc, **cc.OTHER_PARAMS["p2352"])) == (-256 + 20, 255)


# ---- 3. the committed cases --------------------------------------------------
def _kv(plan):
    return dict(f.split("=", 1) for f in plan.split() if "=" in f)


def _assert_checked_lap(plan, m, nw):
    head = plan.split(" est=")[0]
    assert head.startswith("pencil lap i16 ") and head.endswith(" checked"), plan
    kv = _kv(plan)
    assert (int(kv["M"]), int(kv["NW"])) == (m, nw), plan
    return kv


@pytest.mark.parametrize("kind", ["over", "at"])
def test_recipes_hold(orc, kind):
    """Every committed planted-peak recipe, through best_range: the peak is
    hi + 1 (over) / hi (at), at the target cell and nowhere else."""
    op = cc.params(orc)
    assert set(cc.RECIPES) == set(cc.TARGETS)
    for cell, pair in cc.RECIPES.items():
        assert not cc.recipe_facts(orc, op, cc.SHAPE, cell, pair[kind == "at"], kind), (cell, kind)
    for name, pair in cc.OTHER.items():
        opo = cc.params(orc, **cc.OTHER_PARAMS[name])
        assert not cc.recipe_facts(orc, opo, cc.SHAPE, cc.OTHER_TARGET, pair[kind == "at"], kind), (name, kind)
    if kind == "over":
        for (k, row), (cell, rec) in cc.BATCH_RECIPES.items():
            shape = (cc.BATCH_LA, cc.BATCH_LB, cc.batch_lc(k))
            assert cell[1] == row and not cc.recipe_facts(orc, op, shape, cell, rec, kind), (k, row)


def test_low_recipes_hold(orc):
    """The low-limit inputs, through best_range: Bmin is exactly the low limit
    (also with the lap pipeline's drain cells past x = la) / one below it,
    Bmax within hi; lc alone is the smallest length, so the padding position
    lc + 1 would lie below the minimum; and the search still finds them."""
    op = cc.params(orc)
    for kind in ("at", "below"):
        (la, lb, lc), _ = cc.LOW[kind]
        assert not cc.low_facts(orc, op, cc.LOW[kind], kind), kind
        assert la + lb + lc > 127     # beyond the a-priori bound: the plan is the checked kernel's
        assert lc < lb < la
        assert cc.find_low(orc, op, kind, sizes=range(lc - 1, lc + 2)) == cc.LOW[kind]


def test_find_recipe_finds_a_committed_one(orc):
    """The search function beside the data still produces what is committed."""
    cell = cc.TARGETS[5]
    op = cc.params(orc)
    assert cc.find_recipe(orc, op, cc.SHAPE, cell, "over") == cc.RECIPES[cell][0]


def _classes(m, nw, cell, shape=cc.SHAPE):
    """What a target exercises under geometry (M, NW), from the plan's own
    numbers: RW = 2 NW rows per lap, ZT = 64 M positions per tile."""
    x, y, z = cell
    rw, zt = 2 * nw, 64 * m
    r, k = (y - 1) % rw, (z - 1) % zt
    out = {"row_low" if r % 2 == 0 else "row_high", f"sub{k % m}"}
    if r == rw - 1 and y < shape[1]:
        out.add("lap_last_row")
    if r == 0 and y > 1:
        out.add("lap_first_row")
    out |= {f"row{y}"} & {"row49", "row50"}
    if k == zt - 1 and z < shape[2]:
        out |= {"tile_last", "lane63_last_sub"}
    if k == 0 and z > 1:
        out |= {"tile_first", "lane0_first_sub"}
    out |= {f"z{z}"} & {"z269", "z270"}
    out.add("x_la" if x == shape[0] else "x_interior")
    if cell == shape:
        out.add("corner")
    return out


@pytest.mark.parametrize("m,nw", cc.GEOMETRIES)
def test_plans_and_target_classes(tsa, m, nw):
    """Host-only: every geometry plans SHAPE (and every other case of the GPU
    tests) as an int16 checked lap with ragged last lap and tile, so a planner
    change cannot silently turn these tests into helix runs; and the shared
    targets cover every class of row, position and x under this geometry."""
    la, lb, lc = cc.SHAPE
    with tsa.overrides(lap_m=m, lap_nw=nw):
        p = tsa.TsaParams.default(score_bits=cc.BITS)
        for sync, kernel in ((False, "checked"), (True, "auto")):
            kv = _assert_checked_lap(tsa.describe_plan(1, la, lb, lc, p, kernel, sync=sync), m, nw)
            assert (int(kv["laps"]), int(kv["tiles"])) == (-(-lb // (2 * nw)), -(-lc // (64 * m)))
            assert lb % (2 * nw) == 2 and lc % (64 * m) == 14     # ragged last lap, ragged last tile
        for name, kw in cc.OTHER_PARAMS.items():
            _assert_checked_lap(tsa.describe_plan(1, la, lb, lc, tsa.TsaParams.default(**kw), "checked",
                                                  sync=False), m, nw)
        for kind in ("at", "below"):
            shape = cc.LOW[kind][0]
            _assert_checked_lap(tsa.describe_plan(1, *shape, p, "checked", sync=False), m, nw)
            _assert_checked_lap(tsa.describe_plan(1, *shape, p, "auto", sync=True), m, nw)
    need = {"row_low", "row_high", "lap_last_row", "lap_first_row", "row49", "row50", "tile_last", "tile_first",
            "lane63_last_sub", "lane0_first_sub", "z269", "z270", "x_la", "x_interior", "corner"}
    need |= {f"sub{i}" for i in range(m)}
    have = set().union(*(_classes(m, nw, t) for t in cc.TARGETS))
    assert need <= have, need - have
    # every class but x_la / corner also at a target where `at` is asserted
    have_at = set().union(*(_classes(m, nw, t) for t in cc.TARGETS if t[0] <= la - cc.X_DRAIN))
    assert need - {"x_la", "corner"} <= have_at, need - have_at


def test_batch_plans(tsa):
    """The attribution batches: (64, 256, 65..128) x 24 with lap_m=1 loops its
    workgroups over 3 rounds at both NW; (72, 50, 270) x 24 with lap_m=1,
    lap_nw=4 runs as two launches of 12."""
    p = tsa.TsaParams.default(score_bits=cc.BITS)
    assert max(cc.batch_lc(k) for k in range(cc.BATCH_N)) == 128 and cc.batch_lc(0) == 65
    for nw in (4, 8):
        with tsa.overrides(lap_m=1, lap_nw=nw):
            for sync, kernel in ((False, "checked"), (True, "auto")):
                kv = _assert_checked_lap(tsa.describe_plan(cc.BATCH_N, cc.BATCH_LA, cc.BATCH_LB, 128, p, kernel,
                                                           sync=sync), 1, nw)
                assert int(kv["waves"]) == 3 and int(kv["laps"]) == cc.BATCH_LB // (2 * nw), kv
                # first-round rows lie in the first third of the laps, last-round rows in the last lap
                assert (cc.BATCH_ROWS[0] - 1) // (2 * nw) < int(kv["laps"]) // 3
                assert (cc.BATCH_ROWS[1] - 1) // (2 * nw) == int(kv["laps"]) - 1
    with tsa.overrides(lap_m=1, lap_nw=4):
        for sync, kernel in ((False, "checked"), (True, "auto")):
            kv = _assert_checked_lap(tsa.describe_plan(cc.BATCH_N, *cc.SHAPE, p, kernel, sync=sync), 1, 4)
            assert int(kv["chunk"]) == 12, kv


# ---- 4. GPU ------------------------------------------------------------------
def _async(gpu, triples, p, dims=None):
    """tsa_score_batch_async(kernel="checked") under the current overrides."""
    import torch
    seqs, offs = gpu.pack_batch(triples)
    n = len(triples)
    dims = dims or tuple(max(len(t[k]) for t in triples) for k in range(3))
    plan = gpu.describe_plan(n, *dims, p, "checked", sync=False)
    assert plan.split(" est=")[0].endswith(" checked") and " lap " in plan, plan
    d_seqs, d_offs = torch.from_numpy(seqs).cuda(), torch.from_numpy(offs).cuda()
    d_score = torch.zeros(n, dtype=torch.int32, device="cuda")
    ws = gpu.workspace_size(n, *dims, p, "checked")
    d_ws = torch.empty(max(ws, 16), dtype=torch.uint8, device="cuda")
    gpu.score_batch_async(d_seqs.data_ptr(), d_offs.data_ptr(), n, *dims, d_score.data_ptr(), d_ws.data_ptr(), ws,
                          torch.cuda.current_stream().cuda_stream, p, "checked")
    torch.cuda.synchronize()
    return d_score.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _planted(cell, kind, name=None):
    """(triple, wrapped literal oracle score) of a committed recipe; computed once."""
    import oracle as orc
    if name is None:
        op, rec = cc.params(orc), cc.RECIPES[cell][kind == "at"]
    else:
        op, rec = cc.params(orc, **cc.OTHER_PARAMS[name]), cc.OTHER[name][kind == "at"]
    tr = cc.plant(rec[0], cc.SHAPE, cell, *rec[1:])
    return tr, orc.score(*tr, op)


@pytest.mark.gpu
@pytest.mark.parametrize("m,nw", cc.GEOMETRIES)
def test_checked_peak_at_every_cell_class(gpu, orc, m, nw):
    """Async path, every geometry, every target: a peak of hi + 1 at the target
    cell alone reads TSA_SCORE_UNCERTIFIED (the mask keeps that cell, the slot
    reaches the triple's reduction, the threshold is hi); a peak of exactly hi
    there is certified and equals the wrapped literal oracle (for targets with
    x <= la - 4: the pipeline's drain cells past x = la reach the monitor by
    design and may widen the range)."""
    p = gpu.TsaParams.default(score_bits=cc.BITS)
    with gpu.overrides(lap_m=m, lap_nw=nw):
        for cell in cc.TARGETS:
            tr, _ = _planted(cell, "over")
            assert _async(gpu, [tr], p)[0] == gpu.SCORE_UNCERTIFIED, ("over", cell, sorted(_classes(m, nw, cell)))
            if cell[0] <= cc.SHAPE[0] - cc.X_DRAIN:
                tr, ref = _planted(cell, "at")
                assert _async(gpu, [tr], p)[0] == ref, ("at", cell, sorted(_classes(m, nw, cell)))


@pytest.mark.gpu
def test_checked_peak_sync_path_counts_fallbacks(gpu, orc):
    """Synchronous path (tsa_score_gpu, AUTO), one geometry, every target: both
    triples score as the literal oracle; the check-fallback count rises by
    exactly 1 for hi + 1 and by 0 for hi (x <= la - 4)."""
    p = gpu.TsaParams.default(score_bits=cc.BITS)
    with gpu.overrides(lap_m=2, lap_nw=4):
        for cell in cc.TARGETS:
            for kind in ("over", "at"):
                tr, ref = _planted(cell, kind)
                before = gpu.check_fallback_count()
                assert gpu.score(*tr, p) == ref, (kind, cell)
                rose = gpu.check_fallback_count() - before
                if kind == "over":
                    assert rose == 1, (kind, cell, rose)
                elif cell[0] <= cc.SHAPE[0] - cc.X_DRAIN:
                    assert rose == 0, (kind, cell, rose)


@pytest.mark.gpu
@pytest.mark.parametrize("m,nw", [(1, 4), (2, 8)])
def test_checked_low_limit(gpu, orc, m, nw):
    """The low threshold and the min reduction: all-different homopolymers
    whose Bmin is exactly the low limit are certified (async = the wrapped
    oracle, no fallback on the synchronous path); one below is refused (async
    TSA_SCORE_UNCERTIFIED, one fallback, the oracle's score)."""
    p, op = gpu.TsaParams.default(score_bits=cc.BITS), cc.params(orc)
    with gpu.overrides(lap_m=m, lap_nw=nw):
        for kind in ("at", "below"):
            tr = cc.low_triple(cc.LOW[kind])
            ref = orc.score(*tr, op)
            got = _async(gpu, [tr], p)[0]
            assert got == (ref if kind == "at" else gpu.SCORE_UNCERTIFIED), (kind, got, ref)
            before = gpu.check_fallback_count()
            assert gpu.score(*tr, p) == ref, kind
            assert gpu.check_fallback_count() - before == (kind == "below"), kind


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(cc.OTHER_PARAMS))
def test_checked_limits_follow_the_parameters(gpu, orc, name):
    """Sum-of-pairs, and (2, -3, 5, 2) with 9-bit words (hi = 255): hi + 1 at
    one cell is refused, hi exactly is certified -- the library's limits follow
    the parameters, not the RTL constants."""
    kw = cc.OTHER_PARAMS[name]
    p = gpu.TsaParams.default(**kw)
    for m, nw in ((1, 8), (4, 4)):
        with gpu.overrides(lap_m=m, lap_nw=nw):
            tr, ref = _planted(cc.OTHER_TARGET, "over", name)
            assert _async(gpu, [tr], p)[0] == gpu.SCORE_UNCERTIFIED, (name, m, nw)
            before = gpu.check_fallback_count()
            assert gpu.score(*tr, p) == ref and gpu.check_fallback_count() == before + 1
            tr, ref = _planted(cc.OTHER_TARGET, "at", name)
            assert _async(gpu, [tr], p)[0] == ref, (name, m, nw)
            before = gpu.check_fallback_count()
            assert gpu.score(*tr, p) == ref and gpu.check_fallback_count() == before


@functools.lru_cache(maxsize=None)
def _batch(which):
    """Backgrounds inside the limits and their oracle scores, computed once:
    "rounds" = (64, 256, 65..128) x 24, "chunks" = SHAPE x 24."""
    import oracle as orc
    op = cc.params(orc)
    if which == "rounds":
        shapes = [(cc.BATCH_LA, cc.BATCH_LB, cc.batch_lc(k)) for k in range(cc.BATCH_N)]
    else:
        shapes = [cc.SHAPE] * cc.BATCH_N
    triples, _ = cc.batch_backgrounds(orc, op, shapes, 7000 if which == "rounds" else 9000)
    seqs, offs = _pack(triples)
    return triples, orc.score_batch(seqs, offs, op, nthreads=8)


def _pack(triples):
    parts = [np.asarray(s, np.uint8) for t in triples for s in t]
    return np.concatenate(parts), np.concatenate([[0], np.cumsum([len(s) for s in parts])]).astype(np.int64)


def _attribution(gpu, orc, triples, ref, k, planted, dims):
    """Triple k replaced by a planted `over` triple: async refuses exactly
    index k and scores every other as the oracle; the synchronous batch equals
    the oracle everywhere."""
    p, op = gpu.TsaParams.default(score_bits=cc.BITS), cc.params(orc)
    batch = list(triples)
    batch[k] = planted
    want = ref.copy()
    want[k] = orc.score(*planted, op)
    got = _async(gpu, batch, p, dims)
    refused = np.flatnonzero(got == gpu.SCORE_UNCERTIFIED).tolist()
    assert refused == [k], (k, refused)
    others = np.arange(len(batch)) != k
    assert np.array_equal(got[others], want[others]), (k, got, want)
    assert np.array_equal(gpu.score_batch(batch, p), want), k


@pytest.mark.gpu
@pytest.mark.parametrize("nw", [4, 8])
def test_checked_batch_attribution_across_rounds(gpu, orc, nw):
    """24 ragged triples whose workgroups loop over 3 rounds: a peak planted
    into triple 0, a middle one or 23, in a first-round lap or in a last-round
    lap, refuses that triple alone -- a slot a later round overwrites, or a
    slot base shifted by one triple, would refuse another or none."""
    triples, ref = _batch("rounds")
    with gpu.overrides(lap_m=1, lap_nw=nw):
        for (k, row), (cell, rec) in cc.BATCH_RECIPES.items():
            shape = (cc.BATCH_LA, cc.BATCH_LB, cc.batch_lc(k))
            _attribution(gpu, orc, triples, ref, k, cc.plant(rec[0], shape, cell, *rec[1:]),
                         (cc.BATCH_LA, cc.BATCH_LB, 128))


@pytest.mark.gpu
def test_checked_batch_attribution_across_chunks(gpu, orc):
    """SHAPE x 24 at lap_m=1, lap_nw=4 runs as two launches of 12 that share
    the monitor words: a peak in triple 0, 12 (the second launch's first) or
    23 refuses that triple alone."""
    triples, ref = _batch("chunks")
    with gpu.overrides(lap_m=1, lap_nw=4):
        for k, cell in ((0, cc.TARGETS[0]), (12, cc.TARGETS[4]), (23, cc.TARGETS[14])):
            _attribution(gpu, orc, triples, ref, k, _planted(cell, "over")[0], cc.SHAPE)
