"""Inputs that put the checked kernel's certification at its
limits, one cell at a time. Shared by the CPU and GPU tests of
tests/test_checked_certify.py.

* ``limits``: the certification limits, derived from the oracle's own penalty
  table and score functions as DESIGN.md 1.2 words drop and cdrop --
  independent of the library's ``bound_drops`` / ``check_limits``.
* ``plant``: a random background with one common run ending at a chosen cell,
  so the peak of ``best`` sits at that cell.
* ``RECIPES`` & co: ``(seed, r, gaps)`` triples found once by ``find_recipe``
  (``search_all`` regenerates every table below) such that the peak is exactly
  hi + 1 (``over``) or exactly hi (``at``) at the target cell. The CPU tests
  re-verify every recipe through ``oracle.best_range``.
"""
from __future__ import annotations

import numpy as np

SHAPE = (72, 50, 270)   # 7 / 4 laps with a ragged last lap, 5 / 3 / 2 z tiles with a ragged last tile
BITS = 8                # hi = 127 with the RTL constants
GEOMETRIES = tuple((m, nw) for m in (1, 2, 4) for nw in (4, 8))
X_DRAIN = 4             # `at` is asserted on the GPU only for targets with x <= la - X_DRAIN


# ---- limits ------------------------------------------------------------------
def drops(orc, op):
    """(drop, cdrop) of DESIGN.md 1.2: how far below its predecessor's best a
    state can sit, and how far below the state it reads a candidate can sit --
    a penalty less the smallest score its target adds."""
    P = orc.penalty_table(op)
    syms = range(4)
    s3min = min(orc.s3(u, v, w, op) for u in syms for v in syms for w in syms)
    s2min = min(orc.s2(u, v, op) for u in syms for v in syms)
    scmin = [s3min, 0, 0, 0, s2min, s2min, s2min]   # M adds s3, Ix/Iy/Iz nothing, the pair states s2
    drop = max(max(int(P[t][s]) for s in range(7)) - scmin[t] for t in range(7))
    cdrop = max(int(P[t][s]) - scmin[t] for t in range(7) for s in range(7))
    return drop, cdrop


def limits(orc, op):
    """(lo, hi): no candidate of the literal recurrence wraps at op.score_bits
    when every real cell's best lies in [lo, hi]."""
    drop, cdrop = drops(orc, op)
    half = 1 << (op.score_bits - 1)
    return -half + drop + max(0, cdrop), half - 1


def inside(rng_, lim):
    return rng_.bmin >= lim[0] and rng_.bmax <= lim[1]


def params(orc, **kw):
    """Oracle params from keywords; BITS-bit words unless said otherwise."""
    kw.setdefault("score_bits", BITS)
    return orc.default_params(**kw)


# ---- the builder -------------------------------------------------------------
def background(seed, shape):
    rng = np.random.default_rng(seed)
    return tuple(rng.integers(0, 4, n).astype(np.uint8) for n in shape)


def plant(seed, shape, cell, r, gaps=0):
    """Random background (seed) with a common run of r symbols ending at
    cell = (x, y, z) (1-based: the run's last symbols are a[x-1], b[y-1],
    c[z-1]) in all three sequences, followed by three pairwise different
    symbols -- the peak of best sits at cell and decays around it.

    gaps > 0 fixes the peak's residue by construction when the run starts on a
    face (r = the smallest coordinate, start value 0): the two sequences with
    the larger coordinates get `gaps` extra common symbols, spread through
    their copies of the run, which the best path takes as single pair steps
    (one open penalty less one match each)."""
    rng = np.random.default_rng(seed)
    seqs = [rng.integers(0, 4, n).astype(np.uint8) for n in shape]
    run = rng.integers(0, 4, r).astype(np.uint8)
    extra = rng.integers(0, 4, gaps).astype(np.uint8)
    follow = rng.permutation(4)[:3]
    at = [(k + 1) * r // (gaps + 1) for k in range(gaps)]       # single gaps, apart from each other
    long_run = np.insert(run, at, extra) if gaps else run
    short = int(np.argmin(cell))
    for k in range(3):
        body = run if k == short else long_run
        if len(body) > cell[k]:
            raise ValueError(f"run of {len(body)} does not fit before {cell}")
        seqs[k][cell[k] - len(body):cell[k]] = body
        if cell[k] < shape[k]:
            seqs[k][cell[k]] = follow[k]
    return tuple(seqs)


# ---- recipes -----------------------------------------------------------------
def recipe_facts(orc, op, shape, cell, recipe, kind):
    """What a recipe must satisfy, as a list of failed conditions (empty = ok).
    over: Bmax = hi + 1, exactly one cell above hi, the target.
    at:   Bmax = hi, first (and only) attained at the target.
    Both keep Bmin inside the low limit, so only the high side is at issue."""
    lo, hi = limits(orc, op)
    a, b, c = plant(recipe[0], shape, cell, *recipe[1:])
    want = hi + 1 if kind == "over" else hi
    br = orc.best_range(a, b, c, op, hi_thr=want - 1, lo_thr=lo)
    bad = []
    if br.bmax != want:
        bad.append(f"Bmax {br.bmax} != {want}")
    if br.at_max != tuple(cell):
        bad.append(f"peak at {br.at_max}, not {tuple(cell)}")
    if br.n_above != 1:
        bad.append(f"{br.n_above} cells reach {want}")
    if br.n_below:
        bad.append(f"Bmin {br.bmin} below {lo}")
    return bad


def find_recipe(orc, op, shape, cell, kind, seeds=range(400), max_gaps=5):
    """Search (seed, r, gaps) for a recipe of `kind` at `cell`. Combinations
    whose run starts on a face (r = the smallest coordinate) have a known peak,
    3 match r - gaps (gap_open - match); the others start from the
    background's small value at the run's first cell and are tried within a
    few penalties of the wanted peak."""
    lo, hi = limits(orc, op)
    want = hi + 1 if kind == "over" else hi
    per_match, per_gap = orc.s3(0, 0, 0, op), op.gap_open - op.match
    m = min(cell)
    rs = range(min(m, want // per_match + 2), 0, -1)
    for seed in seeds:
        for r in rs:
            for gaps in range(max_gaps + 1):
                peak = per_match * r - per_gap * gaps
                slack = 0 if r == m else 2 * per_match
                if abs(want - peak) > slack or r + gaps > sorted(cell)[1]:
                    continue
                if not recipe_facts(orc, op, shape, cell, (seed, r, gaps), kind):
                    return (seed, r, gaps)
    raise LookupError(f"no {kind} recipe at {cell}")


# Targets (x, y, z) in SHAPE, 1-based, shared by the six geometries. y: wave
# halves (45 low, 46 high at RW 8 and 16), lap seam 48 | 49, last real rows 49
# and 50. z: tile seams 64 | 65 (ZT 64), 128 | 129 (ZT 64, 128), 256 | 257
# (every ZT) = lane 63's last sub-position | lane 0's first; 269, 270 the last
# real positions of the ragged tile; 81..84 the sub-positions of one lane at
# M = 4 (two lanes' at M = 2). x: interior, la, and the corner = the final cell.
TARGETS = (
    (60, 45, 150), (61, 46, 151), (62, 48, 152), (63, 49, 153), (64, 50, 154), (59, 43, 155),
    (58, 47, 64), (59, 47, 65), (60, 47, 128), (61, 47, 129), (62, 47, 256), (63, 47, 257),
    (64, 47, 269), (65, 47, 270), (66, 50, 270),
    (66, 47, 81), (67, 47, 82), (68, 47, 83), (57, 47, 84),
    (72, 47, 140), (72, 50, 270),
)

# {target: (over recipe, at recipe)} -- search_all() output
RECIPES = {
    (60, 45, 150): ((2, 44, 2), (2, 44, 3)),
    (61, 46, 151): ((0, 44, 0), (3, 43, 0)),
    (62, 48, 152): ((1, 43, 0), (2, 44, 5)),
    (63, 49, 153): ((5, 43, 3), (0, 43, 0)),
    (64, 50, 154): ((1, 44, 0), (1, 44, 5)),
    (59, 43, 155): ((2, 43, 1), (1, 43, 2)),
    (58, 47, 64): ((0, 44, 2), (0, 43, 2)),
    (59, 47, 65): ((0, 43, 0), (0, 44, 3)),
    (60, 47, 128): ((0, 44, 3), (0, 43, 0)),
    (61, 47, 129): ((0, 44, 1), (0, 43, 2)),
    (62, 47, 256): ((3, 44, 2), (1, 44, 2)),
    (63, 47, 257): ((1, 43, 0), (2, 44, 3)),
    (64, 47, 269): ((0, 44, 0), (0, 44, 3)),
    (65, 47, 270): ((0, 44, 3), (0, 44, 1)),
    (66, 50, 270): ((0, 44, 1), (3, 42, 4)),
    (66, 47, 81): ((0, 44, 1), (0, 44, 3)),
    (67, 47, 82): ((4, 44, 0), (0, 44, 2)),
    (68, 47, 83): ((2, 43, 0), (1, 43, 0)),
    (57, 47, 84): ((3, 42, 1), (0, 44, 2)),
    (72, 47, 140): ((0, 44, 2), (0, 44, 3)),
    (72, 50, 270): ((0, 44, 1), (0, 43, 1)),
}

# other parameters (OTHER_PARAMS below), at OTHER_TARGET: {name: (over recipe, at recipe)}
OTHER = {
    'sop': ((2, 44, 4), (0, 44, 1)),
    'p2352': ((0, 44, 2), (4, 44, 3)),
}

# low limit: all-different homopolymers a = 0.., b = 1.., c = 2.. of these
# lengths with single symbols changed ((sequence, index, symbol), ...):
# `at` has Bmin = the low limit exactly, `below` one less; Bmax <= hi in both.
LOW = {
    'at': ((68, 64, 60), ()),
    'below': ((69, 65, 61), ((1, 30, 0),)),
}

# batch attribution: backgrounds of (64, 256, 65..128), `over` peaks planted
# into triple k in a first-round and in a last-round lap (lap_m=1: waves=3)
BATCH_N = 24
BATCH_LA, BATCH_LB = 64, 256
BATCH_KS = (0, 11, 23)
BATCH_ROWS = (45, 250)   # lap 5 of 32 / 2 of 16 (first round); lap 31 / 15 (last round)


def batch_lc(k):
    return 65 + (63 * k) // (BATCH_N - 1)


# {(k, row): (cell, over recipe)}
BATCH_RECIPES = {
    (0, 45): ((50, 45, 62), (0, 42, 0)),
    (0, 250): ((50, 250, 62), (0, 44, 1)),
    (11, 45): ((51, 45, 88), (1, 44, 2)),
    (11, 250): ((51, 250, 88), (0, 43, 1)),
    (23, 45): ((53, 45, 123), (0, 44, 2)),
    (23, 250): ((53, 250, 123), (2, 44, 1)),
}


OTHER_PARAMS = {
    "sop": dict(s3_mode=1, score_bits=8),
    "p2352": dict(match=2, mismatch=-3, gap_open=5, gap_extend=2, score_bits=9),
}
OTHER_TARGET = (60, 47, 150)


def low_triple(spec):
    """(a, b, c) of a LOW entry: ((la, lb, lc), ((sequence, index, symbol), ...))."""
    shape, edits = spec
    seqs = [np.full(n, v, np.uint8) for n, v in zip(shape, (0, 1, 2))]
    for s, i, v in edits:
        seqs[s][i] = v
    return tuple(seqs)


LOW_DRAIN = 300  # x cells past la the lap pipeline may run (RW + ZT - 2 at most)


def low_facts(orc, op, spec, kind):
    """Failed conditions of a LOW entry. The lap pipeline's drain cells past
    x = la (padding symbols of a, which match nothing: symbol 3 here) reach the
    monitor too, so `at` must hold with a extended by LOW_DRAIN such cells."""
    lo, hi = limits(orc, op)
    a, b, c = low_triple(spec)
    want = lo if kind == "at" else lo - 1
    bad = []
    br = orc.best_range(a, b, c, op)
    if br.bmin != want:
        bad.append(f"Bmin {br.bmin} != {want}")
    if br.bmax > hi:
        bad.append(f"Bmax {br.bmax} > {hi}")
    if kind == "at":
        ext = orc.best_range(np.concatenate([a, np.full(LOW_DRAIN, 3, np.uint8)]), b, c, op)
        if ext.bmin != want or ext.bmax > hi:
            bad.append(f"with drain cells: [{ext.bmin}, {ext.bmax}]")
    return bad


def find_low(orc, op, kind, sizes=range(40, 80)):
    """Search shapes (lc + 8, lc + 4, lc), then one symbol of b or a changed
    mid-sequence, for a LOW entry of `kind`. Every cell reaches a face within
    its smallest coordinate, so best falls with min(x, y, z) only (2 per step
    here, an odd total once a changed symbol pairs a with b): with lc alone the
    smallest length the minimum sits on z = lc from x, y = lc on, the x drain
    does not lower it, and a monitor that took in the padding position lc + 1
    would see it lower."""
    for lc in sizes:
        shape = (lc + 8, lc + 4, lc)
        for edits in [()] + [((s, lc // 2, v),) for s in (1, 0) for v in range(4) if v != s]:
            if not low_facts(orc, op, (shape, edits), kind):
                return (shape, edits)
    raise LookupError(f"no low-limit {kind} shape")


def batch_backgrounds(orc, op, shapes, seed0):
    """One random triple per shape, re-seeded until its best range is inside
    the limits; returns (triples, seeds)."""
    lim = limits(orc, op)
    out, seeds = [], []
    for k, shape in enumerate(shapes):
        for t in range(50):
            seed = seed0 + 1000 * k + t
            tr = background(seed, shape)
            if inside(orc.best_range(*tr, op), lim):
                break
        else:
            raise LookupError(f"no background inside the limits for triple {k}")
        out.append(tr)
        seeds.append(seed)
    return out, seeds


def search_all(orc):
    """Regenerate every table of this module; prints Python literals."""
    op = params(orc)
    print("RECIPES = {")
    for cell in TARGETS:
        print(f"    {cell}: ({find_recipe(orc, op, SHAPE, cell, 'over')}, "
              f"{find_recipe(orc, op, SHAPE, cell, 'at')}),", flush=True)
    print("}\nOTHER = {")
    for name, kw in OTHER_PARAMS.items():
        opo = params(orc, **kw)
        print(f"    {name!r}: ({find_recipe(orc, opo, SHAPE, OTHER_TARGET, 'over')}, "
              f"{find_recipe(orc, opo, SHAPE, OTHER_TARGET, 'at')}),", flush=True)
    print("}\nLOW = {")
    for kind in ("at", "below"):
        print(f"    {kind!r}: {find_low(orc, op, kind)},", flush=True)
    print("}\nBATCH_RECIPES = {")
    for k in BATCH_KS:
        shape = (BATCH_LA, BATCH_LB, batch_lc(k))
        for row in BATCH_ROWS:
            cell = (50 + k % 10, row, shape[2] - 3 - k % 7)
            print(f"    ({k}, {row}): ({cell}, {find_recipe(orc, op, shape, cell, 'over')}),", flush=True)
    print("}")
