"""Shared by tests/test_range_proof.py (CPU) and tests/test_range_edges_gpu.py:
the parameter sets whose admission edges the two files visit, the input
families that drive the values to the ends of the proven range, and the
arithmetic a plan names."""
import numpy as np

# parameter sets (others default: match 1, mismatch -1, GO 2, GE 1, RTL s3, 12 bit)
SETS = {
    "default": dict(),
    "m2_mm0": dict(match=2, mismatch=0),
    "m3_mm1_b16": dict(match=3, mismatch=1, score_bits=16),
    "m40_b16": dict(match=40, mismatch=-1, score_bits=16),
    "m40_b0": dict(match=40, mismatch=-1, score_bits=0),
    "m10_mm8": dict(match=10, mismatch=8),
    "lam2_b16": dict(match=0, mismatch=-2, gap_open=3, gap_extend=2, score_bits=16),
    "lam3_b16": dict(match=-1, mismatch=-3, gap_open=4, gap_extend=3, score_bits=16),
    "b9": dict(score_bits=9),
    "b8": dict(score_bits=8),
    "b6": dict(score_bits=6),
}

SHAPES = {"cube": lambda L: (L, L, L), "L8L": lambda L: (L, 8, L), "LL256": lambda L: (L, L, 256)}
FAMILIES = ("all-match", "all-distinct", "a=b", "b=c", "a=c", "random", "related")


def plan_token(tsa, n, dims, p, kernel="pencil", sync=False):
    """The arithmetic named by the library's plan, or "refused" (TSA_ERANGE)."""
    try:
        plan = tsa.describe_plan(n, *dims, p, kernel, sync=sync)
    except tsa.TsaError as e:
        assert e.rc == tsa.TSA_ERANGE, e
        return "refused"
    if plan.startswith("plane"):
        return "plane"
    tok = plan.split()[2]
    return tok + (" int" if " int " in plan else "") + (" checked" if " checked" in plan else "")


def family(kind, dims, seed=0):
    """The input families of the edge tests: the symbols of a, b, c."""
    rng = np.random.default_rng([seed, *dims])
    if kind == "all-match":
        vals = (2, 2, 2)
    elif kind == "all-distinct":
        vals = (0, 1, 2)
    elif kind in ("a=b", "b=c", "a=c"):
        vals = {"a=b": (0, 0, 1), "b=c": (0, 1, 1), "a=c": (0, 1, 0)}[kind]
    elif kind == "random":
        return tuple(rng.integers(0, 4, d).astype(np.uint8) for d in dims)
    elif kind == "related":  # one sequence, every 9th symbol changed, at another phase in each copy
        base = rng.integers(0, 4, max(dims)).astype(np.uint8)
        out = []
        for k, d in enumerate(dims):
            s = base[:d].copy()
            s[3 * k::9] = (s[3 * k::9] + 1 + k) & 3
            out.append(s)
        return tuple(out)
    else:
        raise KeyError(kind)
    return tuple(np.full(d, v, np.uint8) for d, v in zip(dims, vals))
