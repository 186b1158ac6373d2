"""The V-space M = 2 helix with the row above's {Iyz, best} read at position
k - 1 (the RP forms of csrc/pencil_kernel.hip), bit-exact against the C oracle.
The lam > 1 and lam q > 2047 cases below were written when the kernel also had
a form that read the face values from a constant table with a saturated tail
(DESIGN.md 4.2); they exercise the kernel's f16 and integer face values as well.

Every batch is three ragged triples (the first at the full lengths) on a
workspace poisoned with f16 +inf, as tests/test_helix_ring_rows.py does: with
the shifted reads, wave 0 takes another lane's record of the prefetched ring
row, and a row nobody wrote would lift a score above the oracle's.

Shapes (small: 256 x 17 x 256 is 1.1 M cells):
  * LC = 129, 130, 255, 256 at LA = 64, LB = 17: position 128 takes its z - 1
    values across the lane 63 -> lane 0 half crossing; LC = 129 is the smallest
    case in which that half holds a real cell;
  * LA = 253..257 at LB = 17, LC = 256: the lap wrap at every phase of the
    four-step group, three laps, so wave 0 reads shifted from the ring rows;
  * LB = 1, 8 (no second lap) and 9 (the first row that comes through the ring);
  * the largest LB the V-space plan accepts at a short A, for every admitted
    lam (1..6): lam q passes 2047 at padding positions only, where the face
    values' f16 adds pass 2047 too.
Parameters: both s3 modes, and every lam = GE = -mismatch the V-space plan
admits at each shape, with gap_open = lam + 1 and the match that keeps
match - mismatch at 2 (at 1 where only that is admitted: the f16 forms bound
the score deltas): lam = 1..6 at LC = 129, 130 and at the LB = 1, 8, 9 shapes,
1..5 at LC = 255, 256, 1..3 at the lap-wrap shapes. test_lam_lists_are_complete
asks the plan for lam = 1..9 at every shape and fails if a list above leaves an
admitted lam out."""
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CROSSING = [(64, 17, lc) for lc in (129, 130, 255, 256)]
WRAPS = [(la, 17, 256) for la in (253, 254, 255, 256, 257)]
ROWS = [(64, lb, 130) for lb in (1, 8, 9)]
LAM_MAX = 9  # no lam beyond 6 is admitted at any of these shapes


def _lams(dims):
    """Every lam the V-space plan admits at dims (test_lam_lists_are_complete)."""
    if dims in WRAPS:
        return (1, 2, 3)
    if dims in CROSSING and dims[2] >= 255:
        return (1, 2, 3, 4, 5)
    return (1, 2, 3, 4, 5, 6)


def _cases(shapes):
    return [pytest.param(d, lam, id=f"{d[0]}x{d[1]}x{d[2]}-lam{lam}") for d in shapes for lam in _lams(d)]


def _candidates(gpu, orc, lam, s3_mode):
    """Parameter sets with gap_extend = -mismatch = lam: match - mismatch = 2,
    then 1 (lam = 1 first meets the RTL's constants 1, -1, 2, 1)."""
    for match in (2 - lam, 1 - lam):
        kw = dict(match=match, mismatch=-lam, gap_extend=lam, s3_mode=s3_mode)
        yield (gpu.TsaParams.default(gap_open=lam + 1, **kw), orc.default_params(gap_open=lam + 1, **kw))


def _is_vs(gpu, n, dims, p):
    try:
        return gpu.describe_plan(n, *dims, p, "pencil", sync=False).startswith("pencil helix f16v ")
    except Exception:  # noqa: BLE001 -- parameters the library refuses are not admitted
        return False


def _params(gpu, orc, dims, lam, s3_mode, n=3):
    """The first candidate the V-space plan admits at dims, or None."""
    for p, op in _candidates(gpu, orc, lam, s3_mode):
        if _is_vs(gpu, n, dims, p):
            return p, op
    return None


def _ragged(rng, n, dims):
    out = [tuple(rng.integers(0, 4, d).astype(np.uint8) for d in dims)]
    for _ in range(n - 1):
        out.append(tuple(rng.integers(0, 4, int(rng.integers(max(1, d // 2), d + 1))).astype(np.uint8)
                         for d in dims))
    return out


def _run(gpu, orc, dims, lam, s3_mode, n=3):
    import torch
    sys.modules["tsa_amd"].set_override("TSA_PENCIL_MODE", "helix")
    admitted = _params(gpu, orc, dims, lam, s3_mode, n)
    assert admitted is not None, (dims, lam, s3_mode)
    p, op = admitted
    plan = gpu.describe_plan(n, *dims, p, "pencil", sync=False)
    assert plan.startswith("pencil helix f16v ") and " M=2 " in plan, plan
    rng = np.random.default_rng(100000 * lam + 1000 * dims[0] + 10 * dims[1] + dims[2] + s3_mode)
    triples = _ragged(rng, n, dims)
    seqs, offs = gpu.pack_batch(triples)
    ws_bytes = gpu.workspace_size(n, *dims, p, "pencil")
    d_ws = torch.empty((ws_bytes + 1) // 2, dtype=torch.int16, device="cuda")
    d_ws.fill_(0x7C00)  # f16 +inf in every half
    d_seqs, d_offs = torch.from_numpy(seqs).cuda(), torch.from_numpy(offs).cuda()
    d_sc = torch.zeros(n, dtype=torch.int32, device="cuda")
    gpu.score_batch_async(d_seqs.data_ptr(), d_offs.data_ptr(), n, *dims, d_sc.data_ptr(), d_ws.data_ptr(),
                          ws_bytes, torch.cuda.current_stream().cuda_stream, p, "pencil")
    torch.cuda.synchronize()
    got = d_sc.cpu().numpy()
    print(plan, "scores", got.tolist())
    assert np.array_equal(got, orc.score_batch(seqs, offs, op, nthreads=8)), (plan, got)


@pytest.mark.parametrize("s3_mode", [0, 1])
@pytest.mark.parametrize("dims,lam", _cases(CROSSING))
def test_half_crossing(gpu, orc, dims, lam, s3_mode):
    _run(gpu, orc, dims, lam, s3_mode)


@pytest.mark.parametrize("s3_mode", [0, 1])
@pytest.mark.parametrize("dims,lam", _cases(WRAPS))
def test_lap_wrap_phases_three_laps(gpu, orc, dims, lam, s3_mode):
    _run(gpu, orc, dims, lam, s3_mode)


@pytest.mark.parametrize("s3_mode", [0, 1])
@pytest.mark.parametrize("dims,lam", _cases(ROWS))
def test_first_ring_row(gpu, orc, dims, lam, s3_mode):
    _run(gpu, orc, dims, lam, s3_mode)


def test_lam_lists_are_complete(gpu, orc):
    """The lists the cases above run over hold every lam the V-space plan
    admits at their shapes, in both s3 modes, and nothing else."""
    sys.modules["tsa_amd"].set_override("TSA_PENCIL_MODE", "helix")
    for dims in CROSSING + WRAPS + ROWS:
        for s3_mode in (0, 1):
            got = tuple(lam for lam in range(1, LAM_MAX + 1) if _params(gpu, orc, dims, lam, s3_mode) is not None)
            assert got == _lams(dims), (dims, s3_mode, got)


@pytest.mark.parametrize("lam", [1, 2, 3, 4, 5, 6])
def test_table_tail_at_padding_positions(gpu, orc, lam):
    """LA = 2, LC = 129 and the largest LB the V-space plan accepts for lam, over
    the candidate parameter sets: P = 256, so position 0 of the last rows runs
    through padding columns up to x = 256, where lam (y + x) passes 2047, the
    last integer step the f16 face values take exactly. Those cells
    feed padding cells only. (No LB is admitted for lam = 7 and up.)"""
    sys.modules["tsa_amd"].set_override("TSA_PENCIL_MODE", "helix")

    def largest_lb(lam_):
        best = 0
        for p, _ in _candidates(gpu, orc, lam_, 0):
            lo, hi = 0, 4096  # the largest lb the plan admits with p (0: none)
            while lo < hi:
                mid = (lo + hi + 1) // 2
                if _is_vs(gpu, 3, (2, mid, 129), p):
                    lo = mid
                else:
                    hi = mid - 1
            best = max(best, lo)
        return best

    if lam == 6:
        assert [largest_lb(x) for x in range(7, LAM_MAX + 1)] == [0] * (LAM_MAX - 6)
    best = largest_lb(lam)
    assert best > 0 and lam * (best + 256) > 2047, (lam, best)  # q beyond the table's exact range, at x > LA only
    _run(gpu, orc, (2, best, 129), lam, 0)
