"""The V-space M = 2 helix on integer bit patterns (cell_messages_vi in
csrc/pencil_common.h, use_vi in csrc/pencil_kernel.hip), bit-exact against the
C oracle, beside the float cell it replaces.

A half holds bias + 8 V inside [0x0400, 0x7BFF]; the cell's sixteen constant
adds per step are 32-bit integer adds of a packed constant, so a low half that
left the window would carry into the high half beside it (position k + 128).
The shapes are those where that could happen first:
  * (5, 9, 129): the most x padding (P = 256 against LA = 5) and z padding (one
    real cell in the high halves), and a partial second lap;
  * (256, 8, 256), (256, 9, 256): one lap exactly, and one row more;
  * (253..257, 17, 256): the lap wrap at every phase of the four-step group.
Every batch runs on a workspace filled with 0x7C00 (f16 +inf, outside the
window) and used for a second call as the first left it. Batches of one triple
hold the all-match and the all-distinct triple (the top and the bottom of the
value range); the batch of three holds a random triple at the full lengths, a
ragged random one and a ragged all-match one. Scores under the default plan,
under pencil_arith = f16vi and under f16vf must all equal the oracle's, in both
s3 modes, for every lam = gap_extend = -mismatch the V-space plan admits at the
shape (tests/test_helix_prev_reads.py lists them the same way; the last test
here checks the lists). The plan names the integer cell with the token " int";
f16vi is refused (TSA_EINVAL) exactly where that token is missing.
"""
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PADDED = [(5, 9, 129)]
LAPS = [(256, 8, 256), (256, 9, 256)]
WRAPS = [(la, 17, 256) for la in (253, 254, 255, 256, 257)]
LAM_MAX = 9
# admitted by the f16v plan and refused by use_vi: 8 lam (P + LB + 2 NW + 256) alone passes the window
REFUSED = ((5, 9, 129), 6)


def _lams(dims):
    return (1, 2, 3, 4, 5, 6) if dims in PADDED else (1, 2, 3)


def _cases(shapes):
    return [pytest.param(d, lam, id=f"{d[0]}x{d[1]}x{d[2]}-lam{lam}") for d in shapes for lam in _lams(d)]


def _candidates(gpu, orc, lam, s3_mode):
    for match in (2 - lam, 1 - lam):
        kw = dict(match=match, mismatch=-lam, gap_extend=lam, s3_mode=s3_mode)
        yield (gpu.TsaParams.default(gap_open=lam + 1, **kw), orc.default_params(gap_open=lam + 1, **kw))


def _plan(gpu, n, dims, p):
    try:
        return gpu.describe_plan(n, *dims, p, "pencil", sync=False)
    except Exception:  # noqa: BLE001 -- parameters the library refuses are not admitted
        return ""


def _params(gpu, orc, dims, lam, s3_mode, n=3):
    for p, op in _candidates(gpu, orc, lam, s3_mode):
        if _plan(gpu, n, dims, p).startswith("pencil helix f16v "):
            return p, op
    return None


def _batches(rng, dims):
    la, lb, lc = dims
    same = tuple(np.full(d, 2, np.uint8) for d in dims)
    distinct = tuple(np.full(d, v, np.uint8) for d, v in zip(dims, (0, 1, 2)))
    rand = tuple(rng.integers(0, 4, d).astype(np.uint8) for d in dims)
    ragged = tuple(rng.integers(0, 4, int(rng.integers(max(1, d // 2), d + 1))).astype(np.uint8) for d in dims)
    short = tuple(np.full(int(rng.integers(max(1, d // 2), d + 1)), 1, np.uint8) for d in dims)
    return [[same], [distinct], [rand, ragged, short]]


def _score_twice(gpu, torch, triples, dims, p):
    n = len(triples)
    seqs, offs = gpu.pack_batch(triples)
    ws_bytes = gpu.workspace_size(n, *dims, p, "pencil")
    d_ws = torch.empty((ws_bytes + 1) // 2, dtype=torch.int16, device="cuda")
    d_ws.fill_(0x7C00)
    d_seqs, d_offs = torch.from_numpy(seqs).cuda(), torch.from_numpy(offs).cuda()
    out = []
    for _ in range(2):  # the second call meets the rows the first one left
        d_sc = torch.zeros(n, dtype=torch.int32, device="cuda")
        gpu.score_batch_async(d_seqs.data_ptr(), d_offs.data_ptr(), n, *dims, d_sc.data_ptr(), d_ws.data_ptr(),
                              ws_bytes, torch.cuda.current_stream().cuda_stream, p, "pencil")
        torch.cuda.synchronize()
        out.append(d_sc.cpu().numpy())
    return out


def _run(gpu, orc, dims, lam, expect_int=True):
    import torch
    mod = sys.modules["tsa_amd"]
    for s3_mode in (0, 1):
        mod.clear_overrides()
        mod.set_override("TSA_PENCIL_MODE", "helix")
        admitted = _params(gpu, orc, dims, lam, s3_mode)
        assert admitted is not None, (dims, lam, s3_mode)
        p, op = admitted
        rng = np.random.default_rng(900000 * lam + 1000 * dims[0] + 10 * dims[1] + dims[2] + s3_mode)
        for triples in _batches(rng, dims):
            n = len(triples)
            seqs, offs = gpu.pack_batch(triples)
            ref = orc.score_batch(seqs, offs, op, nthreads=8)
            for arith in (None, "f16vi", "f16vf"):
                mod.clear_overrides()
                mod.set_override("TSA_PENCIL_MODE", "helix")
                if arith:
                    mod.set_override("TSA_PENCIL_ARITH", arith)
                plan = gpu.describe_plan(n, *dims, p, "pencil", sync=False)
                assert plan.startswith("pencil helix f16v ") and " M=2 " in plan, plan
                is_int = f" P={(max(dims[0], 256) + 3) // 4 * 4} int " in plan
                assert is_int == (expect_int and arith != "f16vf"), (arith, plan)
                if arith == "f16vi" and not is_int:
                    with pytest.raises(gpu.TsaError) as e:
                        _score_twice(gpu, torch, triples, dims, p)
                    assert e.value.rc == gpu.TSA_EINVAL, e.value
                    continue
                for got in _score_twice(gpu, torch, triples, dims, p):
                    print(plan, "scores", got.tolist())
                    assert np.array_equal(got, ref), (plan, arith, got, ref)


@pytest.mark.parametrize("dims,lam", _cases(PADDED))
def test_padding_and_partial_lap(gpu, orc, dims, lam):
    _run(gpu, orc, dims, lam, expect_int=(dims, lam) != REFUSED)


@pytest.mark.parametrize("dims,lam", _cases(LAPS))
def test_one_lap_and_one_row_more(gpu, orc, dims, lam):
    _run(gpu, orc, dims, lam)


@pytest.mark.parametrize("dims,lam", _cases(WRAPS))
def test_lap_wrap_phases(gpu, orc, dims, lam):
    _run(gpu, orc, dims, lam)


def test_plans(gpu, orc):
    """The 512 x 256^3 batch with default parameters runs the integer cell; the
    lam lists above hold every lam the V-space plan admits at their shapes; and
    the set the f16v plan admits but use_vi refuses plans f16v without the token."""
    mod = sys.modules["tsa_amd"]
    plan = gpu.describe_plan(512, 256, 256, 256, gpu.TsaParams.default(), "pencil", sync=False)
    assert plan.startswith("pencil helix f16v rtl M=2 NW=8 P=256 int "), plan
    mod.set_override("TSA_PENCIL_MODE", "helix")
    for dims in PADDED + LAPS + WRAPS:
        for s3_mode in (0, 1):
            got = tuple(lam for lam in range(1, LAM_MAX + 1) if _params(gpu, orc, dims, lam, s3_mode) is not None)
            assert got == _lams(dims), (dims, s3_mode, got)
    dims, lam = REFUSED
    p, _ = _params(gpu, orc, dims, lam, 0)
    plan = gpu.describe_plan(3, *dims, p, "pencil", sync=False)
    assert plan.startswith("pencil helix f16v ") and " int" not in plan, plan
