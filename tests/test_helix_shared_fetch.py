"""The helix's shared ring fetch on the GPU (csrc/pencil_kernel.hip, the RP
forms): waves 1 and 2 issue the LDS-DMA fetches of wave 0's ring rows
at static steps of the four-step group, wave 0 only reads its slots, and the
step barrier is the only order between them. A fetch that lands late, or over
a row wave 0 has not read, gives a wrong score; a row fetched before the last
wave wrote it brings in what the workspace held. So every launch runs on a
workspace whose halves all hold 0x7C00 (f16 +inf; outside the integer cell's
window too), which lifts a score above the oracle's wherever it gets in.
Three ragged triples per case, bit-exact against the C oracle, in both s3
modes, under the integer and the float cell.

Shapes (max LA, max LB, max LC):
  * (256, 9, 256): the second lap is one row, so the first fetched rows follow
    wave 0's switch step t_sw directly;
  * (256, 16, 256), (256, 17, 129): the lap boundary exact, and one row past it;
  * (257, 24, 256): P = 260, t_sw = 4 (mod 8): the issuers' first groups and
    wave 0's two groups of slots meet in the other phase;
  * (253, 40, 200): five laps, padding columns.
"""
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(256, 9, 256), (256, 16, 256), (256, 17, 129), (257, 24, 256), (253, 40, 200)]
ARITH = ["f16vi", "f16vf"]


def _ragged(rng, n, dims):
    """n triples, the first at the full lengths, the others shorter."""
    out = [tuple(rng.integers(0, 4, d).astype(np.uint8) for d in dims)]
    for _ in range(n - 1):
        out.append(tuple(rng.integers(0, 4, int(rng.integers(max(1, d // 2), d + 1))).astype(np.uint8)
                         for d in dims))
    return out


def _poisoned(torch, nbytes):
    ws = torch.empty((nbytes + 1) // 2, dtype=torch.int16, device="cuda")
    ws.fill_(0x7C00)
    return ws


def _plan(gpu, arith, n, ml, p):
    """Select the helix and the cell; the plan must name both."""
    mod = sys.modules["tsa_amd"]
    mod.clear_overrides()
    mod.set_override("TSA_PENCIL_MODE", "helix")
    mod.set_override("TSA_PENCIL_ARITH", arith)
    plan = gpu.describe_plan(n, *ml, p, "pencil", sync=False)
    assert plan.startswith("pencil helix f16v ") and " M=2 " in plan and " NW=8" in plan, plan
    assert (" int " in plan) == (arith == "f16vi"), plan
    return plan


def _launch(gpu, torch, triples, p, d_ws, ws_bytes):
    ml = [max(len(t[k]) for t in triples) for k in range(3)]
    seqs, offs = gpu.pack_batch(triples)
    assert gpu.workspace_size(len(triples), *ml, p, "pencil") <= ws_bytes
    d_seqs, d_offs = torch.from_numpy(seqs).cuda(), torch.from_numpy(offs).cuda()
    d_sc = torch.zeros(len(triples), dtype=torch.int32, device="cuda")
    gpu.score_batch_async(d_seqs.data_ptr(), d_offs.data_ptr(), len(triples), *ml, d_sc.data_ptr(),
                          d_ws.data_ptr(), ws_bytes, torch.cuda.current_stream().cuda_stream, p, "pencil")
    torch.cuda.synchronize()
    return d_sc.cpu().numpy(), seqs, offs


@pytest.fixture(scope="module")
def cases(orc):
    """Each shape's ragged batch and its oracle scores per s3 mode, computed once."""
    out = {}
    for dims in SHAPES:
        rng = np.random.default_rng(1000 * dims[0] + 10 * dims[1] + dims[2])
        triples = _ragged(rng, 3, dims)
        out[dims] = triples, {}
    return out


def _ref(gpu, orc, cases, dims, s3_mode):
    triples, refs = cases[dims]
    if s3_mode not in refs:
        seqs, offs = gpu.pack_batch(triples)
        refs[s3_mode] = orc.score_batch(seqs, offs, orc.default_params(s3_mode=s3_mode), nthreads=8)
    return triples, refs[s3_mode]


@pytest.mark.parametrize("arith", ARITH)
@pytest.mark.parametrize("s3_mode", [0, 1])
@pytest.mark.parametrize("dims", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_poisoned_workspace(gpu, orc, cases, dims, s3_mode, arith):
    import torch
    triples, ref = _ref(gpu, orc, cases, dims, s3_mode)
    p = gpu.TsaParams.default(s3_mode=s3_mode)
    plan = _plan(gpu, arith, len(triples), dims, p)
    ws_bytes = gpu.workspace_size(len(triples), *dims, p, "pencil")
    got, _, _ = _launch(gpu, torch, triples, p, _poisoned(torch, ws_bytes), ws_bytes)
    print(plan, "scores", got.tolist(), "oracle", ref.tolist())
    assert np.array_equal(got, ref), (plan, got, ref)


@pytest.mark.parametrize("arith", ARITH)
def test_second_triple_in_a_used_workspace(gpu, orc, arith):
    """A workgroup scores another triple where it scored one before: two ragged
    batches back to back in one workspace, the second shorter in every dimension
    (another lap period and ring stride), then the first again. The slots and
    the ring hold the earlier triple's rows when the issuers' first groups run."""
    import torch
    p, op = gpu.TsaParams.default(), orc.default_params()
    rng = np.random.default_rng(77)
    first, second = _ragged(rng, 3, (300, 26, 256)), _ragged(rng, 3, (257, 17, 140))
    ws_bytes = gpu.workspace_size(3, 300, 26, 256, p, "pencil")
    d_ws = _poisoned(torch, ws_bytes)
    for triples in (first, second, first):
        ml = [max(len(t[k]) for t in triples) for k in range(3)]
        plan = _plan(gpu, arith, len(triples), ml, p)
        got, seqs, offs = _launch(gpu, torch, triples, p, d_ws, ws_bytes)
        ref = orc.score_batch(seqs, offs, op, nthreads=8)
        print(plan, "scores", got.tolist(), "oracle", ref.tolist())
        assert np.array_equal(got, ref), (plan, got, ref)


@pytest.mark.parametrize("arith", ARITH)
def test_end_search_instantiation(gpu, orc, arith):
    """tsa_score_batch_ends at (256, 17, 256): the END instantiation of the same
    loop. Score and end cell against the oracle's best cell."""
    dims = (256, 17, 256)
    rng = np.random.default_rng(4242)
    triples = _ragged(rng, 3, dims)
    with gpu.overrides(pencil_arith=arith):
        text = gpu.describe_score_ends_plan(len(triples), *dims, end="any")
        assert text.startswith("pencil helix f16v rtl M=2 NW=8") and ((" int " in text) == (arith == "f16vi")), text
        got = gpu.score_batch_ends(triples, end="any")
    for t, g in zip(triples, got):
        r = orc.best_range(*t)
        want = (int(r.bmax), tuple(int(v) for v in r.at_max))
        print(text, "got", g, "oracle", want)
        assert g == want, (text, g, want)
