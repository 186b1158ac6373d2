"""The helix's y = 0 ring rows (csrc/pencil_kernel.hip): wave 0 builds the face
records of its first steps from its own H registers (the first-lap role) and
fetches the ring only from step t_sw on; the prologue fills just the rows of
steps [t_sw, lag). Every other row wave 0 reads must have been written by the
last wave of the same unit, whatever the workspace held at entry.

The workspace is therefore poisoned before each launch: every half holds the
f16 +inf pattern 0x7C00, so a row read before it is written lifts a score above
the oracle's and cannot hide. Bit-exact against the C oracle."""
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (max LA, max LB, max LC), triples: what the shape exercises
SHAPES = [
    ((256, 24, 256), 3),  # several laps
    ((256, 8, 256), 3),   # one lap: every row wave 0 reads is a face row
    ((200, 3, 250), 3),   # one lap, fewer rows than waves
    ((256, 9, 256), 3),   # the second lap is a single row
    ((300, 17, 200), 3),  # P = 300 > 256 positions
    ((301, 17, 129), 3),  # P = 304: LA rounded up to a multiple of 4
    ((90, 20, 100), 3),   # M = 1
    ((60, 12, 60), 3),    # TWO mode, an odd number of triples
]


def _helix(gpu):
    sys.modules["tsa_amd"].set_override("TSA_PENCIL_MODE", "helix")


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


def _launch(gpu, torch, triples, p, d_ws, ws_bytes):
    ml = [max(len(t[k]) for t in triples) for k in range(3)]
    plan = gpu.describe_plan(len(triples), *ml, p, "pencil", sync=False)
    assert plan.startswith("pencil helix f16v "), plan
    seqs, offs = gpu.pack_batch(triples)
    assert gpu.workspace_size(len(triples), *ml, p, "pencil") <= ws_bytes
    d_seqs, d_offs = torch.from_numpy(seqs).cuda(), torch.from_numpy(offs).cuda()
    d_sc = torch.zeros(len(triples), dtype=torch.int32, device="cuda")
    gpu.score_batch_async(d_seqs.data_ptr(), d_offs.data_ptr(), len(triples), *ml, d_sc.data_ptr(),
                          d_ws.data_ptr(), ws_bytes, torch.cuda.current_stream().cuda_stream, p, "pencil")
    torch.cuda.synchronize()
    return d_sc.cpu().numpy(), seqs, offs, plan


@pytest.mark.parametrize("s3_mode", [0, 1])
@pytest.mark.parametrize("dims,n", SHAPES)
def test_poisoned_workspace(gpu, orc, dims, n, s3_mode):
    import torch
    _helix(gpu)
    p, op = gpu.TsaParams.default(s3_mode=s3_mode), orc.default_params(s3_mode=s3_mode)
    rng = np.random.default_rng(1000 * dims[0] + 10 * dims[1] + dims[2] + s3_mode)
    triples = _ragged(rng, n, dims)
    ws_bytes = gpu.workspace_size(n, *dims, p, "pencil")
    d_ws = _poisoned(torch, ws_bytes)
    got, seqs, offs, plan = _launch(gpu, torch, triples, p, d_ws, ws_bytes)
    assert ("two" in plan.split()) == (dims[2] <= 64), plan
    assert np.array_equal(got, orc.score_batch(seqs, offs, op, nthreads=8)), (plan, got)


@pytest.mark.parametrize("s3_mode", [0, 1])
def test_workspace_reuse(gpu, orc, s3_mode):
    """Two different ragged batches back to back in one workspace, the second
    shorter than the first in every dimension (another lap period and ring
    stride): the rows the first left behind must not reach the second."""
    import torch
    _helix(gpu)
    p, op = gpu.TsaParams.default(s3_mode=s3_mode), orc.default_params(s3_mode=s3_mode)
    rng = np.random.default_rng(50 + s3_mode)
    first, second = _ragged(rng, 6, (300, 26, 256)), _ragged(rng, 5, (180, 19, 140))
    ws_bytes = gpu.workspace_size(6, 300, 26, 256, p, "pencil")
    d_ws = _poisoned(torch, ws_bytes)
    for triples in (first, second, first):
        got, seqs, offs, plan = _launch(gpu, torch, triples, p, d_ws, ws_bytes)
        assert np.array_equal(got, orc.score_batch(seqs, offs, op, nthreads=8)), (plan, got)


@pytest.mark.parametrize("la", [253, 254, 255, 256, 257])
def test_lap_wrap_at_every_group_phase(gpu, orc, la):
    """LA around the position count with LB = 17, LC = 256: the lap wrap falls
    on every phase of the four-step group, real positions next to padding."""
    import torch
    _helix(gpu)
    p = gpu.TsaParams.default()
    rng = np.random.default_rng(la)
    triples = [tuple(rng.integers(0, 4, d).astype(np.uint8) for d in (la, 17, 256)) for _ in range(2)]
    ws_bytes = gpu.workspace_size(2, la, 17, 256, p, "pencil")
    got, seqs, offs, plan = _launch(gpu, torch, triples, p, _poisoned(torch, ws_bytes), ws_bytes)
    assert np.array_equal(got, orc.score_batch(seqs, offs, orc.default_params(), nthreads=8)), (plan, got)
