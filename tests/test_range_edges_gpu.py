"""Every score arithmetic at the edge of its admission, on the GPU.

tests/test_range_proof.py pins where the host's range proof
switches the plan and shows, on the oracle, that the values really reach the
limits there. Here the kernels run at those sizes: each row is one edge, given
by parameter set (tests/_range_cases.py), schedule and shape. A row first
asserts the plan's arithmetic (a drifted predicate then fails loudly instead of
silently testing another kernel), then requires scores equal to the oracle's.

On the helix a row is a batch of three: the extreme input at the full lengths,
a second extreme family at the full lengths, and a ragged shorter random
triple, so the proof's use of the MAXIMUM lengths is exercised. On the lap the
two full-length triples run as single cubes. kernel="pencil" where it is
admitted, kernel="auto" one past the edge.

  * f16 top: (3, 1) at 224^3, (2, 0) at 337^3 (the helix at M = 4); 225^3 and
    338^3 plan int16.
  * V-space top: (0, -2, 3, 2) at (377, 377, 256) (the integer-pattern cell's
    last shape; V-space faces reach 2020, + slack 28 = 2048) and (378, 378, 256);
    the lap's opt-in V-space cell (lap_vs = 1) at 338^3 (default set, the upper
    end) and 334^3 ((0, -2, 3, 2), the lower end).
  * int16 top: (40, -1) at 270^3 (values to 32400, + slack 328); 271^3 is
    refused and auto runs the literal plan.
  * the 12-bit word's top in int16: (2, 0) at 341^3 (values to 2046); at 342^3
    the all-match score 2052 no longer fits and the literal result differs from
    the unwrapped one; (10, 8) at 56^3 and 57^3 with a = b != c (RTL s3: 36 a
    cell).
  * the literal kernels at the int16 top: (40, -1), score_bits = 0, 273^3.
  * the split cube at 270^3 (factored) and 271^3 (literal) of (40, -1).
References come from the oracle, eight threads, once per row for the module.
"""
import numpy as np
import pytest

from _range_cases import SETS, family, plan_token

pytestmark = pytest.mark.gpu

# (set, dims, kernel, arithmetic under helix, under lap, the two full-length families)
ROWS = [
    ("m3_mm1_b16", (224, 224, 224), "pencil", "f16", "f16", ("all-match", "a=b")),
    ("m3_mm1_b16", (225, 225, 225), "pencil", "i16", "i16", ("all-match", "a=b")),
    ("m2_mm0", (337, 337, 337), "pencil", "f16", "f16", ("all-match", "a=b")),
    ("m2_mm0", (338, 338, 338), "pencil", "i16", "i16", ("all-match", "a=b")),
    ("lam2_b16", (377, 377, 256), "pencil", "f16v int", "f16", ("all-match", "all-distinct")),
    ("lam2_b16", (378, 378, 256), "pencil", "f16", "f16", ("all-match", "all-distinct")),
    ("m40_b16", (270, 270, 270), "pencil", "i16", "i16", ("all-match", "all-distinct")),
    ("m40_b16", (271, 271, 271), "auto", "plane", "plane", ("all-match", "all-distinct")),
    ("m2_mm0", (341, 341, 341), "pencil", "i16", "i16", ("all-match", "a=b")),
    ("m2_mm0", (342, 342, 342), "auto", "plane", "plane", ("all-match", "a=b")),
    ("m10_mm8", (56, 56, 56), "pencil", "i16", "i16", ("a=b", "all-match")),
    ("m10_mm8", (57, 57, 57), "auto", "plane", "plane", ("a=b", "all-match")),
]
# the lap kernel's V-space cell under lap_vs = 1: its last admitted cube, and one past
LAP_VS_ROWS = [
    ("default", (338, 338, 338), "f16v", ("all-match", "all-distinct")),
    ("default", (339, 339, 339), "f16", ("all-match", "all-distinct")),
    ("lam2_b16", (334, 334, 334), "f16v", ("all-match", "all-distinct")),
    ("lam2_b16", (335, 335, 335), "i16", ("all-match", "all-distinct")),
]
# known answers at the very top (the oracle must agree with the arithmetic of the issue)
KNOWN = {("m3_mm1_b16", 224): 2016, ("m2_mm0", 337): 2022, ("m2_mm0", 341): 2046, ("m40_b16", 270): 32400,
         ("m10_mm8", 56): 2016}
# One past the 12-bit word the unwrapped score would be 2052. The candidate that carries it wraps to
# 2052 - 4096, and MAX7 then takes the largest candidate that did not wrap (2046 from the pair states of
# the diagonal cell at 342^3, 2024 at 57^3): the literal score differs from the unwrapped one.
UNWRAPPED = {("m2_mm0", 342): 2052, ("m10_mm8", 57): 2052}


def _id(row):
    return row[0] + "-" + "x".join(map(str, row[1]))


_REF = {}


def _case(gpu, orc, name, dims, kinds):
    """The row's three triples and their oracle scores."""
    key = (name, dims, kinds)
    if key not in _REF:
        rng = np.random.default_rng([len(_REF), *dims])
        ragged = tuple(rng.integers(0, 4, int(rng.integers(max(1, d // 2), d))).astype(np.uint8) for d in dims)
        triples = [family(kinds[0], dims), family(kinds[1], dims), ragged]
        seqs, offs = gpu.pack_batch(triples)
        ref = orc.score_batch(seqs, offs, orc.default_params(**SETS[name]), nthreads=8)
        if (name, dims[0]) in KNOWN:
            assert ref[0] == KNOWN[(name, dims[0])], (name, dims, ref)
        if (name, dims[0]) in UNWRAPPED:
            assert ref[0] != UNWRAPPED[(name, dims[0])], (name, dims, ref)
        _REF[key] = (triples, ref)
    return _REF[key]


def _score_async(gpu, triples, dims, p, kernel):
    import torch
    n = len(triples)
    seqs, offs = gpu.pack_batch(triples)
    ws = gpu.workspace_size(n, *dims, p, kernel)
    d_ws = torch.empty(max(ws, 16), dtype=torch.uint8, device="cuda")
    d_seqs, d_offs = torch.from_numpy(seqs).cuda(), torch.from_numpy(offs).cuda()
    d_sc = torch.zeros(n, dtype=torch.int32, device="cuda")
    gpu.score_batch_async(d_seqs.data_ptr(), d_offs.data_ptr(), n, *dims, d_sc.data_ptr(), d_ws.data_ptr(), ws,
                          torch.cuda.current_stream().cuda_stream, p, kernel)
    torch.cuda.synchronize()
    return d_sc.cpu().numpy()


@pytest.mark.parametrize("row", ROWS, ids=_id)
def test_helix_edge(gpu, orc, row):
    name, dims, kernel, token, _, kinds = row
    p = gpu.TsaParams.default(**SETS[name])
    triples, ref = _case(gpu, orc, name, dims, kinds)
    gpu.set_override("pencil_mode", "helix")
    plan = gpu.describe_plan(3, *dims, p, kernel, sync=False)
    assert plan_token(gpu, 3, dims, p, kernel) == token, plan
    assert plan_token(gpu, 3, dims, p, "pencil") == ("refused" if kernel == "auto" else token), plan
    if token != "plane":
        assert plan.startswith("pencil helix "), plan
    if name == "m2_mm0" and token == "f16":
        assert " M=4 " in plan, plan
    got = _score_async(gpu, triples, dims, p, kernel)
    print(plan, "scores", got.tolist(), "oracle", ref.tolist())
    assert np.array_equal(got, ref), (plan, got, ref)


@pytest.mark.parametrize("row", ROWS, ids=_id)
def test_lap_edge(gpu, orc, row):
    name, dims, kernel, _, token, kinds = row
    p = gpu.TsaParams.default(**SETS[name])
    triples, ref = _case(gpu, orc, name, dims, kinds)
    gpu.set_override("pencil_mode", "lap")
    plan = gpu.describe_plan(1, *dims, p, kernel, sync=False)
    assert plan_token(gpu, 1, dims, p, kernel) == token, plan
    assert plan_token(gpu, 1, dims, p, "pencil") == ("refused" if kernel == "auto" else token), plan
    if token != "plane":
        assert plan.startswith("pencil lap "), plan
    for t, want in zip(triples[:2], ref[:2]):
        got = _score_async(gpu, [t], dims, p, kernel)
        print(plan, "score", got.tolist(), "oracle", int(want))
        assert got[0] == want, (plan, got, want)


@pytest.mark.parametrize("row", LAP_VS_ROWS, ids=_id)
def test_lap_vspace_edge(gpu, orc, row):
    name, dims, token, kinds = row
    p = gpu.TsaParams.default(**SETS[name])
    triples, ref = _case(gpu, orc, name, dims, kinds)
    gpu.set_override("pencil_mode", "lap")
    gpu.set_override("lap_vs", 1)
    plan = gpu.describe_plan(1, *dims, p, "pencil", sync=False)
    assert plan.startswith("pencil lap ") and plan_token(gpu, 1, dims, p) == token, plan
    for t, want in zip(triples[:2], ref[:2]):
        got = _score_async(gpu, [t], dims, p, "pencil")
        print(plan, "score", got.tolist(), "oracle", int(want))
        assert got[0] == want, (plan, got, want)


def test_checked_kernel_one_past_the_word(gpu, orc):
    """(2, 0) at 342^3 on the synchronous path: auto plans the checked kernel,
    which cannot certify the all-match cube (2052 leaves the 12-bit word; the
    literal score is 2046) and has it rescored literally (counted), and
    certifies a = b != c (values to 4 * 342 = 1368) -- both equal to the oracle."""
    name, dims, kinds = "m2_mm0", (342, 342, 342), ("all-match", "a=b")
    p = gpu.TsaParams.default(**SETS[name])
    triples, ref = _case(gpu, orc, name, dims, kinds)
    gpu.set_override("pencil_mode", "lap")
    assert plan_token(gpu, 1, dims, p, "auto", sync=True) == "i16 checked"
    before = gpu.check_fallback_count()
    assert gpu.score(*triples[0], p) == ref[0] == 2046
    assert gpu.check_fallback_count() == before + 1
    assert gpu.score(*triples[1], p) == ref[1] == 4 * 342
    assert gpu.check_fallback_count() == before + 1


@pytest.mark.parametrize("mode,prefix", [("litlap", "plane literal-lap "), ("literal", "plane literal-helix "),
                                         ("plane", "plane est=")])
def test_literal_kernels_at_the_int16_top(gpu, orc, mode, prefix):
    """(40, -1), score_bits = 0: the all-match 273^3 cube, the last one
    tsa_validate admits, scores 32760 with int16 states up to 32760, on every
    literal kernel; score and final states equal the oracle's."""
    name, L = "m40_b0", 273
    p = gpu.TsaParams.default(**SETS[name])
    a, b, c = family("all-match", (L, L, L))
    key = ("literal", L)
    if key not in _REF:
        _REF[key] = orc.score(a, b, c, orc.default_params(**SETS[name]), final_states=True)
    want = _REF[key]
    assert want[0] == 32760
    gpu.set_override("pencil_mode", mode)
    plan = gpu.describe_plan(1, L, L, L, p, "plane", sync=True)
    assert plan.startswith(prefix), plan
    assert plan_token(gpu, 1, (L, L, L), p, "pencil") == "refused"
    got = gpu.score(a, b, c, p, kernel="plane", final_states=True)
    print(plan, got)
    assert got == want, (plan, got, want)


@pytest.mark.parametrize("L,exact", [(270, True), (271, False)])
def test_split_cube_edge(gpu, orc, L, exact):
    """score_multi over devices (0, 0) of (40, -1): the factored split at 270^3,
    the literal one at 271^3 (the choice follows pencil_exact, as the plan of
    kernel="pencil" does)."""
    name, dims, kinds = "m40_b16", (L, L, L), ("all-match", "all-distinct")
    p = gpu.TsaParams.default(**SETS[name])
    triples, ref = _case(gpu, orc, name, dims, kinds)
    assert (plan_token(gpu, 1, dims, p, "pencil") != "refused") == exact
    for t, want in zip(triples[:2], ref[:2]):
        got, _ = gpu.score_multi(*t, [0, 0], p)
        assert got == want, (L, got, want)
