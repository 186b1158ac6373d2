#!/usr/bin/env python3
"""Device time of the end-free score next to the plain score, on the batch
bench.py times (synth.batch(0, n, L): n x L^3), device-resident input.

Legs, interleaved in every pass of ONE process: tsa_score_batch_async
(TSA_KERNEL_PENCIL, the corner score) and tsa_score_batch_ends_async under
face and under any. A pass times, per leg, one train of --train back-to-back
launches on one stream between two events, after --warmup launches of every
leg that are not timed; the figure is the train's time over its length. The
cost of the end search is read against the corner leg of the same pass.
  python tools/score_ends_bench.py --n 512 --L 256
  python tools/score_ends_bench.py --n 512 --L 64 --out profiles/score_ends.jsonl
  python tools/score_ends_bench.py --kernel plane --n 512 --L 256 --out profiles/score_ends_literal.jsonl
--kernel plane times the literal arithmetic instead: the corner leg is the
literal helix score (tsa_score_batch_async, TSA_KERNEL_PLANE under
pencil_mode=literal), the face and any legs its end search
(tsa_score_batch_ends_async_ex, TSA_KERNEL_PLANE).
  python tools/score_ends_bench.py --lap --n 1 --L 1024 --out profiles/score_ends_lap.jsonl
  python tools/score_ends_bench.py --lap --n 8 --L 512 --grid --out profiles/score_ends_lap.jsonl
--lap times the end search of the lap schedule (tsa_score_batch_ends_async_lap)
on a few large cubes: the corner leg is the checked (or, where the factored
form is exact a priori, the plain) lap score of the same cubes
(tsa_score_batch_async, TSA_KERNEL_CHECKED). --grid adds, per pass, one
synchronous tsa_align_batch_grid_ends call (any) on the same cubes, timed on
the host clock: the free-end answer these cubes had before.
Prints one JSON line per process (every pass's figures, and per leg the median,
min and max in ms) and appends it to --out when given. The first call of each
leg is also a check: the corner leg equals tsa_score_batch_ends' corner mode,
and the any leg's score is never below the face leg's, nor that below the corner's."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--L", type=int, default=256)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--train", type=int, default=20)
    ap.add_argument("--kernel", choices=("pencil", "plane"), default="pencil",
                    help="pencil: the factored helix (default); plane: the literal helix and its end search")
    ap.add_argument("--lap", action="store_true", help="the lap schedule: checked lap score, tsa_*_ends_*_lap")
    ap.add_argument("--grid", action="store_true", help="with --lap: also one tsa_align_batch_grid_ends call per pass")
    ap.add_argument("--out", default=None, help="append the JSON line to this file")
    args = ap.parse_args()
    import bench
    tsa = bench.load_pkg()
    kernel = "checked" if args.lap else args.kernel
    # None: the entry points without a kernel argument
    ends_kernel = "lap" if args.lap else None if kernel == "pencil" else kernel
    if kernel == "plane":
        tsa.set_override("pencil_mode", "literal")            # the literal helix for every leg, whatever the cost model
    import torch
    import tsa_amd.synth as synth
    n, L = args.n, args.L
    seqs, offs = synth.batch(0, n, L)
    d_seqs, d_offs = torch.from_numpy(seqs).cuda(), torch.from_numpy(offs).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    legs, outs = {}, {}

    def add(name, ws_bytes, queue_of):
        ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device="cuda")
        sc = torch.zeros(n, dtype=torch.int32, device="cuda")
        en = torch.zeros(3 * n, dtype=torch.int32, device="cuda")
        legs[name] = queue_of(sc, en, ws, ws_bytes)
        outs[name] = (sc, en, ws)

    add("corner", tsa.workspace_size(n, L, L, L, kernel=kernel),
        lambda sc, en, ws, nb: lambda: tsa.score_batch_async(d_seqs.data_ptr(), d_offs.data_ptr(), n, L, L, L,
                                                             sc.data_ptr(), ws.data_ptr(), nb, stream, kernel=kernel))
    for mode in ("face", "any"):
        add(mode, tsa.score_ends_workspace_size(n, L, L, L, end=mode, kernel=ends_kernel),
            lambda sc, en, ws, nb, mode=mode: lambda: tsa.score_batch_ends_async(
                d_seqs.data_ptr(), d_offs.data_ptr(), n, L, L, L, sc.data_ptr(), en.data_ptr(), ws.data_ptr(), nb,
                stream, end=mode, kernel=ends_kernel))
    plans = {"corner": tsa.describe_plan(n, L, L, L, kernel=kernel, sync=False),
             "face": tsa.describe_score_ends_plan(n, L, L, L, end="face", kernel=ends_kernel),
             "any": tsa.describe_score_ends_plan(n, L, L, L, end="any", kernel=ends_kernel)}
    for q in legs.values():          # first call: the check
        q()
    torch.cuda.synchronize()
    h = {k: outs[k][0].cpu().numpy() for k in legs}
    ok = bool((h["any"] >= h["face"]).all() and (h["face"] >= h["corner"]).all())
    k = min(n, 64)                   # the corner against the synchronous entry point, on a part of the batch
    ref = tsa.score_batch_ends(seqs=seqs[:int(offs[3 * k])], offsets=offs[:3 * k + 1], end="corner",
                               kernel=ends_kernel)
    ok = ok and [s for s, _ in ref] == h["corner"][:k].tolist()
    for _ in range(args.warmup):
        for q in legs.values():
            q()
    torch.cuda.synchronize()
    passes = []
    for _ in range(args.passes):
        row = {}
        for name, q in legs.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.train):
                q()
            t1.record()
            t1.synchronize()
            row[name] = round(t0.elapsed_time(t1) / args.train, 4)
        if args.lap and args.grid:   # the grid traceback with a free end: a synchronous host call
            import time
            torch.cuda.synchronize()
            w0 = time.perf_counter()
            grid_res = tsa.align_batch_ends(seqs=seqs, offsets=offs, end="any", grid=True)
            row["grid_any_host"] = round((time.perf_counter() - w0) * 1e3, 3)
            ok = ok and [r[0] for r in grid_res] == h["any"].tolist()
        passes.append(row)
    res = {"bench": "score_ends", "kernel": kernel, "n": n, "shape": [L, L, L], "train": args.train, "warmup": args.warmup,
           "passes": passes, "plans": plans, "legs_consistent": ok, "lap": bool(args.lap), "version": tsa.version(), "pid": os.getpid()}
    for name in list(legs) + (["grid_any_host"] if args.lap and args.grid else []):
        ts = [p[name] for p in passes]
        res[name + "_ms"] = {"median": round(statistics.median(ts), 4), "min": min(ts), "max": max(ts)}
    for name in ("face", "any"):
        res[name + "_over_corner"] = round(statistics.median(p[name] / p["corner"] for p in passes), 3)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
