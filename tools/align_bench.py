#!/usr/bin/env python3
"""Wall time of batched traceback: tsa_align_batch under align_mode=resident
and align_mode=plane, and a loop of tsa_align_gpu over the same triples, in
ONE process with the passes interleaved (every pass runs each form once, in
turn), after warm-up passes that are not timed. All three calls are
synchronous, so host wall time is the time a caller waits.
  python tools/align_bench.py --n 512 --la 64 --lb 64 --lc 64
  python tools/align_bench.py --n 64 --la 64 --related
  python tools/align_bench.py --n 256 --la 256 --forms tiled,plane
  python tools/align_bench.py --n 256 --la 256 --forms tiled,strip
  python tools/align_bench.py --n 8 --la 512 --forms tiled,strip --tb-bytes 1073741824
  python tools/align_bench.py --n 8 --la 512 --forms tiled,strip,grid --tb-bytes 536870912
  python tools/align_bench.py --n 1 --la 1024 --forms strip,grid --passes 1 --warmup 0
(a form other than loop is passed to align_mode as it stands: resident, plane,
tiled, strip or grid; --tb-bytes sets align_tb_bytes for every batch form, and a form
the library refuses, such as tiled with a cube over that budget, is recorded
with its error instead of a time).
--async adds, for every batch form but plane, a leg through tsa_align_batch_async
(<form>_async_ms): the same batch with its sequences and offsets already on
the device and a full_bytes workspace, timed with one event pair around a train
of --train calls on one stream and divided by the train, next to the
synchronous leg in the same process; its results stay on the device, which the
synchronous leg's do not. The form names the path of the larger triples
(resident: no larger ones are expected, path tiled).
  python tools/align_bench.py --n 512 --la 64 --forms resident --async
  python tools/align_bench.py --n 256 --la 128 --forms tiled --async
--end adds, for every batch form, a leg through tsa_align_batch_ends per listed
end mode (<form>_end_<mode>_ms): corner runs tsa_align_batch's own path and
must cost what the plain leg costs; face and any run the kernels that search
the end cell as they sweep (resident and tiled only). Their results differ
from the corner's by design, so only the corner leg joins the cross-check. A
library without tsa_align_batch_ends (the parent of a comparison) skips them.
The grid form's end legs go through tsa_align_batch_grid_ends
(align_batch_ends(grid=True)); --core-tails makes triples whose end lies far
from the corner: a shared first half and unrelated second halves.
  python tools/align_bench.py --n 512 --la 64 --forms resident --end corner,face,any
  python tools/align_bench.py --n 256 --la 128 --forms tiled --end corner,face,any
  python tools/align_bench.py --n 256 --la 128 --forms grid,tiled --end corner,face,any
  python tools/align_bench.py --n 8 --la 512 --forms grid --end corner,face,any --core-tails --tb-bytes 536870912
--async together with --end adds, for the forms resident, tiled and grid, a leg
through tsa_align_batch_ends_async per listed end mode
(<form>_async_end_<mode>_ms), timed by the train and event scheme of the async
leg, so one process holds the async corner leg (<form>_async_ms), the
device-resident end-free legs and the synchronous ones; ends_async_agree says
that every such leg returned what its synchronous leg returned, ends included.
A library without tsa_align_batch_ends_async (the parent of a comparison) skips
them.
  python tools/align_bench.py --n 512 --la 64 --forms resident --async --end corner,face,any
  python tools/align_bench.py --n 256 --la 128 --forms grid --async --end corner,face,any
A library without tsa_align_batch (an older build named by TSA_PKG_DIR) runs
the loop alone: that is how the baseline of a comparison is taken.
Prints one JSON line: per form the median, min and max of the passes in ms."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--la", type=int, default=64)
    ap.add_argument("--lb", type=int, default=None)
    ap.add_argument("--lc", type=int, default=None)
    ap.add_argument("--related", action="store_true", help="related triples (B, C = mutated A), cubes only")
    ap.add_argument("--core-tails", action="store_true",
                    help="cubes whose sequences share their first half and have unrelated second halves")
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--loop-n", type=int, default=None, help="triples of the align loop (default: all)")
    ap.add_argument("--forms", default="resident,plane,loop",
                    help="comma list of loop and align_mode values: resident, plane, tiled, strip, grid")
    ap.add_argument("--tb-bytes", type=int, default=None, help="align_tb_bytes of the batch forms")
    ap.add_argument("--async", dest="async_", action="store_true",
                    help="add the tsa_align_batch_async leg of every batch form")
    ap.add_argument("--train", type=int, default=10, help="calls between the two events of an async pass")
    ap.add_argument("--end", default="", help="comma list of end modes (corner, face, any): tsa_align_batch_ends legs")
    args = ap.parse_args()
    import bench
    tsa = bench.load_pkg()
    import tsa_amd.synth as synth
    la = args.la
    lb = la if args.lb is None else args.lb
    lc = la if args.lc is None else args.lc
    if args.related:
        trips = [synth.related_triple(900 + i, la) for i in range(args.n)]
        lb = lc = la
    elif args.core_tails:
        import numpy as np
        lb = lc = la
        trips = []
        for i in range(args.n):
            rng = np.random.default_rng(900 + i)
            core = rng.integers(0, 4, la // 2).astype(np.uint8)
            # a tail of one symbol per sequence, each its own: no tail symbol matches another sequence's tail
            trips.append(tuple(np.concatenate([core, np.full(la - la // 2, k + 1, np.uint8)]) for k in range(3)))
    else:
        trips = [synth.triple(i, la, lb, lc) for i in range(args.n)]
    seqs, offs = tsa.pack_batch(trips)
    loop_n = args.n if args.loop_n is None else min(args.loop_n, args.n)
    have_batch = hasattr(tsa, "align_batch")

    def batch(mode):
        def run():
            ov = dict(align_mode=mode)
            if args.tb_bytes is not None:
                ov["align_tb_bytes"] = args.tb_bytes
            with tsa.overrides(**ov):
                return tsa.align_batch(seqs=seqs, offsets=offs)
        return run

    def batch_ends(mode, end):
        def run():
            ov = dict(align_mode=mode)
            if args.tb_bytes is not None:
                ov["align_tb_bytes"] = args.tb_bytes
            with tsa.overrides(**ov):
                if mode == "grid":                   # tsa_align_batch_grid_ends
                    return tsa.align_batch_ends(seqs=seqs, offsets=offs, end=end, grid=True)
                return tsa.align_batch_ends(seqs=seqs, offsets=offs, end=end)
        return run

    def loop():
        return [tsa.align(a, b, c) for a, b, c in trips[:loop_n]]

    dev = {}

    def device_leg(mode, end=None):
        """tsa_align_batch_async (tsa_align_batch_ends_async with `end`) on
        device-resident inputs; returns (results, timed)."""
        import torch
        if not dev:
            dev["seqs"], dev["offs"] = torch.from_numpy(seqs).cuda(), torch.from_numpy(offs).cuda()
            dev["out"] = (torch.zeros(args.n, dtype=torch.int32, device="cuda"),
                          torch.zeros(len(seqs), dtype=torch.uint8, device="cuda"),
                          torch.zeros(args.n, dtype=torch.int32, device="cuda"),
                          torch.zeros(3 * args.n, dtype=torch.int32, device="cuda"))
            dev["ends"] = torch.zeros(3 * args.n, dtype=torch.int32, device="cuda")
        path = "tiled" if mode == "resident" else mode
        ws_bytes = (tsa.align_workspace_size(offs, path=path) if end is None else
                    tsa.align_ends_workspace_size(offs, path=path, end=end))[1]
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
        sc, mv, nm, st = dev["out"]
        en = dev["ends"]

        def queue():
            if end is not None:
                tsa.align_batch_ends_async(dev["seqs"].data_ptr(), dev["offs"].data_ptr(), offs, sc.data_ptr(),
                                           mv.data_ptr(), nm.data_ptr(), st.data_ptr(), en.data_ptr(), ws.data_ptr(),
                                           ws_bytes, torch.cuda.current_stream().cuda_stream, path=path, end=end)
                return
            tsa.align_batch_async(dev["seqs"].data_ptr(), dev["offs"].data_ptr(), offs, sc.data_ptr(), mv.data_ptr(),
                                  nm.data_ptr(), st.data_ptr(), ws.data_ptr(), ws_bytes,
                                  torch.cuda.current_stream().cuda_stream, path=path)

        def results():
            queue()
            torch.cuda.synchronize()
            h = [t.cpu().numpy() for t in (sc, mv, nm, st, en)]
            return [(int(h[0][i]), tuple(h[3][3 * i:3 * i + 3]), h[1][int(offs[3 * i]):int(offs[3 * i]) + int(h[2][i])]) +
                    ((tuple(h[4][3 * i:3 * i + 3]),) if end is not None else ())
                    for i in range(args.n)]

        def timed():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.train):
                queue()
            t1.record()
            t1.synchronize()
            return t0.elapsed_time(t1) / args.train
        return results, timed

    forms, timers = {}, {}
    for f in args.forms.split(","):
        if f == "loop":
            forms[f] = loop
        elif have_batch:
            forms[f] = batch(f)
            if args.async_ and f != "plane" and hasattr(tsa, "align_batch_async"):
                forms[f + "_async"], timers[f + "_async"] = device_leg(f)
            for e in filter(None, args.end.split(",")):
                if hasattr(tsa, "align_batch_ends") and (f != "grid" or "tsa_align_batch_grid_ends" in tsa.EXPORTS):
                    forms["%s_end_%s" % (f, e)] = batch_ends(f, e)
                    if args.async_ and f in ("resident", "tiled", "grid") and hasattr(tsa, "align_batch_ends_async"):
                        name = "%s_async_end_%s" % (f, e)
                        forms[name], timers[name] = device_leg(f, e)
    out, refused = {}, {}
    for f, fn in list(forms.items()):                # first call: also the cross-check
        try:
            out[f] = fn()
        except tsa.TsaError as e:                    # e.g. TSA_ENOMEM: the form cannot run this batch
            refused[f] = str(e)
            del forms[f]
    names = [f for f in out if not f.endswith(("_end_face", "_end_any"))]
    same = True
    for f in names[1:]:
        for g, r in zip(out[f], out[names[0]]):
            same = same and g[0] == r[0] and tuple(g[1]) == tuple(r[1]) and bool((g[2] == r[2]).all())
    ends_agree = None                                # every device-resident end leg against its synchronous leg
    for f in out:
        sync = f.replace("_async_end_", "_end_")
        if "_async_end_" in f and sync in out:
            ends_agree = ends_agree is not False and all(
                g[0] == r[0] and tuple(g[1]) == tuple(r[1]) and bool((g[2] == r[2]).all()) and tuple(g[3]) == tuple(r[3])
                for g, r in zip(out[f], out[sync]))
    times = {f: [] for f in forms}
    for k in range(args.warmup + args.passes):
        for f, fn in forms.items():
            if f in timers:                          # device time of one call of a train
                dt = timers[f]()
            else:
                t0 = time.perf_counter()
                fn()
                dt = (time.perf_counter() - t0) * 1e3
            if k >= args.warmup:
                times[f].append(dt)
    res = {"bench": "align", "n": args.n, "shape": [la, lb, lc], "related": bool(args.related),
           "core_tails": bool(args.core_tails), "passes": args.passes, "warmup": args.warmup, "loop_n": loop_n, "forms_agree": same,
           "version": tsa.version()}
    if args.tb_bytes is not None:
        res["tb_bytes"] = args.tb_bytes
    if timers:
        res["train"] = args.train
    if ends_agree is not None:
        res["ends_async_agree"] = ends_agree
    for f, why in refused.items():
        res[f + "_error"] = why
    for f, ts in times.items():
        scale = args.n / loop_n if f == "loop" else 1.0  # a shortened loop, scaled to the batch
        res[f + "_ms"] = {"median": round(statistics.median(ts) * scale, 3), "min": round(min(ts) * scale, 3),
                          "max": round(max(ts) * scale, 3)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
