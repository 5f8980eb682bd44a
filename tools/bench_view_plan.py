#!/usr/bin/env python3
"""find -> match for the 256 new frames of a step against 32 views each (cap 8 192, the place parameters at their defaults), two
ways in one process, alternating, on one MI355X:

  planned   FrameIndex.find, Registration.match_found: the views are chosen, the distinct blocks counted and the recoding plan
            written on the device (hm_view_plan_device, hm_knn_planned_batch_device, hm_best_of_views_planned_batch_device);
            the host enqueues and returns.
  host      the way before it: FrameIndex.find, hm_sync, place_recognition.view_blocks (two copies to the host, a Python loop,
            one upload), Registration.match_views.

Time: HIP events on hm_stream() from in front of the find to behind the best-of-views decision (for `host` the stream's idle time
during the host step is inside), and wall time from the first call to the return of a final hm_sync.  Median of --rounds after a
warm-up.  Then hm_view_plan_device alone (its three launches and one clear).  Two tables: `full`, every frame finds 32 views;
`half`, every second frame finds 8 — where `host` repeats the last view 24 times and searches each repeat, and `planned`
leaves 24 dead problems.  The decisions of both ways are compared once per table.  Prints one line per table and one JSON line.
Nothing is asserted about the ratio."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cv_amd import build  # noqa: E402
build.build()
import torch  # noqa: E402
from cv_amd import _device, _lib, place_recognition as P  # noqa: E402
from cv_amd.registration import Registration  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=256)
ap.add_argument("--views", type=int, default=32)
ap.add_argument("--cap", type=int, default=8192)
ap.add_argument("--view-blocks", type=int, default=64, help="distinct stored blocks the views name")
ap.add_argument("--rounds", type=int, default=20)
ap.add_argument("--tables", nargs="+", default=["full", "half"])
args = ap.parse_args()

dev = torch.device("cuda", 0)
L = _lib.lib()
F, V, cap, NV = args.frames, args.views, args.cap, args.view_blocks
n_blocks = NV + F
rng = np.random.default_rng(0x5650)
g = torch.Generator(device=dev).manual_seed(0x5650)
d_descs = torch.randint(0, 256, (n_blocks, cap, 64), dtype=torch.uint8, device=dev, generator=g)
d_counts = torch.full((n_blocks,), cap, dtype=torch.int32, device=dev)
d_landmarks = torch.randint(0, 1 << 20, (n_blocks, cap), dtype=torch.int32, device=dev, generator=g)
codewords = rng.integers(0, 256, (256, 64), dtype=np.uint8)
reg = Registration(torch, cap, F, V, codewords, (1000.0, 1000.0, 640.0, 360.0, 0.0, None), n_hypotheses=256, max_candidates=64,
                   estimations_per_block=16, block_size=32)
hm_s = torch.cuda.ExternalStream(reg.hm_stream(), device=dev)
prm = P.params()
frame_blocks = list(range(NV, NV + F))


def table(kind):
    """feed f holds frame f in the middle of its stored frames, all views of reconstruction 1: V of them, or 8 for every second
    feed of `half`; the views name the NV stored blocks, neighbouring feeds mostly the same ones"""
    feed, pos, recon, view, queries = [], [], [], [], []
    for f in range(F):
        n = 8 if (kind == "half" and f % 2) else V
        for s in range(n + 1):
            if s == n // 2:
                queries.append(len(feed))
                feed.append(f); pos.append(s); recon.append(P.NONE); view.append(0)
            else:
                feed.append(f); pos.append(s); recon.append(1); view.append((f // 8 + s) % NV)
    n = len(feed)
    idx = P.FrameIndex(torch, reg.matcher, n, hash_bytes=512)
    idx.append_rows(np.array(feed, np.uint32), np.array(pos, np.uint32), rng.integers(0, 256, (n, 512), dtype=np.uint8))
    idx.set_views(np.arange(n), np.array(recon, np.uint32), np.array(view, np.uint32))
    return idx, torch.from_numpy(np.array(queries, np.int32)).to(dev)


def timed(body):
    """-> (HIP-event ms on hm_stream(), wall ms until a final hm_sync has returned)"""
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record(hm_s)
    body()
    e1.record(hm_s)
    _lib.check(L.hm_sync(reg.matcher.handle), "hm_sync")
    wall = (time.perf_counter() - t0) * 1e3
    e1.synchronize()
    return e0.elapsed_time(e1), wall


results = {}
for kind in args.tables:
    idx, d_q = table(kind)

    def planned():
        found = idx.find(d_q, prm)
        reg.match_found(d_descs, d_counts, frame_blocks, found, d_landmarks)

    def host():
        found = idx.find(d_q, prm)
        _lib.check(L.hm_sync(reg.matcher.handle), "hm_sync")
        reg.match_views(d_descs, d_counts, frame_blocks, P.view_blocks(found, V).tolist(), d_landmarks)

    def outputs(way):
        timed(way)
        return reg.best.cpu().numpy().tobytes(), reg.decision.cpu().numpy().tobytes()

    same = outputs(planned) == outputs(host)                       # warm-up of both, and the comparison
    outputs(planned), outputs(host)                                # (the second output set of each)
    counts = reg.plan.counts.cpu().tolist() if hasattr(reg, "plan") else None
    tp, th = [], []
    for _ in range(args.rounds):
        tp.append(timed(planned))
        th.append(timed(host))
    plan = reg.plan
    found = idx.find(d_q, prm)
    _lib.check(L.hm_sync(reg.matcher.handle), "hm_sync")

    def plan_alone():
        _device.call("hm_view_plan_device", reg.matcher.handle, found.views_out, found.group_recon, found.group_start, found.counts, found.verdict,
                     found.room, None, 0, F, V, n_blocks, plan.exp_blocks, plan.view_idx, plan.n_views, plan.verdict, plan.counts, None)

    timed(plan_alone)
    tpl = [timed(plan_alone) for _ in range(args.rounds)]
    med = lambda ts, k: round(float(np.median([t[k] for t in ts])), 3)
    e = {"planned_ms": {"events": med(tp, 0), "wall": med(tp, 1)}, "host_ms": {"events": med(th, 0), "wall": med(th, 1)},
         "plan_alone_ms": {"events": med(tpl, 0), "wall": med(tpl, 1)}, "plan_counts": counts, "same_decisions": same}
    results[kind] = e
    print(f"{kind}: planned {e['planned_ms']['events']} ms events / {e['planned_ms']['wall']} ms wall; host {e['host_ms']['events']} / "
          f"{e['host_ms']['wall']} ms; the plan alone {e['plan_alone_ms']['events']} ms events / {e['plan_alone_ms']['wall']} ms wall; "
          f"plan counts {counts}; same decisions: {same}", flush=True)
print(json.dumps({"workload": f"find -> match: {F} frames x {V} views, cap {cap}, {NV} stored blocks, place parameters at their defaults",
                  "rounds": args.rounds, "tables": results,
                  "time": "median; events: HIP events on hm_stream() around find .. best-of-views; wall: first call .. hm_sync returned"}))
reg.close()
