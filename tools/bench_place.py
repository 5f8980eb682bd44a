#!/usr/bin/env python3
"""Choosing the frames a frame is compared with, for the 256 frames of a step: hm_find_frames_batch_device over a resident frame
table (one call, HIP-event time on hm_stream()) beside the only path that gave the same search lists before it, 256 calls of
hm_hash_knn over the same store (wall time: each call uploads the store and waits), alternating in one process, on one MI355X.
512-byte hashes, the reference's defaults with num_similar = 8, n_stored = 1 000, 10 000 and 100 000.  The search lists of both
paths are compared on the first queries.  Prints one line per size and one JSON line; the condition is that the batched call is
the faster at all three sizes.

The VALU share is a count from the source, not a counter: nq x n_stored x (hash_bytes / 4) word pairs, two lane-instructions each
(xor, accumulating population count), over the call's time and the four-cycle issue rate tools/roofline.py uses."""
import argparse
import ctypes as C
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
from cv_amd import _lib, place_recognition as P  # noqa: E402
from cv_amd.knn import Matcher  # noqa: E402
from tools.roofline import VALU_ISSUE_PEAK_T  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", type=int, nargs="+", default=[1000, 10000, 100000])
ap.add_argument("--queries", type=int, default=256)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--hash-bytes", type=int, default=512)
ap.add_argument("--checked", type=int, default=4, help="queries whose search lists are compared between the two paths")
args = ap.parse_args()

dev = torch.device("cuda", 0)
L = _lib.lib()
m = Matcher(64)
hm_s = torch.cuda.ExternalStream(L.hm_stream(m.handle), device=dev)
prm = P.params(num_similar=8)
nq, hb = args.queries, args.hash_bytes
results = []
for n in args.sizes:
    rng = np.random.default_rng([0x504C, n])
    hashes = rng.integers(0, 256, (n, hb), dtype=np.uint8)
    feed, pos = (np.arange(n) % 4).astype(np.uint32), (np.arange(n) // 4).astype(np.uint32)
    idx = P.FrameIndex(torch, m, n, hash_bytes=hb)
    idx.append_rows(feed, pos, hashes)
    idx.set_views(np.arange(n), np.where(np.arange(n) % 3 == 0, P.NONE, 1 + np.arange(n) % 5).astype(np.uint32), np.arange(n, dtype=np.uint32))
    queries = np.sort(rng.choice(n, nq, replace=nq > n)).astype(np.uint32)
    d_q = torch.from_numpy(queries.view(np.int32)).to(dev)
    torch.cuda.synchronize()

    r = idx.find(d_q, prm, search=True)                          # the outputs, allocated once; warm-up
    _lib.check(L.hm_sync(m.handle), "hm_sync")

    def batched():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(hm_s)
        idx.find_device(d_q, None, nq, prm, r.room, r.found, r.views_out, r.group_recon, r.group_start, r.free, r.search, r.counts, r.verdict)
        e1.record(hm_s)
        e1.synchronize()
        return e0.elapsed_time(e1)

    out = np.zeros(prm.search_num, _lib.NB_DTYPE)
    n_out = C.c_uint32(0)

    def one_by_one(keep=0):
        kept = []
        t0 = time.perf_counter()
        for j in range(nq):
            _lib.check(L.hm_hash_knn(m.handle, hashes[queries[j]].ctypes.data, hashes.ctypes.data, n, hb, prm.search_num, out.ctypes.data,
                                     C.byref(n_out)), "hm_hash_knn")
            if j < keep:
                kept.append(out[:n_out.value].copy())
        return (time.perf_counter() - t0) * 1e3, kept

    batched()                                                    # warm-up of both, and the comparison
    _, kept = one_by_one(keep=args.checked)
    got = r.search.cpu().numpy().view(np.uint32)
    for j, want in enumerate(kept):
        assert np.array_equal(got[j, :len(want), 0], want["index"]) and np.array_equal(got[j, :len(want), 1], want["distance"]), (n, j)
    tb, to = [], []
    for _ in range(args.rounds):
        tb.append(batched())
        to.append(one_by_one()[0])
    lane_ops = 2.0 * nq * n * (hb // 4)
    best, med = min(tb), float(np.median(tb))
    e = {"n_stored": n, "batched_ms": {"best": round(best, 4), "median": round(med, 4)},
         "hm_hash_knn_x%d_ms" % nq: {"best": round(min(to), 3), "median": round(float(np.median(to)), 3)},
         "ratio_median": round(float(np.median(to)) / med, 1),
         "valu_share_of_issue_rate": round(lane_ops / (best * 1e-3) / 1e12 / VALU_ISSUE_PEAK_T, 4)}
    results.append(e)
    print(f"n_stored {n:7d}: batched {best:.3f} ms best / {med:.3f} ms median; {nq} x hm_hash_knn {min(to):.1f} / {np.median(to):.1f} ms; "
          f"ratio {e['ratio_median']}; VALU share (count from the source) {e['valu_share_of_issue_rate']}", flush=True)
ok = all(e["batched_ms"]["median"] < e["hm_hash_knn_x%d_ms" % nq]["median"] for e in results)
print(json.dumps({"workload": f"place recognition: {nq} queries, {hb}-byte hashes, defaults with num_similar = 8, search lists returned",
                  "rounds": args.rounds, "sizes": results, "batched_faster_at_every_size": ok,
                  "valu_issue_peak_T": VALU_ISSUE_PEAK_T, "time": "HIP events on hm_stream() (batched), wall (hm_hash_knn: each call waits)"}))
m.close()
sys.exit(0 if ok else 1)
