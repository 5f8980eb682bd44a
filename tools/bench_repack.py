#!/usr/bin/env python3
"""Times of the repack of a reconstruction (cv_amd/csrc/rs_repack.hip) against the host build of the same header on one core.
It has no part in bench.py.

  python tools/bench_repack.py [--repeat 20]
        one child process under `timeout`.  The 50 000-landmark table of tests/test_gpu_triangulate.py's big_map (805 902
        observations, lists of 0 to 48 — the one tools/bench_observation_filter.py times the filter on) with every second
        observation of a view moved to a second view (132 views), one empty row in ten (tombstones), the empty tail of 64
        frames that never registered, and one view removed.  rs_repack_table_device and, in the same run, the yardsticks —
        rs_add_views_device (one frame on that table) and rs_incorporate_reconstruction_device (a second copy of the 50 000-landmark
        table on blocks of its own incorporated into that table through a map of 2 048 entries) — alternating, `repeat` calls
        each, HIP-event time on rs_stream(): median and best.  rs_gather_blocks_device on the keypoint pool [132][cap][28 bytes] next to a device-to-device hipMemcpyAsync of
        the same bytes on the same stream, and the gather with a NULL map (the identity: no map check, two stream operations
        instead of three), alternating: median, best and worst of each.  The host build's wall time for the table.  Outputs
        compared in bytes.
Prints one JSON line.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(stream, sync, torch, fn, before=None):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if before is not None:
        with torch.cuda.stream(stream):
            before()
    t0.record(stream)
    fn()
    t1.record(stream)
    sync()
    return t0.elapsed_time(t1)


def step(repeat):
    import torch
    import landmark_table_checker as LT
    import repack_catalogue as cat
    import test_gpu_triangulate as big
    from cv_amd import _lib, build
    from cv_amd.landmark_table import LandmarkUpdate
    from cv_amd.ransac import EssentialConsensus
    from cv_amd.reconstruction_merge import ReconstructionMerge
    from cv_amd.repack import TableRepack
    from cv_amd.triangulation import LandmarkTable
    build.build()
    cons = EssentialConsensus(8, 1)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.ExternalStream(cons.stream(), device=dev)
    up = lambda a: None if a is None else _lib.device_bytes(torch, a, dev)
    p = lambda t: None if t is None else t.data_ptr()
    kps, _, start, obs = big.big_map(np.random.default_rng(0x7121))
    nv, cap = kps.shape
    obs = obs.astype(np.uint32).copy()
    src_start, src_obs = start.astype(np.uint32).copy(), obs.copy()     # the source of the incorporate: the table as it came
    obs[1::2, 0] += nv                                                   # every second observation in a second view
    n_blocks, tail = 2 * nv, 64
    lens = np.diff(start.astype(np.int64))
    rows = []
    for r, n in enumerate(lens):                                         # one tombstone behind every nine rows
        rows.append(n)
        if r % 9 == 8:
            rows.append(0)
    rows += [0] * (tail * cap)
    start = np.concatenate([[0], np.cumsum(rows)]).astype(np.uint32)
    n_lm, n_obs = len(start) - 1, len(obs)
    block_map, n_out = cat.compact(n_blocks, {7})
    case = cat.Case("bench", [], n_blocks, block_map, n_out, start=start, cap=cap)
    case.obs, case.n_obs = obs, n_obs
    cat._lib()                                                           # the host build is compiled before anything is timed
    t0 = time.perf_counter()
    want = cat.host_table(case)
    t_host = time.perf_counter() - t0

    rp, upd = TableRepack(cons), LandmarkUpdate(cons)
    d_start, d_obs, d_map = up(start), up(obs), up(case.map)
    d = {k: up(v) for k, v in cat.blank(case).items()}

    def run_repack():
        rp.table_device(d_start, d_obs, n_obs, n_lm, cap, n_blocks, d_map, n_out, None, 0, case.obs_room, case.lm_room, d["obs_start_out"],
                        d["obs_out"], d["obs_counts_out"], d["landmarks_out"], d["key_out"], None, d["counts_out"], d["call_verdict"])

    # the yardstick: one frame added to the same table
    counts = np.zeros(n_blocks + 1, np.uint32)
    counts[n_blocks] = min(cap, 2048)
    feats = np.arange(int(counts[n_blocks]) * 3 // 4)
    slot = LT.slot(n_blocks, int(counts[n_blocks]), [(int(j), int(j) * 7 % 50000) for j in feats])
    av = LT.inputs(start, obs, n_obs, cap, n_blocks + 1, [slot], counts=counts)
    d_av = {k: up(av[k]) for k in ("counts", "matches", "nmatches", "final", "verdict", "pose_out")}
    av_fill = LT.outputs(av)
    d_avo = {k: up(av_fill[k]) for k in LT.OUTPUT_NAMES}

    def run_add():
        upd.add_views_device(p(d_start), p(d_obs), n_obs, n_lm, n_lm, None, None, 0, cap, n_blocks + 1, av["ik"], p(d_av["counts"]),
                             p(d_av["matches"]), p(d_av["nmatches"]), p(d_av["final"]), p(d_av["verdict"]), p(d_av["pose_out"]), None, None,
                             av["obs_room"], av["lm_room"], *(p(d_avo[k]) for k in LT.OUTPUT_NAMES))

    # the other yardstick: the untouched table, on blocks of its own behind the frame's, incorporated through 2 048 entries
    n_all = n_blocks + 1 + nv
    src_obs[:, 0] += n_blocks + 1
    n_src = len(src_start) - 1
    pairs = np.stack([np.arange(2048, dtype=np.uint32) * 24 + 1, np.arange(2048, dtype=np.uint32) * 500], 1)
    w32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).to(dev)
    dst_table = LandmarkTable.from_device(torch, w32(start), w32(obs), n_lm, n_obs)
    src_table = LandmarkTable.from_device(torch, w32(src_start), w32(src_obs), n_src, len(src_obs))
    eye = np.tile(np.hstack([np.eye(3), np.zeros((3, 1))]).reshape(12), (n_all, 1))
    d_poses0 = torch.from_numpy(eye).to(dev)
    d_ir_poses = d_poses0.clone()
    rm = ReconstructionMerge(cons)
    src_blocks = list(range(n_blocks + 1, n_all))
    ir = rm.incorporate_tensors(torch, dst_table, src_table, pairs, d_ir_poses, cap, src_blocks, n_blocks, eye[0])
    cons.sync()
    ir_verdict, ir_counts = int(ir.call_verdict.cpu()[0]), ir.counts_out.cpu().numpy().view(np.uint32).tolist()
    d_pairs, d_npairs, d_src_pose = w32(pairs), w32([len(pairs)]), torch.from_numpy(eye[0].copy()).to(dev)

    def run_inc():
        rm.incorporate_device(dst_table.d_start, dst_table.d_obs, n_obs, n_lm, src_table.d_start, src_table.d_obs, len(src_obs), n_src, d_pairs,
                              d_npairs, len(pairs), cap, n_all, src_blocks, n_blocks, d_src_pose, None, ir.obs_room, ir.lm_room, d_ir_poses,
                              ir.obs_start_out, ir.obs_out, ir.counts_out, ir.landmarks_out, ir.obs_counts_out, ir.src_key_out, ir.call_verdict)

    # the pools: the keypoints of every view
    pool = np.concatenate([kps, kps]).view(np.uint8).reshape(n_blocks, cap * 28)
    d_pool = up(pool).reshape(n_blocks, cap * 28)
    d_moved = torch.empty((n_out, cap * 28), dtype=torch.uint8, device=dev)
    d_copy = torch.empty((n_blocks, cap * 28), dtype=torch.uint8, device=dev)
    d_verdict = torch.zeros(1, dtype=torch.int32, device=dev)

    def run_gather():
        rp.gather_device(d_pool, d_moved, cap * 28, n_blocks, d_map, n_out, d_verdict)

    def run_copy():
        with torch.cuda.stream(stream):
            d_copy[:n_out].copy_(d_pool[:n_out])                         # the same bytes, device to device

    d_same = torch.empty((n_blocks, cap * 28), dtype=torch.uint8, device=dev)

    def run_gather_identity():
        rp.gather_device(d_pool, d_same, cap * 28, n_blocks, None, n_blocks, d_verdict)

    def run_copy_all():
        with torch.cuda.stream(stream):
            d_copy.copy_(d_pool)

    restore = lambda: d_ir_poses.copy_(d_poses0)                         # the incorporate re-poses the source's views in place
    calls = (("repack_table", run_repack, None), ("add_views", run_add, None), ("incorporate", run_inc, restore), ("gather_kps", run_gather, None),
             ("copy_kps", run_copy, None), ("gather_identity_kps", run_gather_identity, None), ("copy_all_kps", run_copy_all, None))
    torch.cuda.synchronize()
    for name, fn, before in calls * 3:                                   # warm-up: module load, scratch
        timed(stream, cons.sync, torch, fn, before)
    t = {name: [] for name, _, _ in calls}
    for _ in range(repeat):
        for name, fn, before in calls:
            t[name].append(timed(stream, cons.sync, torch, fn, before))
    got = {k: d[k].cpu().numpy().view(want[k].dtype).reshape(want[k].shape) for k in want}
    same = cat.same(got, want) is None and int(want["call_verdict"][0]) == cat.OK
    moved, verdict = cat.host_gather(pool, cap * 28, n_blocks, block_map, n_out)
    same = same and d_moved.cpu().numpy().tobytes() == moved.tobytes() and int(d_verdict.cpu()[0]) == cat.OK
    same = same and d_same.cpu().numpy().tobytes() == pool.tobytes() and ir_verdict == 0
    res = {"landmarks": n_lm, "observations": n_obs, "views": n_blocks, "cap": cap, "counts": want["counts_out"].tolist(),
           "rooms": [case.lm_room, case.obs_room], "pool_bytes": int(n_out) * cap * 28, "host_repack_table_ms": round(t_host * 1e3, 2), "incorporate_counts": ir_counts,
           "bit_equal": bool(same)}
    for name, v in t.items():
        res[name + "_ms_median"], res[name + "_ms_best"], res[name + "_ms_worst"] = round(float(np.median(v)), 4), round(min(v), 4), round(max(v), 4)
    print(json.dumps(res))
    cons.close()
    return 0 if same else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--step", action="store_true", help="run in this process (the default starts a child under `timeout`)")
    a = ap.parse_args()
    if a.step:
        return step(a.repeat)
    cmd = ["timeout", "-k", "10", "400", sys.executable, os.path.abspath(__file__), "--step", "--repeat", str(a.repeat)]
    print("#", " ".join(cmd), flush=True)
    return subprocess.run(cmd).returncode


if __name__ == "__main__":
    sys.exit(main())
