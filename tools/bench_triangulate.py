#!/usr/bin/env python3
"""Times of the triangulation kernels (cv_amd/csrc/rs_triangulate.hip) and their effect on the registration leg.

  python tools/bench_triangulate.py --profile table    kernel times of a 100 000-landmark table under rocprofv3
  python tools/bench_triangulate.py --profile pairs    the same for 256 scenes of two-view inliers
        (starts `rocprofv3 --kernel-trace --stats -- python tools/bench_triangulate.py --run <what>` as a fresh child process
        and prints the k_tri_* rows of its kernel statistics beside what the run printed: list-length histogram, bytes, flops)
  python tools/bench_triangulate.py --run table|pairs  the workload alone, timed with HIP events
  python tools/bench_triangulate.py --register [--refresh] [--steps K]
        the pipeline+register leg of bench.py (tools/bench_extras.py, unchanged) — with --refresh the whole 100 000-landmark
        table is triangulated again on rs_stream() in every 256-frame step, in front of the consensus.  Prints one JSON line.
"""
import argparse
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CAM = (1000.0, 1000.0, 960.0, 540.0, 0.0, None)
# what one observation costs in f64 operations (include/akz_triangulate_math.h): calibrate 14, accumulate 12 * 6 + 10 * 6,
# the (0, j) robustness pair 15 + 7, cheirality 15 + 5; the eigen-solve: ~6 sweeps x 6 rotations x ~60 + selection ~40
FLOPS_PER_OBS, FLOPS_PER_SOLVE = 14 + 132 + 22 + 14 + 20, 6 * 6 * 60 + 40
# MI355X: 78.6 TFLOP/s of vector FP64 counts an FMA as two; the kernels are unfused (-ffp-contract=off), one operation per
# issue slot: 256 CUs x 64 lanes x 2.4 GHz = 39.3e12 f64 instructions-lanes / s.  HBM: 8 TB/s.
F64_PEAK, HBM_PEAK = 39.3e12, 8.0e12


def rodrigues(v):
    th = np.linalg.norm(v, axis=-1, keepdims=True)
    k = v / np.where(th == 0, 1, th)
    K = np.zeros(v.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 0] = -k[..., 2], k[..., 1], k[..., 2]
    K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -k[..., 0], -k[..., 1], k[..., 0]
    s, c = np.sin(th)[..., None], np.cos(th)[..., None]
    return np.eye(3) + s * K + (1 - c) * (K @ K)


def make_table(n_landmarks=100000, n_blocks=256, cap=8192, seed=0x7AB):
    """A map of n_landmarks points seen from n_blocks cameras: list lengths 0..32 (a third of the landmarks 2-4 observations,
    the rest uniform — young landmarks dominate a real map), observation = projection + 0.5 px noise."""
    rng = np.random.default_rng(seed)
    centres = rng.uniform([-1, -1, -0.3], [1, 1, 0.3], (n_blocks, 3))
    R = rodrigues(rng.normal(0, 0.05, (n_blocks, 3)))
    poses = np.concatenate([R, -(R @ centres[..., None])], 2)
    pts = np.stack([rng.uniform(-2, 2, n_landmarks), rng.uniform(-1.5, 1.5, n_landmarks), rng.uniform(2, 10, n_landmarks)], 1)
    lens = np.where(rng.random(n_landmarks) < 1 / 3, rng.integers(2, 5, n_landmarks), rng.integers(0, 33, n_landmarks))
    start = np.concatenate([[0], np.cumsum(lens)])
    total = int(start[-1])
    lm = np.repeat(np.arange(n_landmarks), lens)
    blk = rng.integers(0, n_blocks, total)
    order = np.argsort(blk, kind="stable")
    feat = np.empty(total, np.int64)
    feat[order] = np.arange(total) - np.searchsorted(blk[order], blk[order])          # slot = rank inside the block
    assert feat.max() < cap
    q = np.einsum("nij,nj->ni", poses[blk][:, :, :3], pts[lm]) + poses[blk][:, :, 3]
    from cv_amd._lib import KP_DTYPE
    kps = np.zeros((n_blocks, cap), KP_DTYPE)
    kps["x"][blk, feat] = CAM[0] * q[:, 0] / q[:, 2] + CAM[2] + rng.uniform(-0.5, 0.5, total)
    kps["y"][blk, feat] = CAM[1] * q[:, 1] / q[:, 2] + CAM[3] + rng.uniform(-0.5, 0.5, total)
    obs = np.stack([blk, feat], 1).astype(np.uint32)
    return kps, poses.reshape(n_blocks, 12), start, obs, lens


def device_table(torch, dev, n_landmarks=100000):
    from cv_amd.triangulation import LandmarkTable
    kps, poses, start, obs, lens = make_table(n_landmarks)
    d_kps = torch.from_numpy(kps.view(np.uint8).reshape(kps.shape + (28,))).to(dev)
    d_poses = torch.from_numpy(poses).to(dev)
    table = LandmarkTable(torch, start=start, obs=obs, device=dev.index or 0)
    return table, d_kps, d_poses, lens


def run_table(torch, dev, reps):
    from cv_amd import triangulation
    from cv_amd.ransac import EssentialConsensus
    table, d_kps, d_poses, lens = device_table(torch, dev)
    cons = EssentialConsensus(8, 1)
    cam, prm = cons.camera(CAM), triangulation.make_params()
    d_world = table.new_world()
    d_reason = torch.zeros((table.n_landmarks,), dtype=torch.uint8, device=dev)
    s = torch.cuda.ExternalStream(cons.stream(), device=dev)
    go = lambda: triangulation.triangulate_landmarks_device(cons._h, table, d_kps, d_kps.shape[1], d_kps.shape[0], d_poses, cam, prm,
                                                           d_world, d_reason)
    go(); cons.sync()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(reps):
        go()
    e1.record(s); cons.sync()
    us = e0.elapsed_time(e1) * 1e3 / reps
    reasons = np.bincount(d_reason.cpu().numpy(), minlength=7)
    hist = np.bincount(np.minimum(lens, 32) // 4, minlength=9)
    n_obs, solved = int(lens.sum()), int(reasons[0] + reasons[5])
    flops = n_obs * FLOPS_PER_OBS + solved * FLOPS_PER_SOLVE
    # every observation is gathered twice (accumulation, cheirality): 8 B of index + a 64 B line of the 28 B keypoint + the
    # 96 B pose (poses of 256 blocks stay in cache: not counted); 32 B + 1 B written per landmark
    byts = n_obs * 2 * (8 + 64) + table.n_landmarks * (8 + 33)
    out = {"what": "k_tri_landmarks", "landmarks": table.n_landmarks, "observations": n_obs, "reps": reps, "us_per_launch_hip_events": round(us, 1),
           "list_length_histogram_0-3_4-7_.._28-31_32": hist.tolist(), "reasons_0..6": reasons.tolist(),
           "f64_operations": flops, "f64_issue_fraction": round(flops / (us * 1e-6) / F64_PEAK, 4),
           "gathered_bytes": byts, "hbm_fraction": round(byts / (us * 1e-6) / HBM_PEAK, 4)}
    cons.close()
    return out


def run_pairs(torch, dev, reps, S=256, cap=2048):
    """256 scenes, ~1 000-2 000 inliers each, behind a consensus whose outputs are given (known pose, every pair an inlier)."""
    from cv_amd import triangulation
    from cv_amd._lib import KP_DTYPE
    from cv_amd.ransac import EssentialConsensus
    rng = np.random.default_rng(0x9A1)
    n = rng.integers(1000, cap + 1, S)
    R = rodrigues(rng.normal(0, 0.1, (S, 3)))
    t = rng.uniform(-0.3, 0.3, (S, 3))
    pts = np.stack([rng.uniform(-2, 2, (S, cap)), rng.uniform(-1.2, 1.2, (S, cap)), rng.uniform(3, 9, (S, cap))], 2)
    q = np.einsum("sij,snj->sni", R, pts) + t[:, None, :]
    ka, kb = np.zeros((S, cap), KP_DTYPE), np.zeros((S, cap), KP_DTYPE)
    for k, p in ((ka, pts), (kb, q)):
        k["x"] = CAM[0] * p[..., 0] / p[..., 2] + CAM[2] + rng.uniform(-0.3, 0.3, (S, cap))
        k["y"] = CAM[1] * p[..., 1] / p[..., 2] + CAM[3] + rng.uniform(-0.3, 0.3, (S, cap))
    idx = np.broadcast_to(np.arange(cap, dtype=np.uint32), (S, cap))
    pairs = np.stack([idx, idx], 2).copy()
    to = lambda a, v=None: torch.from_numpy(np.ascontiguousarray(a if v is None else a.view(v))).to(dev)
    d_ka, d_kb = to(ka.view(np.uint8).reshape(S, cap, 28)), to(kb.view(np.uint8).reshape(S, cap, 28))
    d_pairs, d_np = to(pairs, np.int32), to(n.astype(np.uint32), np.int32)
    d_pose = to(np.concatenate([R, t[..., None]], 2).reshape(S, 12))
    d_best, d_inl, d_ninl = to(np.zeros(S, np.int32)), to(idx.copy(), np.int32), to(n.astype(np.uint32), np.int32)
    d_pts = torch.zeros((S, cap, 4), dtype=torch.float64, device=dev)
    d_why = torch.zeros((S, cap), dtype=torch.uint8, device=dev)
    cons = EssentialConsensus(cap, 8)
    cons.reserve(S)
    cam, prm = cons.camera(CAM), triangulation.make_params()
    ia = list(range(S))
    go = lambda: cons.triangulate_inliers(d_ka.data_ptr(), d_kb.data_ptr(), cap, ia, ia, d_pairs.data_ptr(), d_np.data_ptr(), cam, cam,
                                          d_pose.data_ptr(), d_best.data_ptr(), d_inl.data_ptr(), d_ninl.data_ptr(), d_pts.data_ptr(),
                                          d_why.data_ptr(), params=prm)
    go(); cons.sync()
    s = torch.cuda.ExternalStream(cons.stream(), device=dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(reps):
        go()
    e1.record(s); cons.sync()
    us = e0.elapsed_time(e1) * 1e3 / reps
    total = int(n.sum())
    reasons = np.bincount(np.concatenate([d_why.cpu().numpy()[i, :n[i]] for i in range(S)]), minlength=7)
    flops = total * (2 * FLOPS_PER_OBS + FLOPS_PER_SOLVE)
    byts = total * (4 + 8 + 2 * 64 + 33)
    out = {"what": "k_tri_pairs", "scenes": S, "inliers": total, "reps": reps, "us_per_launch_hip_events": round(us, 1),
           "reasons_0..6": reasons.tolist(), "f64_operations": flops, "f64_issue_fraction": round(flops / (us * 1e-6) / F64_PEAK, 4),
           "gathered_bytes": byts, "hbm_fraction": round(byts / (us * 1e-6) / HBM_PEAK, 4)}
    cons.close()
    return out


def profile(what, reps):
    """The run as a fresh child under rocprofv3 --kernel-trace --stats (the program after `--`); the k_tri_* rows of the
    kernel statistics and the run's own line."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
               "--run", what, "--reps", str(reps)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        print(f"# python tools/bench_triangulate.py --profile {what}   (= rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- "
              f"python tools/bench_triangulate.py --run {what} --reps {reps})")
        if r.returncode != 0 or not lines:
            print(r.stdout[-2000:] + r.stderr[-2000:])
            return 1
        stats = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not stats:
            print("no kernel statistics file under", d, os.listdir(d))
            return 1
        with open(stats[0]) as f:
            rows = f.read().splitlines()
        mine = [row for row in rows[1:] if "k_tri_" in row]
        if not mine:
            print("no k_tri_* row in the kernel statistics")
            return 1
        # the fractions against the kernel's own average duration in the trace (the HIP-event time of the run includes the
        # gaps between launches): columns after the quoted name are Calls, TotalDurationNs, AverageNs, ...
        avg_ns = float(mine[0].rsplit('",', 1)[1].split(",")[2])
        out = json.loads(lines[-1])
        out["f64_issue_fraction"] = round(out["f64_operations"] / (avg_ns * 1e-9) / F64_PEAK, 4)
        out["hbm_fraction"] = round(out["gathered_bytes"] / (avg_ns * 1e-9) / HBM_PEAK, 4)
        out["fractions_are_of"] = ("the kernel's average duration in the trace below; peaks %.3g unfused f64 operations / s, %.3g B / s; "
                                   "f64_operations and gathered_bytes are estimates from the source (FLOPS_PER_OBS, FLOPS_PER_SOLVE, "
                                   "one 64 B line per gathered keypoint), not counters" % (F64_PEAK, HBM_PEAK))
        print(f"MI355X, the kernel alone on the GPU: {what}")
        print(json.dumps(out))
        print(rows[0])
        for row in mine:
            print(row)
    return 0


def register_leg(torch, dev, steps, refresh):
    """bench.py's pipeline+register leg (tools/bench_extras.extra_pipeline_register, as it is); with `refresh` every
    Registration.enqueue() — one per 256-frame step — first triangulates the whole 100 000-landmark table on rs_stream()."""
    import types
    from cv_amd import _lib
    from cv_amd.akaze import Akaze
    from cv_amd.registration import Registration
    from tools import bench_extras
    from tools.bench_common import CAP, FRAMES_PER_STEP, H, W, make_frames
    L = _lib.lib()
    NF = MB = FRAMES_PER_STEP
    frames = make_frames(torch, dev, 0, NF, 1)
    ak = Akaze.default()
    ak.max_keypoints = CAP
    ctx = ak.context(W, H, MB)
    args = types.SimpleNamespace(register_views=32, register_steps=steps, register_check=2)
    launches = [0]
    if refresh:
        table, d_kps, d_poses, _ = device_table(torch, dev)
        d_table_world = table.new_world()
        plain = Registration.enqueue

        def enqueue(self, *a, **kw):
            # the refresh reads its own (static) map and writes its own table: the leg's results stay what they were
            from cv_amd import triangulation
            triangulation.triangulate_landmarks_device(self.cons._h, table, d_kps, d_kps.shape[1], d_kps.shape[0], d_poses,
                                                       self.cons.camera(CAM), self.tri_prm, d_table_world)
            launches[0] += 1
            return plain(self, *a, **kw)
        Registration.enqueue = enqueue
    out = bench_extras.extra_pipeline_register(torch, dev, L, _lib, args, ctx, frames, NF, MB)
    return {"leg": "pipeline+register", "refresh_100k_table_per_step": bool(refresh), "refresh_launches": launches[0],
            "registered_frames_per_s": out["registered_frames_per_s"], "ms_per_step": out["ms_per_step"], "steps": steps,
            "frames_with_a_model": out["frames_with_a_model"], "parity_mismatches": out["parity"]["mismatches"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--profile", choices=["table", "pairs"])
    ap.add_argument("--run", choices=["table", "pairs"])
    ap.add_argument("--register", action="store_true")
    ap.add_argument("--refresh", action="store_true")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    if a.profile:
        return profile(a.profile, a.reps)
    import torch
    from cv_amd import build
    build.build()
    dev = torch.device("cuda", 0)
    if a.run:
        print(json.dumps((run_table if a.run == "table" else run_pairs)(torch, dev, a.reps)))
    elif a.register:
        print(json.dumps(register_leg(torch, dev, a.steps, a.refresh)))
    else:
        ap.error("one of --profile, --run, --register")
    return 0


if __name__ == "__main__":
    sys.exit(main())
