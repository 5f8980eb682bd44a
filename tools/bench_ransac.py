#!/usr/bin/env python3
"""BASELINE.json configs[3]: 10k eight-point hypotheses scored on 1000 matches (30 % outliers), threshold 1e-7,
on one MI355X, beside the CPU oracle on a bounded sample of the hypotheses.  Prints one JSON line.

--estimator five_point: the same exhaustive call through rs_five_point_batch (n_hyp / 10 five-match samples: the same number
of pose slots; no CPU oracle beside it — the host build of include/akz_five_point_math.h is the tests' business).
--scenes S: instead, the batched device entry (rs_essential_arrsac_batch_device) over S frame pairs of 400 matches, 30 %
outliers, --samples minimal samples per scene, the default retirement rules; median of --reps runs after --warmup."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from cv_amd import build  # noqa: E402
build.build()
from cv_amd.ransac import EssentialConsensus  # noqa: E402
from oracle import oracle as O  # noqa: E402
from test_gpu_parity import _two_view_scene  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--estimator", choices=("eight_point", "five_point"), default="eight_point")
ap.add_argument("--scenes", type=int, default=0, help="> 0: the batched device entry over this many frame pairs")
ap.add_argument("--samples", type=int, default=1024, help="minimal samples per scene of the batched run")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
args = ap.parse_args()
five = args.estimator == "five_point"


def batched():
    import torch
    from test_gpu_parity import _pixel_scene
    rng = np.random.default_rng(0x5AC)
    cap, n, S, thr = 512, 400, args.scenes, 2e-7
    cam = (984.2439, 980.8141, 690.0, 233.1966, 0.0, None)
    scenes = [_pixel_scene(rng, cap, cap, n, 0.3, cam) for _ in range(S)]
    pairs = np.zeros((S, cap, 2), np.uint32)
    for s in range(S):
        pairs[s, :n] = scenes[s][2]
    dev = torch.device("cuda", 0)
    d_ka = torch.from_numpy(np.stack([sc[0] for sc in scenes]).view(np.uint8).reshape(S, cap, 28)).to(dev)
    d_kb = torch.from_numpy(np.stack([sc[1] for sc in scenes]).view(np.uint8).reshape(S, cap, 28)).to(dev)
    d_pairs = torch.from_numpy(pairs.view(np.int32)).to(dev)
    d_np = torch.from_numpy(np.full(S, n, np.uint32).view(np.int32)).to(dev)
    d_pose = torch.zeros((S, 12), dtype=torch.float64, device=dev)
    d_best = torch.zeros((S,), dtype=torch.int32, device=dev)
    d_inl = torch.zeros((S, cap), dtype=torch.int32, device=dev)
    d_ninl = torch.zeros((S,), dtype=torch.int32, device=dev)
    d_stats = torch.zeros((S, 32), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    slots = args.samples * (10 if five else 1)
    cons = EssentialConsensus(cap, slots)
    cons.reserve(S)
    prm = cons.make_params(thr, n_hypotheses=args.samples, seed=7, estimator=args.estimator)
    c = cons.camera(cam)
    times = []
    for i in range(args.warmup + args.reps):
        t0 = time.perf_counter()
        cons.model_inliers_batch_device(d_ka.data_ptr(), d_kb.data_ptr(), cap, list(range(S)), list(range(S)), d_pairs.data_ptr(),
                                        d_np.data_ptr(), c, c, prm, d_pose.data_ptr(), d_best.data_ptr(), d_inl.data_ptr(),
                                        d_ninl.data_ptr(), d_stats.data_ptr(), shuffle=True)
        cons.sync()
        if i >= args.warmup:
            times.append(time.perf_counter() - t0)
    st = d_stats.cpu().numpy().view(np.dtype([("poses", "<u4"), ("survivors", "<u4"), ("blocks", "<u4"), ("reserved", "<u4"),
                                               ("evaluated", "<u8"), ("exhaustive", "<u8")])).reshape(S)
    ninl = d_ninl.cpu().numpy().view(np.uint32)
    best = d_best.cpu().numpy().view(np.uint32)
    t = np.array(times)
    print(json.dumps({
        "workload": f"{S} scenes x {args.samples} {args.estimator} samples ({slots} hypothesis slots, {4 * slots} pose slots) x {n} matches "
                    "(30% outliers), thr 2e-7, device-resident, default retirement rules",
        "estimator": args.estimator, "scenes": S, "samples": args.samples, "pose_slots": 4 * slots,
        "ms_median": round(float(np.median(t)) * 1e3, 3), "ms_min": round(float(t.min()) * 1e3, 3),
        "ms_max": round(float(t.max()) * 1e3, 3), "runs": len(times), "warmup": args.warmup,
        "models": int((best != 0xFFFFFFFF).sum()), "inliers_mean": round(float(ninl.mean()), 1),
        "residuals_evaluated": int(st["evaluated"].sum()), "residuals_exhaustive": int(st["exhaustive"].sum())}))


if args.scenes > 0:
    batched()
    sys.exit(0)

rng = np.random.default_rng(0x5AC)
n, n_hyp, thr = 1000, 10000, 1e-7
a, b = _two_view_scene(rng, n, 0.3)
if five:
    samples = np.stack([rng.choice(n, 5, replace=False) for _ in range(n_hyp // 10)]).astype(np.uint32)
    cons = EssentialConsensus(n, n_hyp)
    cons.five_point_model_inliers(a, b, samples, thr)  # warm-up
    times = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        pose, inl, best = cons.five_point_model_inliers(a, b, samples, thr)
        times.append(time.perf_counter() - t0)
    E, nsol = cons.essentials(len(samples))
    gpu_s = float(np.median(times))
    print(json.dumps({
        "workload": f"{len(samples)} five-point samples ({n_hyp} hypothesis slots) x 4 poses x 1000 matches (30% outliers), thr 1e-7, "
                    "host buffers in/out",
        "estimator": "five_point", "gpu_seconds_per_scene": round(gpu_s, 5), "samples_per_s": round(len(samples) / gpu_s, 1),
        "solutions": int(nsol.sum()), "inliers": int(len(inl)), "runs": args.reps}))
    sys.exit(0)
samples = np.stack([rng.choice(n, 8, replace=False) for _ in range(n_hyp)]).astype(np.uint32)
cons = EssentialConsensus(n, n_hyp)
cons.model_inliers(a, b, samples, thr)  # warm-up
t0 = time.perf_counter()
reps = 5
for _ in range(reps):
    pose, inl, best = cons.model_inliers(a, b, samples, thr)
gpu_s = (time.perf_counter() - t0) / reps
sub = 100
t0 = time.perf_counter()
w = O.essential_batch(a, b, samples[:sub], thr)
cpu_s = time.perf_counter() - t0
g2 = cons.model_inliers(a, b, samples[:sub], thr)
assert g2[2] == w[1] and np.array_equal(g2[1], w[2]) and g2[0].tobytes() == w[0].tobytes()
print(json.dumps({
    "workload": "10k eight-point hypotheses x 4 poses x 1000 matches (30% outliers), thr 1e-7, host buffers in/out",
    "gpu_seconds_per_scene": round(gpu_s, 5), "hypotheses_per_s": round(n_hyp / gpu_s, 1),
    "pose_match_residuals_per_s": round(n_hyp * 4 * n / gpu_s, 1), "inliers": int(len(inl)),
    "cpu_oracle": {"hypotheses_per_s": round(sub / cpu_s, 2), "cores": 1, "sample": f"first {sub} hypotheses, {cpu_s:.1f} s"},
    "parity": "best id, pose bits and inlier set identical to the oracle on the sampled hypotheses"}))
