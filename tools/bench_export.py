#!/usr/bin/env python3
"""Times of the export of a reconstruction (cv_amd/csrc/rs_export.hip) against the host build of the same header on one core.
It has no part in bench.py.

  python tools/bench_export.py [--repeat 20]
        one child process under `timeout`.  The 50 000-landmark table of tests/test_gpu_triangulate.py's big_map (805 902
        observations, lists of 0 to 48 — the one tools/bench_observation_filter.py times the filter on), its world table from
        rs_triangulate_landmarks_device, and 132 views: big_map's 66 and a second copy of them in blocks of their own.
        rs_export_reconstruction_device with all the views (`export`), the same call with one view (`points`: the four
        launches of the point cloud and one camera's workgroup), and in the same run rs_triangulate_landmarks_device — the
        yardstick — alternating, `repeat` calls each after a warm-up, HIP-event time on rs_stream(): median and best.  The
        cameras' launch is not timed alone: `cameras_ms_derived` is the difference of the two medians.  The host build's wall
        time for the same call.  Outputs compared in bytes.
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


def timed(stream, sync, torch, fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(stream)
    fn()
    t1.record(stream)
    sync()
    return t0.elapsed_time(t1)


def step(repeat):
    import torch
    import export_checker as K
    import test_gpu_triangulate as big
    import triangulate_checker as tc
    from cv_amd import _lib, build, triangulation
    from cv_amd.export import ReconstructionExport
    from cv_amd.ransac import EssentialConsensus
    build.build()
    cons = EssentialConsensus(8, 1)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.ExternalStream(cons.stream(), device=dev)
    up = lambda a: _lib.device_bytes(torch, a, dev)
    kps, poses, start, obs = big.big_map(np.random.default_rng(0x7121))
    nl, (nv, cap) = len(start) - 1, kps.shape
    n_obs, n_blocks = len(obs), 2 * nv
    cam = tc.camera(*big.CAM[:5])
    rcam = _lib.Camera(cam.fx, cam.fy, cam.cx, cam.cy, cam.skew, cam.k1, cam.use_k1, 0)
    obs = obs.astype(np.uint32).reshape(-1, 2)
    lm = np.full((n_blocks, cap), K.NONE, np.uint32)
    rows = np.repeat(np.arange(nl), np.diff(start.astype(np.int64)))
    lm[obs[::-1, 0], obs[::-1, 1]] = rows[::-1]                           # the lowest key where a feature is listed twice
    lm[nv:] = lm[:nv]
    counts = np.zeros(n_blocks, np.uint32)
    counts[:nv] = [int(obs[obs[:, 0] == b, 1].astype(np.int64).max(initial=-1)) + 1 for b in range(nv)]
    counts[nv:] = counts[:nv]
    all_poses = np.concatenate([poses, poses]).reshape(n_blocks, 12).copy()
    table = triangulation.LandmarkTable(torch, start=start, obs=obs)
    d_kps, d_poses = up(kps.view(np.uint8)), torch.from_numpy(all_poses).to(dev)
    d_world, d_reason = table.new_world(), torch.zeros((nl,), dtype=torch.uint8, device=dev)
    tprm = triangulation.make_params(n_views=nv)

    def run_tri():
        triangulation.triangulate_landmarks_device(cons._h, table, d_kps, cap, nv, d_poses, rcam, tprm, d_world, d_reason)

    torch.cuda.synchronize()
    timed(stream, cons.sync, torch, run_tri)
    inp = K.inputs(d_world.cpu().numpy(), None, np.arange(n_blocks), counts, lm, all_poses, cap, start=start.astype(np.uint32), start_obs=obs)
    K.lib()                                                                # the host build is compiled before anything is timed
    t0 = time.perf_counter()
    want = K.export(inp)
    t_host = time.perf_counter() - t0
    d_in = {k: up(inp[k]) for k in ("colors", "counts", "landmarks")}
    fill = K.outputs(inp)
    d = {k: up(fill[k]) for k in K.OUTPUTS}
    d_one = {k: up(fill[k]) for k in K.OUTPUTS}
    ex = ReconstructionExport(cons)

    def run_export(views=list(range(n_blocks)), out=d):
        ex.export_device(d_world, nl, table.d_start, table.d_obs, n_obs, nl, d_in["colors"], views, d_in["counts"], d_in["landmarks"], cap, n_blocks,
                         d_poses, inp["room"], *(out[k] for k in K.OUTPUTS))

    calls = (("export", run_export), ("points", lambda: run_export([0], d_one)), ("triangulate", run_tri))
    for name, fn in calls * 2:                                              # warm-up: module load, scratch
        timed(stream, cons.sync, torch, fn)
    t = {name: [] for name, _ in calls}
    for _ in range(repeat):
        for name, fn in calls:
            t[name].append(timed(stream, cons.sync, torch, fn))
    got = {k: d[k].cpu().numpy().view(want[k].dtype).reshape(want[k].shape) for k in K.OUTPUTS}
    same = all(got[k].tobytes() == want[k].tobytes() for k in K.OUTPUTS)
    res = {"landmarks": nl, "observations": n_obs, "views": n_blocks, "cap": cap, "counts": want["counts_out"].tolist(),
           "verdict": int(want["verdict"][0]), "host_export_ms": round(t_host * 1e3, 2), "bit_equal": bool(same)}
    for name, v in t.items():
        res[name + "_ms_median"], res[name + "_ms_best"] = round(float(np.median(v)), 4), round(min(v), 4)
    res["cameras_ms_derived"] = round(res["export_ms_median"] - res["points_ms_median"], 4)
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
