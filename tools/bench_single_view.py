#!/usr/bin/env python3
"""Times of the single-view refinement (cv_amd/csrc/rs_single_view.hip) at the reference's default settings, behind the
consensus, against the host build of the same header on one core.  It has no part in bench.py.

  python tools/bench_single_view.py [--scenes 1 64 256] [--matches 2048] [--patience 100000] [--host-patience 2000]
        one child process under `timeout`.  For every S of --scenes: S new frames of --matches original matches each (every
        twentieth 20 - 40 px off, 0.3 px noise) against one map of a dozen views; rs_p3p_arrsac_batch_device (the
        registration consensus, vslam-sandbox's settings) and rs_refine_poses_batch_device behind it on rs_stream(), the
        refinement between two HIP events: milliseconds, the optimiser iterations it made (from its stats words) and the
        microseconds per iteration.  The parent commit has no device path: the baseline is the host build of
        include/akz_single_view_math.h on scene 0 with the device consensus' outputs, at --host-patience iterations a run (a
        default run takes the host minutes), in microseconds per iteration; at equal patience the outputs are compared in bytes.
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


def iterations_of(stats, V):
    """optimiser iterations a scene made: a run left at `iteration` k has summed k + 1 times"""
    stops = stats[V.S_RUN_STOP:V.S_RUN_STOP + 9].astype(np.int64)
    matches = stats[V.S_RUN_MATCHES:V.S_RUN_MATCHES + 9].astype(np.int64)
    return int(sum(k + 1 for k, m in zip(stops, matches) if k != 0xFFFFFFFF and m > 0))


def step(scenes, matches, patience, host_patience):
    import torch
    import single_view_checker as V
    from cv_amd import _lib, build
    from cv_amd.ransac import EssentialConsensus
    from cv_amd.single_view import SingleViewRefiner
    build.build()
    dev = torch.device("cuda", 0)
    up = lambda a: _lib.device_bytes(torch, a, dev)
    rig = V.Rig(0x5EED, matches, noise=0.3, perturb=0.0, outliers=range(7, matches, 20))
    one = V.Batch([rig], matches)
    blocks = (matches + 63) // 64
    cons = EssentialConsensus(matches, 16384 + 256 * blocks)
    cons.reserve(max(scenes))
    stream = torch.cuda.ExternalStream(cons.stream(), device=dev)
    cam = V.rig_camera_dev()
    arr = cons.make_params(1e-5, n_hypotheses=16384, seed=7, block_size=64, init_blocks=1, max_candidates=1024, halve=True, sprt=True,
                           estimations_per_block=256)
    refiner = SingleViewRefiner(cons)
    res, ok = {"matches": matches, "patience": patience, "host_patience": host_patience, "sizes": {}}, True
    for S in scenes:
        # the map once, the new frame S times
        kps = np.concatenate([one.kps[:rig.n_views]] + [one.kps[rig.n_views:]] * S)
        poses = np.concatenate([one.poses[:rig.n_views], np.zeros((S, 12))])
        ik = [rig.n_views + s for s in range(S)]
        d_kps, d_poses, d_start, d_obs, d_world = up(kps.view(np.uint8)), up(poses), up(one.obs_start), up(one.obs), up(one.world)
        d_matches, d_nm = up(np.tile(one.matches, (S, 1, 1))), up(np.tile(one.nmatches, S))
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        d_pose, d_id, d_inl, d_ninl = z((S, 12), torch.float64), z((S,), torch.int32), z((S, matches), torch.int32), z((S,), torch.int32)
        out = dict(pose=z((S, 12), torch.float64), verdict=z((S,), torch.int32), final=z((S, matches), torch.uint8), n_final=z((S,), torch.int32),
                   stats=z((S, V.STATS), torch.int32))
        torch.cuda.synchronize()

        def run(prm, timed):
            cons.p3p_model_inliers_batch_device(d_kps.data_ptr(), matches, ik, d_matches.data_ptr(), d_nm.data_ptr(), d_world.data_ptr(),
                                                one.n_world, cam, arr, d_pose.data_ptr(), d_id.data_ptr(), d_inl.data_ptr(), d_ninl.data_ptr())
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(stream)
            refiner.refine_batch_device(d_kps.data_ptr(), matches, len(kps), d_poses.data_ptr(), cam, d_start.data_ptr(), d_obs.data_ptr(),
                                        one.n_obs, one.n_landmarks, d_world.data_ptr(), one.n_world, ik, d_matches.data_ptr(), d_nm.data_ptr(),
                                        None, d_pose.data_ptr(), d_id.data_ptr(), d_inl.data_ptr(), d_ninl.data_ptr(), prm, out["pose"].data_ptr(),
                                        out["verdict"].data_ptr(), out["final"].data_ptr(), out["n_final"].data_ptr(), out["stats"].data_ptr())
            t1.record(stream)
            cons.sync()
            return t0.elapsed_time(t1) if timed else None

        run(SingleViewRefiner.params(single_view_patience=host_patience), False)          # warm-up, and the run the host repeats
        got = {k: v.cpu().numpy() for k, v in out.items()}
        host_entry = None
        if S == scenes[0]:
            hb = V.Batch([rig], matches)
            hb.pose, hb.best_id = d_pose.cpu().numpy()[:1].copy(), d_id.cpu().numpy().view(np.uint32)[:1].copy()
            hb.inliers, hb.n_inliers = d_inl.cpu().numpy().view(np.uint32)[:1].copy(), d_ninl.cpu().numpy().view(np.uint32)[:1].copy()
            t0 = time.perf_counter()
            want = hb.host(V.settings(single_view_patience=host_patience), np.zeros((1, 12)), np.zeros((1, matches), np.uint8))
            host_s = time.perf_counter() - t0
            its = iterations_of(want["stats"][0], V)
            same = (got["pose"][0].tobytes() == want["pose_out"][0].tobytes() and np.array_equal(got["final"][0], want["final"][0]) and
                    np.array_equal(got["stats"][0].view(np.uint32), want["stats"][0]) and int(got["verdict"][0]) == int(want["verdict"][0]))
            ok = ok and same
            host_entry = {"host_ms": round(host_s * 1e3, 1), "host_iterations": its, "host_us_per_iteration": round(host_s * 1e6 / max(its, 1), 3),
                          "verdict": int(want["verdict"][0]), "bit_equal": bool(same)}
        ms = run(SingleViewRefiner.params(single_view_patience=patience), True)
        stats = out["stats"].cpu().numpy().view(np.uint32)
        verdict = out["verdict"].cpu().numpy()
        its = [iterations_of(stats[s], V) for s in range(S)]
        entry = {"refine_ms": round(ms, 3), "iterations_per_scene_max": max(its), "us_per_iteration": round(ms * 1e3 / max(max(its), 1), 4),
                 "scene_iterations_per_second": round(sum(its) / (ms * 1e-3), 1), "verdicts_ok": int((verdict == 0).sum()),
                 "inliers_taken": int(stats[0, V.S_INLIERS]), "run_stops_first": stats[0, V.S_RUN_STOP:V.S_RUN_STOP + 6].tolist()}
        if host_entry:
            entry["host"] = host_entry
        res["sizes"][str(S)] = entry
    print(json.dumps(res))
    cons.close()
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, nargs="+", default=[1, 64, 256])
    ap.add_argument("--matches", type=int, default=2048)
    ap.add_argument("--patience", type=int, default=100000)
    ap.add_argument("--host-patience", type=int, default=2000)
    ap.add_argument("--step", action="store_true", help="run in this process (the default starts a child under `timeout`)")
    a = ap.parse_args()
    if a.step:
        return step(a.scenes, a.matches, a.patience, a.host_patience)
    cmd = ["timeout", "-k", "10", "500", sys.executable, os.path.abspath(__file__), "--step", "--matches", str(a.matches), "--patience",
           str(a.patience), "--host-patience", str(a.host_patience), "--scenes"] + [str(s) for s in a.scenes]
    print("#", " ".join(cmd), flush=True)
    return subprocess.run(cmd).returncode


if __name__ == "__main__":
    sys.exit(main())
