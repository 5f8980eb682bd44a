#!/usr/bin/env python3
"""Times of the landmark bookkeeping (cv_amd/csrc/rs_landmark_table.hip) against the host build of the same header on one core.
It has no part in bench.py.

  python tools/bench_landmark_table.py [--frames 1 8 64] [--matches 2048] [--repeat 20]
        one child process under `timeout`.  The table is the 50 000-landmark table of tests/test_gpu_triangulate.py's big_map
        (66 views, lists of 0 to 48 — the one tools/bench_observation_filter.py times the filter on).  For every F of --frames: a
        micro-batch of F accepted frames in the blocks behind the table's, --matches final matches each to landmarks drawn at
        random (so frames of one call name the same landmarks now and then), one in 32 of them a merge, and as many merge
        candidates again for the mask alone.  rs_landmarks_sharing_view_device and rs_add_views_device, and in the same run
        rs_filter_observations_device and rs_triangulate_landmarks_device on that table — the yardsticks — alternating, `repeat`
        calls each, HIP-event time on rs_stream(): median and best.  The host build's wall time for the same two calls.  Outputs
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


def timed(stream, sync, torch, fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(stream)
    fn()
    t1.record(stream)
    sync()
    return t0.elapsed_time(t1)


def micro_batch(rng, start, n_frames, n_matches, cap, n_views):
    """-> (slots, best {(slot, feature): (a, b)}, decision [F][cap]): n_matches final matches per frame on distinct landmarks,
    one in 32 a merge with another landmark; decision 2 on those and on as many unmatched features again"""
    import landmark_table_checker as K
    n_lm = len(start) - 1
    slots, best = [], {}
    decision = np.zeros((max(n_frames, 1), cap), np.uint32)
    count = min(cap, n_matches + n_matches // 4)
    for f in range(n_frames):
        lms = rng.choice(n_lm, 2 * n_matches, replace=False)
        feats = rng.permutation(count)[:n_matches]
        matches = []
        for k, j in enumerate(feats):
            if k % 32 == 0:
                best[(f, int(j))] = (int(lms[k]), int(lms[n_matches + k]))
                matches.append((int(j), n_lm + f * cap + int(j)))
                decision[f, j] = 2
            else:
                matches.append((int(j), int(lms[k])))
                decision[f, j] = 1
        for k, j in enumerate(np.setdiff1d(np.arange(count), feats)[:n_matches // 32]):
            best[(f, int(j))] = (int(lms[k]), int(lms[k + 1]))
            decision[f, j] = 2
        slots.append(K.slot(n_views + f, count, matches))
    return slots, best, decision


def step(frames, n_matches, repeat):
    import torch
    import landmark_table_checker as K
    import test_gpu_triangulate as big
    import triangulate_checker as tc
    from cv_amd import _lib, build, triangulation
    from cv_amd.landmark_table import LandmarkUpdate
    from cv_amd.ransac import EssentialConsensus
    from cv_amd.reconstruction import ObservationFilter
    build.build()
    cons = EssentialConsensus(8, 1)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.ExternalStream(cons.stream(), device=dev)
    up = lambda a: None if a is None else _lib.device_bytes(torch, a, dev)
    p = lambda t: None if t is None else t.data_ptr()
    flt, upd = ObservationFilter(cons), LandmarkUpdate(cons)
    kps, poses, start, obs = big.big_map(np.random.default_rng(0x7121))
    nl, (nb, cap) = len(start) - 1, kps.shape
    cam = tc.camera(*big.CAM[:5])
    rcam = _lib.Camera(cam.fx, cam.fy, cam.cx, cam.cy, cam.skew, cam.k1, cam.use_k1, 0)
    table = triangulation.LandmarkTable(torch, start=start, obs=obs)
    d_kps, d_poses = up(kps.view(np.uint8)), up(poses)
    d_rs, d_vs = up(np.array([0, nl], np.uint32)), up(np.array([0, nb], np.uint32))
    o = ObservationFilter._outputs(torch, dev, table.n_obs, nl, 1)
    d_world, d_reason = table.new_world(), torch.zeros((nl,), dtype=torch.uint8, device=dev)
    prm, tprm = ObservationFilter.params(), triangulation.make_params(n_views=nb)

    def run_filter():
        flt.filter_device(d_kps.data_ptr(), cap, nb, d_poses.data_ptr(), rcam, table.d_start.data_ptr(), table.d_obs.data_ptr(), table.n_obs, nl,
                          d_rs.data_ptr(), d_vs.data_ptr(), 1, None, prm, o.keep.data_ptr(), o.lm_state.data_ptr(), o.tri_reason.data_ptr(),
                          o.robust.data_ptr(), o.obs_start_out.data_ptr(), o.obs_out.data_ptr(), o.split_out.data_ptr(), o.counts.data_ptr(),
                          o.recon_verdict.data_ptr(), o.stats.data_ptr())

    def run_tri():
        triangulation.triangulate_landmarks_device(cons._h, table, d_kps, cap, nb, d_poses, rcam, tprm, d_world, d_reason)

    res = {"landmarks": nl, "observations": int(len(obs)), "views": nb, "cap": cap, "matches_per_frame": n_matches, "sizes": {}}
    ok = True
    counts_old = np.bincount(obs[:, 0].astype(np.int64), minlength=nb)[:nb].astype(np.uint32)      # a view's features are its observations
    for F in frames:
        rng = np.random.default_rng(100 + F)
        slots, best, decision = micro_batch(rng, start, F, n_matches, cap, nb)
        cnt = np.zeros(nb + F, np.uint32)
        cnt[:nb] = counts_old
        for s in slots:
            cnt[s["block"]] = s["count"]
        inp = K.inputs(start, obs, len(obs), cap, nb + F, slots, best=best, counts=cnt)
        d_in = {k: up(inp[k]) for k in ("start", "obs", "counts", "matches", "nmatches", "final", "verdict", "pose_out", "best")}
        d_decision = up(decision)
        want_fill = K.outputs(inp)
        d = {k: up(want_fill[k]) for k in K.OUTPUT_NAMES}
        d_mask = torch.zeros((max(F, 1) * cap,), dtype=torch.uint8, device=dev)

        def run_mask():
            upd.sharing_view_device(p(d_in["start"]), p(d_in["obs"]), inp["n_obs"], nl, p(d_in["best"]), p(d_decision), cap, F, p(d_mask))

        def run_add():
            upd.add_views_device(p(d_in["start"]), p(d_in["obs"]), inp["n_obs"], nl, nl, None, None, 0, cap, nb + F, inp["ik"], p(d_in["counts"]),
                                 p(d_in["matches"]), p(d_in["nmatches"]), p(d_in["final"]), p(d_in["verdict"]), p(d_in["pose_out"]), p(d_in["best"]),
                                 None, inp["obs_room"], inp["lm_room"], *(p(d[k]) for k in K.OUTPUT_NAMES))

        torch.cuda.synchronize()
        for fn in (run_mask, run_add, run_filter, run_tri) * 2:                     # warm-up: module load, scratch
            timed(stream, cons.sync, torch, fn)
        t = {"mask": [], "add_views": [], "filter": [], "triangulate": []}
        for _ in range(repeat):
            for name, fn in (("mask", run_mask), ("add_views", run_add), ("filter", run_filter), ("triangulate", run_tri)):
                t[name].append(timed(stream, cons.sync, torch, fn))
        t0 = time.perf_counter()
        want = K.add_views(inp)
        t1 = time.perf_counter()
        want_mask = K.sharing_view(inp["start"], inp["obs"], inp["n_obs"], inp["best"], decision)
        t2 = time.perf_counter()
        got = {k: d[k].cpu().numpy().view(want[k].dtype).reshape(want[k].shape) for k in K.OUTPUT_NAMES}
        same = all(got[k].tobytes() == want[k].tobytes() for k in K.OUTPUT_NAMES) and d_mask.cpu().numpy()[:F * cap].tobytes() == want_mask.tobytes()
        ok = ok and same
        row = {"frames": F, "counts": want["counts_out"].tolist(), "mask_set": int(want_mask.sum()), "lm_room": inp["lm_room"], "obs_room": inp["obs_room"],
               "host_add_views_ms": round((t1 - t0) * 1e3, 2), "host_mask_ms": round((t2 - t1) * 1e3, 2), "bit_equal": bool(same)}
        for name, v in t.items():
            row[name + "_ms_median"], row[name + "_ms_best"] = round(float(np.median(v)), 4), round(min(v), 4)
        res["sizes"][str(F)] = row
    print(json.dumps(res))
    cons.close()
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--matches", type=int, default=2048)
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--step", action="store_true", help="run in this process (the default starts a child under `timeout`)")
    a = ap.parse_args()
    if a.step:
        return step(a.frames, a.matches, a.repeat)
    cmd = ["timeout", "-k", "10", "400", sys.executable, os.path.abspath(__file__), "--step", "--matches", str(a.matches), "--repeat", str(a.repeat),
           "--frames"] + [str(f) for f in a.frames]
    print("#", " ".join(cmd), flush=True)
    return subprocess.run(cmd).returncode


if __name__ == "__main__":
    sys.exit(main())
