#!/usr/bin/env python3
"""Times of the merge of two reconstructions (cv_amd/csrc/rs_reconstruction_merge.hip) against the host build of the same
header on one core.  It has no part in bench.py.

  python tools/bench_reconstruction_merge.py [--map 2048] [--repeat 20]
        one child process under `timeout`.  Two copies of the 50 000-landmark table of tests/test_gpu_triangulate.py's big_map
        (66 views, 805 902 observations, lists of 0 to 48 — the one tools/bench_observation_filter.py times the filter on) over
        disjoint blocks: the destination over blocks [0, 66), the bridging frame in block 66, the source over [67, 133).  The
        bridging frame has --map final matches to destination landmarks drawn at random, its features on source landmarks drawn
        at random: the map has --map entries, all applied.  rs_merge_map_device, rs_incorporate_reconstruction_device and
        rs_normalize_reconstruction_device (132 views, the first view's features on the merged table's keys, 128 constraints),
        and in the same run rs_add_views_device (the bridging frame alone on the destination) and
        rs_triangulate_landmarks_device on the destination — the yardsticks — alternating, `repeat` calls each, HIP-event time
        on rs_stream(): median and best.  The poses the calls update in place are put back in front of every timed call,
        outside the events.  The host build's wall time for the same three calls.  Outputs compared in bytes.
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


def step(n_map, repeat):
    import torch
    import landmark_table_checker as LT
    import reconstruction_merge_checker as K
    import test_gpu_triangulate as big
    import triangulate_checker as tc
    from cv_amd import _lib, build, triangulation
    from cv_amd.landmark_table import LandmarkUpdate
    from cv_amd.ransac import EssentialConsensus
    from cv_amd.reconstruction_merge import ReconstructionMerge
    build.build()
    cons = EssentialConsensus(8, 1)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.ExternalStream(cons.stream(), device=dev)
    up = lambda a: None if a is None else _lib.device_bytes(torch, a, dev)
    p = lambda t: None if t is None else t.data_ptr()
    upd, rm = LandmarkUpdate(cons), ReconstructionMerge(cons)
    kps, poses, start, obs = big.big_map(np.random.default_rng(0x7121))
    nl, (nv, cap) = len(start) - 1, kps.shape
    n_obs, bridge, n_blocks = len(obs), nv, 2 * nv + 1
    rng = np.random.default_rng(0x3e26)
    cam = tc.camera(*big.CAM[:5])
    rcam = _lib.Camera(cam.fx, cam.fy, cam.cx, cam.cy, cam.skew, cam.k1, cam.use_k1, 0)
    src_obs = obs.copy()
    src_obs[:, 0] += nv + 1
    all_kps = np.concatenate([kps, kps[:1], kps])
    all_poses = np.concatenate([poses, poses[:1], poses]).reshape(n_blocks, 12).copy()
    counts = np.zeros(n_blocks, np.uint32)
    counts[:nv] = np.bincount(obs[:, 0].astype(np.int64), minlength=nv)[:nv]
    counts[nv + 1:] = counts[:nv]
    counts[bridge] = min(cap, n_map + n_map // 4)
    # the bridging frame: n_map final matches to destination landmarks, its features on source landmarks
    feats = rng.permutation(int(counts[bridge]))[:n_map]
    dst_lm, src_lm_of = rng.choice(nl, n_map, replace=False), rng.choice(nl, n_map, replace=False)
    src_landmarks = np.full((n_blocks, cap), K.NONE, np.uint32)
    src_landmarks[bridge, feats] = src_lm_of
    slot = LT.slot(bridge, int(counts[bridge]), [(int(j), int(l)) for j, l in zip(feats, dst_lm)], pose=all_poses[bridge])
    av = LT.inputs(start, obs, n_obs, cap, n_blocks, [slot], counts=counts)
    av["poses"] = all_poses.copy()
    minp = dict(matches=av["matches"], nmatches=av["nmatches"], final=av["final"], best=None, n_world=nl, n_dst=nl, cap=cap, slot=0, counts=counts,
                src_landmarks=src_landmarks, n_blocks=n_blocks, bridge_block=bridge)
    K.lib()                                                                         # the host build is compiled before anything is timed
    t0 = time.perf_counter()
    hmap = K.merge_map(minp)
    t_map = time.perf_counter() - t0
    inp = dict(dst_start=start.astype(np.uint32), dst_obs=obs.astype(np.uint32), n_dst_obs=n_obs, n_dst=nl, src_start=start.astype(np.uint32),
               src_obs=src_obs.astype(np.uint32), n_src_obs=n_obs, n_src=nl, map=hmap["map"], map_count=hmap["map_count"], map_room=cap, cap=cap,
               n_blocks=n_blocks, src_blocks=np.arange(nv + 1, n_blocks, dtype=np.uint32), bridge_block=bridge, src_pose=all_poses[bridge].copy(),
               skip=None, obs_room=2 * n_obs, lm_room=2 * nl, poses=all_poses.copy())
    t0 = time.perf_counter()
    want = K.incorporate(inp)
    t_inc = time.perf_counter() - t0

    table = triangulation.LandmarkTable(torch, start=start, obs=obs)
    d_kps, d_poses0 = up(all_kps.view(np.uint8)), torch.from_numpy(all_poses).to(dev)
    d_world, d_reason = table.new_world(), torch.zeros((nl,), dtype=torch.uint8, device=dev)
    tprm = triangulation.make_params(n_views=nv)
    d_av = {k: up(av[k]) for k in ("start", "obs", "counts", "matches", "nmatches", "final", "verdict", "pose_out")}
    av_fill = LT.outputs(av)
    d_avo = {k: up(av_fill[k]) for k in LT.OUTPUT_NAMES}
    d_src = {k: up(inp[k]) for k in ("src_start", "src_obs", "src_pose")}
    d_srclm = up(src_landmarks)
    map_fill, inc_fill = K.map_outputs(minp), K.incorporate_outputs(inp)
    d_map = {k: up(map_fill[k]) for k in ("map", "map_count")}
    d_inc = {k: up(inc_fill[k]) for k in K.IR_OUTPUTS}
    d_inc["poses"] = d_inc["poses"].view(torch.float64).reshape(n_blocks, 12)
    restore_inc = lambda: d_inc["poses"].copy_(d_poses0)

    def run_tri():
        triangulation.triangulate_landmarks_device(cons._h, table, d_kps, cap, nv, d_poses0, rcam, tprm, d_world, d_reason)

    def run_add():
        upd.add_views_device(p(d_av["start"]), p(d_av["obs"]), n_obs, nl, nl, None, None, 0, cap, n_blocks, av["ik"], p(d_av["counts"]),
                             p(d_av["matches"]), p(d_av["nmatches"]), p(d_av["final"]), p(d_av["verdict"]), p(d_av["pose_out"]), None, None,
                             av["obs_room"], av["lm_room"], *(p(d_avo[k]) for k in LT.OUTPUT_NAMES))

    def run_map():
        rm.merge_map_device(p(d_av["matches"]), p(d_av["nmatches"]), p(d_av["final"]), None, nl, nl, cap, 0, p(d_av["counts"]), p(d_srclm), n_blocks,
                            bridge, p(d_map["map"]), p(d_map["map_count"]))

    def run_inc():
        rm.incorporate_device(p(d_av["start"]), p(d_av["obs"]), n_obs, nl, p(d_src["src_start"]), p(d_src["src_obs"]), n_obs, nl, p(d_map["map"]),
                              p(d_map["map_count"]), cap, cap, n_blocks, inp["src_blocks"], bridge, p(d_src["src_pose"]), None, inp["obs_room"],
                              inp["lm_room"], *(p(d_inc[k]) for k in K.IR_OUTPUTS))

    torch.cuda.synchronize()
    timed(stream, cons.sync, torch, run_tri)
    # normalise: the merged reconstruction's 132 views from the first, on the destination's world table
    views = np.concatenate([np.arange(nv), np.arange(nv + 1, n_blocks)]).astype(np.uint32)
    n_constraints = 128
    cposes = np.stack([K.random_pose(rng) for _ in range(2 * n_constraints)]).reshape(n_constraints, 2, 12)
    world = d_world.cpu().numpy()
    ninp = dict(view_blocks=views, counts=counts, landmarks=want["landmarks_out"], cap=cap, n_blocks=n_blocks, world=world, n_world=nl,
                poses=all_poses.copy(), constraint_poses=cposes, n_constraints=n_constraints)
    t0 = time.perf_counter()
    nwant = K.normalize(ninp)
    t_nrm = time.perf_counter() - t0
    d_lm, d_cnt = up(want["landmarks_out"]), up(counts)
    d_nposes, d_cposes0 = torch.from_numpy(all_poses).to(dev), torch.from_numpy(cposes).to(dev)
    d_cposes = d_cposes0.clone()
    d_stats, d_verdict = torch.zeros((2,), dtype=torch.float64, device=dev), torch.zeros((1,), dtype=torch.int32, device=dev)

    def restore_nrm():
        d_nposes.copy_(d_poses0)
        d_cposes.copy_(d_cposes0)

    def run_nrm():
        rm.normalize_device(views, p(d_cnt), p(d_lm), cap, n_blocks, p(d_world), nl, p(d_nposes), p(d_cposes), n_constraints, p(d_stats),
                            p(d_verdict))

    calls = (("merge_map", run_map, None), ("incorporate", run_inc, restore_inc), ("normalize", run_nrm, restore_nrm), ("add_views", run_add, None),
             ("triangulate", run_tri, None))
    for name, fn, before in calls * 2:                                              # warm-up: module load, scratch
        timed(stream, cons.sync, torch, fn, before)
    t = {name: [] for name, _, _ in calls}
    for _ in range(repeat):
        for name, fn, before in calls:
            t[name].append(timed(stream, cons.sync, torch, fn, before))
    back = lambda d, w, names: {k: d[k].cpu().numpy().view(w[k].dtype).reshape(w[k].shape) for k in names}
    got_map, got_inc = back(d_map, hmap, ("map", "map_count")), back(d_inc, want, K.IR_OUTPUTS)
    same = all(got_map[k].tobytes() == hmap[k].tobytes() for k in got_map) and all(got_inc[k].tobytes() == want[k].tobytes() for k in K.IR_OUTPUTS)
    same = same and d_nposes.cpu().numpy().tobytes() == nwant["poses"].tobytes() and d_cposes.cpu().numpy().tobytes() == nwant["constraint_poses"].tobytes()
    same = same and d_stats.cpu().numpy().tobytes() == nwant["stats"].tobytes() and int(d_verdict.cpu().numpy()[0]) == int(nwant["verdict"][0]) == K.NR_OK
    res = {"landmarks_per_side": nl, "observations_per_side": n_obs, "views_per_side": nv, "cap": cap, "map_entries": int(hmap["map_count"][0]),
           "counts": want["counts_out"].tolist(), "call_verdict": int(want["call_verdict"][0]), "normalize_mean": float(nwant["stats"][0]),
           "normalize_features": int(nwant["stats"][1]), "host_merge_map_ms": round(t_map * 1e3, 3), "host_incorporate_ms": round(t_inc * 1e3, 2),
           "host_normalize_ms": round(t_nrm * 1e3, 3), "bit_equal": bool(same)}
    for name, v in t.items():
        res[name + "_ms_median"], res[name + "_ms_best"] = round(float(np.median(v)), 4), round(min(v), 4)
    print(json.dumps(res))
    cons.close()
    return 0 if same else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--map", type=int, default=2048)
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--step", action="store_true", help="run in this process (the default starts a child under `timeout`)")
    a = ap.parse_args()
    if a.step:
        return step(a.map, a.repeat)
    cmd = ["timeout", "-k", "10", "400", sys.executable, os.path.abspath(__file__), "--step", "--map", str(a.map), "--repeat", str(a.repeat)]
    print("#", " ".join(cmd), flush=True)
    return subprocess.run(cmd).returncode


if __name__ == "__main__":
    sys.exit(main())
