#!/usr/bin/env python3
"""Times of the observation filter and of the optimize_reconstruction chain (cv_amd/csrc/rs_observation_filter.hip) at the
reference's default settings, against the host builds of the same headers on one core.  It has no part in bench.py.

  python tools/bench_observation_filter.py [--graphs 1 64] [--views 256] [--landmarks 1024] [--rounds 1024] [--repeat 20]
        one child process under `timeout`.
          filter   rs_filter_observations_device on the 50 000-landmark table of tests/test_gpu_triangulate.py's big_map (66
                   views, lists of 0 to 48), next to rs_triangulate_landmarks_device on the same table — that kernel is the
                   yardstick — the two alternating, `repeat` calls each, HIP-event time on rs_stream(): median and best.  The
                   host build's wall time for the same pass.  Outputs compared in bytes.
          chain    for every G of --graphs: G ring graphs of --views views (18 edges a row) with --landmarks landmarks each,
                   rs_optimize_reconstruction_batch_device (one round: --rounds Jacobi rounds, the filter, the world table) next
                   to rs_pose_graph_relax_batch_device alone on the same graphs, alternating, three calls each, the best.  The
                   host builds' wall time for one reconstruction.
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


def ring_landmarks(graph, n, rng, f=1000.0, cx=960.0, cy=540.0):
    """n landmarks of 2 to 7 observations among the views of a pose_graph_checker.Graph that have them a unit or more in front,
    0.5 px noise, every fifth with one observation displaced by 40 to 120 px -> (kps [views][n], start, obs)"""
    import observation_filter_checker as F
    kps = np.zeros((graph.n, n), F.KP_DTYPE)
    used = np.zeros(graph.n, np.int64)
    start, obs = [0], []
    for _ in range(n):
        while True:
            X = rng.uniform(-5.0, 5.0, 3)
            visible = np.flatnonzero(graph.truth[:, 2, :3] @ X + graph.truth[:, 2, 3] > 1.0)
            if len(visible) >= 2:
                break
        views = rng.permutation(visible)[:rng.integers(2, min(len(visible), 7) + 1)]
        bad = rng.integers(0, len(views)) if rng.random() < 0.2 else -1
        for k, v in enumerate(views):
            q = graph.truth[v][:, :3] @ X + graph.truth[v][:, 3]
            x, y = f * q[0] / q[2] + cx + rng.uniform(-0.5, 0.5), f * q[1] / q[2] + cy + rng.uniform(-0.5, 0.5)
            kps[v, used[v]]["x"], kps[v, used[v]]["y"] = x + (rng.uniform(40, 120) if k == bad else 0.0), y
            obs.append((v, used[v]))
            used[v] += 1
        start.append(len(obs))
    return kps, np.array(start, np.uint32), np.array(obs, np.uint32).reshape(-1, 2)


def timed(stream, sync, torch, fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(stream)
    fn()
    t1.record(stream)
    sync()
    return t0.elapsed_time(t1)


def step(graphs, views, landmarks, rounds, repeat):
    import torch
    import observation_filter_checker as F
    import pose_graph_checker as P
    import test_gpu_triangulate as big
    import triangulate_checker as tc
    from cv_amd import _lib, build, triangulation
    from cv_amd.pose_graph import PoseGraph
    from cv_amd.ransac import EssentialConsensus
    from cv_amd.reconstruction import ObservationFilter, ReconstructionOptimizer
    build.build()
    cons = EssentialConsensus(8, 1)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.ExternalStream(cons.stream(), device=dev)
    up = lambda a: _lib.device_bytes(torch, a, dev)
    flt, pg = ObservationFilter(cons), PoseGraph(cons)
    res, ok = {}, True

    # ---- the filter alone, next to the triangulation of the same table ----
    kps, poses, start, obs = big.big_map(np.random.default_rng(0x7121))
    nl, (nb, cap) = len(start) - 1, kps.shape
    cam = tc.camera(*big.CAM[:5])
    rcam = _lib.Camera(cam.fx, cam.fy, cam.cx, cam.cy, cam.skew, cam.k1, cam.use_k1, 0)
    table = triangulation.LandmarkTable(torch, start=start, obs=obs)
    d_kps, d_poses = up(kps.view(np.uint8)), up(poses)
    rs, vs = np.array([0, nl], np.uint32), np.array([0, nb], np.uint32)
    d_rs, d_vs = up(rs), up(vs)
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

    torch.cuda.synchronize()
    for fn in (run_filter, run_tri, run_filter, run_tri):                       # warm-up: module load, scratch
        timed(stream, cons.sync, torch, fn)
    tf, tt = [], []
    for _ in range(repeat):
        tf.append(timed(stream, cons.sync, torch, run_filter))
        tt.append(timed(stream, cons.sync, torch, run_tri))
    t0 = time.perf_counter()
    h = F.filter_table(kps, poses, cam, start, obs, rs, vs)
    host = time.perf_counter() - t0
    same = (np.array_equal(o.keep.cpu().numpy()[:len(obs)], h["keep"]) and np.array_equal(o.obs_start_out.cpu().numpy().view(np.uint32), h["start_out"]) and
            np.array_equal(o.lm_state.cpu().numpy(), h["state"]) and np.array_equal(o.stats.cpu().numpy().view(np.uint32)[0], h["stats"][0]))
    ok = ok and same
    res["filter"] = {"landmarks": nl, "observations": int(len(obs)), "filter_ms_median": round(float(np.median(tf)), 4), "filter_ms_best": round(min(tf), 4),
                     "triangulate_ms_median": round(float(np.median(tt)), 4), "triangulate_ms_best": round(min(tt), 4),
                     "ratio_of_medians": round(float(np.median(tf) / np.median(tt)), 3), "host_ms": round(host * 1e3, 2), "stats": h["stats"][0].tolist(),
                     "bit_equal": bool(same)}

    # ---- the chain next to the relaxation alone ----
    res["chain"] = {"views": views, "landmarks_per_reconstruction": landmarks, "rounds": rounds, "sizes": {}}
    one = P.Graph(7000 + views, views, triples=[(i, (i + 1) % views, (i + 2) % views) for i in range(views)], noise=1e-3)
    k1, s1, o1 = ring_landmarks(one, landmarks, np.random.default_rng(5))
    pgp = PoseGraph.params(optimization_iterations=rounds)
    for g in graphs:
        A = P.batch([one] * g)
        kps_g = np.concatenate([k1] * g)
        start_g = np.concatenate([[0]] + [s1[1:].astype(np.int64) + int(s1[-1]) * i for i in range(g)]).astype(np.uint32)
        obs_g = np.concatenate([o1 + np.array([views * i, 0], np.uint32) for i in range(g)])
        recon = (np.arange(g + 1) * landmarks).astype(np.uint32)
        d = {k: up(A[k]) for k in ("graph_start", "row_start", "row_edges", "views", "cverdict", "edges")}
        d_k, d_recon = up(kps_g.view(np.uint8)), up(recon)
        tab = triangulation.LandmarkTable(torch, start=start_g, obs=obs_g)
        n_views, n_c = len(A["poses"]), len(A["views"])
        oc = ObservationFilter._outputs(torch, dev, tab.n_obs, tab.n_landmarks, g)
        d_v = torch.zeros((g * (2 + P.STATS) + n_views,), dtype=torch.int32, device=dev)
        d_w, d_r = tab.new_world(), torch.zeros((tab.n_landmarks,), dtype=torch.uint8, device=dev)
        opt = ReconstructionOptimizer(pg)
        state = {}

        def chain():
            state["poses"] = up(A["poses"])
            torch.cuda.synchronize()
            return lambda: opt.optimize_device(
                state["poses"].data_ptr(), n_views, d["graph_start"].data_ptr(), g, d["row_start"].data_ptr(), d["row_edges"].data_ptr(),
                len(A["row_edges"]), d["views"].data_ptr(), d["cverdict"].data_ptr(), d["edges"].data_ptr(), n_c, pgp, d_k.data_ptr(), landmarks, rcam,
                tab.d_start.data_ptr(), tab.d_obs.data_ptr(), tab.n_obs, tab.n_landmarks, d_recon.data_ptr(), prm, d_v.data_ptr(),
                d_v.data_ptr() + 4 * g, d_v.data_ptr() + 4 * g * (2 + P.STATS), d_v.data_ptr() + 8 * g, oc.keep.data_ptr(), oc.lm_state.data_ptr(),
                oc.tri_reason.data_ptr(), oc.robust.data_ptr(), oc.obs_start_out.data_ptr(), oc.obs_out.data_ptr(), oc.split_out.data_ptr(),
                oc.counts.data_ptr(), oc.recon_verdict.data_ptr(), oc.stats.data_ptr(), d_w.data_ptr(), d_r.data_ptr())

        def relax():
            state["poses"] = up(A["poses"])
            torch.cuda.synchronize()
            return lambda: pg.relax_batch_device(
                state["poses"].data_ptr(), n_views, d["graph_start"].data_ptr(), g, d["row_start"].data_ptr(), d["row_edges"].data_ptr(),
                len(A["row_edges"]), d["views"].data_ptr(), d["cverdict"].data_ptr(), d["edges"].data_ptr(), n_c, pgp, d_v.data_ptr() + 4 * g,
                d_v.data_ptr() + 4 * g * (2 + P.STATS), d_v.data_ptr() + 8 * g)

        timed(stream, cons.sync, torch, chain())                              # warm-up
        timed(stream, cons.sync, torch, relax())
        tc_, tr_ = [], []
        for _ in range(3):
            tr_.append(timed(stream, cons.sync, torch, relax()))
            tc_.append(timed(stream, cons.sync, torch, chain()))
        got_poses = state["poses"].cpu().numpy().view(np.float64).reshape(-1, 12)
        verdict = d_v[:g].cpu().numpy()
        H = P.batch([one])
        t0 = time.perf_counter()
        hp = P.relax(H, P.settings(rounds))
        t1 = time.perf_counter()
        hf = F.filter_table(k1, hp["poses"], cam, s1, o1, np.array([0, landmarks], np.uint32), H["graph_start"])
        t2 = time.perf_counter()
        same = (got_poses[:views].tobytes() == hp["poses"].tobytes() and np.array_equal(oc.keep.cpu().numpy()[:len(o1)], hf["keep"]) and
                np.array_equal(oc.stats.cpu().numpy().view(np.uint32)[0], hf["stats"][0]) and
                np.array_equal(oc.obs_start_out.cpu().numpy().view(np.uint32)[:landmarks + 1], hf["start_out"]))
        ok = ok and same
        res["chain"]["sizes"][str(g)] = {"chain_ms_best": round(min(tc_), 3), "chain_ms": [round(t, 3) for t in tc_], "relax_ms_best": round(min(tr_), 3),
                                         "relax_ms": [round(t, 3) for t in tr_], "filter_and_world_ms": round(min(tc_) - min(tr_), 3),
                                         "observations": int(tab.n_obs), "verdicts_ok": int((verdict == 0).sum()),
                                         "host_relax_one_ms": round((t1 - t0) * 1e3, 2), "host_filter_one_ms": round((t2 - t1) * 1e3, 2),
                                         "stats_first": hf["stats"][0].tolist(), "bit_equal": bool(same)}
    print(json.dumps(res))
    cons.close()
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, nargs="+", default=[1, 64])
    ap.add_argument("--views", type=int, default=256)
    ap.add_argument("--landmarks", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=1024)
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--step", action="store_true", help="run in this process (the default starts a child under `timeout`)")
    a = ap.parse_args()
    if a.step:
        return step(a.graphs, a.views, a.landmarks, a.rounds, a.repeat)
    cmd = ["timeout", "-k", "10", "400", sys.executable, os.path.abspath(__file__), "--step", "--views", str(a.views), "--landmarks", str(a.landmarks),
           "--rounds", str(a.rounds), "--repeat", str(a.repeat), "--graphs"] + [str(g) for g in a.graphs]
    print("#", " ".join(cmd), flush=True)
    return subprocess.run(cmd).returncode


if __name__ == "__main__":
    sys.exit(main())
