#!/usr/bin/env python3
"""Times of the two steps that start a reconstruction (cv_amd/csrc/rs_bootstrap_table.hip) against the host build of the same
header on one core, and of the chain reconstruction.start_reconstructions against the same chain with its two host steps.  It
has no part in bench.py.

  python tools/bench_bootstrap.py [--scenes 1 8 64] [--inliers 2048] [--repeat 20]
        one child process under `timeout`.  For every S of --scenes: 2 S slots of --inliers inliers each over 9/8 as many features
        (cap; a list lacks one centre feature in nine of the other's), S scenes; rs_join_pairs_batch_device without and with RS_BATCH_SHUFFLE and
        rs_add_reconstruction_batch_device on the join's lists with nine masks in ten set, `repeat` calls each after two warm-up
        calls, HIP-event time on rs_stream(): median and best.  The host build's wall time for the same calls.  Outputs compared
        in bytes.
        The chain: three synthetic views of 200 points at cap 256 (tests/test_gpu_bootstrap.py's), the bootstrap at patience 64
        with two filter rounds; wall time from the first enqueue to the end of the wait, median of `repeat`:
        start_reconstructions, and the same stages with the read back, three_view.join_pairs and a Python table
        (tests/bootstrap_table_statement.py) in between.
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


def calls(rng, n_scenes, n_inliers):
    """-> (join inputs, add inputs over the host join's lists)"""
    import bootstrap_table_checker as K
    cap = n_inliers + n_inliers // 8
    slots = [K.slot(list(zip(rng.permutation(cap)[:n_inliers].tolist(), rng.permutation(cap)[:n_inliers].tolist()))) for _ in range(2 * n_scenes)]
    jin = K.join_inputs(slots, [(2 * s, 2 * s + 1) for s in range(n_scenes)], cap, minimum=256)
    joined = K.join(jin)
    ain = K.add_inputs([K.scene((3 * s, 3 * s + 1, 3 * s + 2), (cap, cap, cap)) for s in range(n_scenes)], cap, 3 * n_scenes, 3 * n_scenes, 0)
    for k in K.JOIN_OUTPUT_NAMES[:6]:
        ain[k] = joined[k]
    for k in ("combined", "first_ok", "second_ok"):
        ain[k] = (rng.random((n_scenes, cap)) < 0.9).astype(np.uint8)
    return jin, ain


def chain(torch, repeat):
    import bootstrap_table_checker as K
    import bootstrap_table_statement as S
    import test_gpu_bootstrap as T
    from cv_amd import _lib, triangulation
    from cv_amd.pose_graph import PoseGraph
    from cv_amd.ransac import EssentialConsensus
    from cv_amd.reconstruction import ReconstructionOptimizer, start_reconstructions
    from cv_amd.three_view import ThreeViewInit, join_pairs
    cap, n = 256, 200
    kps, feature, cam = T.synthetic_views(61, n, cap)
    dev = torch.device("cuda", 0)
    c = EssentialConsensus(2048, 1024)
    c.reserve(2)
    d_kps = _lib.device_bytes(torch, kps, dev)
    counts = np.array([n, n, n], np.uint32)
    rng = np.random.default_rng(4)
    pairs = np.zeros((2, cap, 2), np.uint32)
    for k in (0, 1):
        order = rng.permutation(n)
        pairs[k, :n] = np.stack([feature[0][order], feature[k + 1][order]], 1)
    d_pairs, d_npairs = torch.from_numpy(pairs.view(np.int32)).to(dev), torch.from_numpy(np.array([n, n], np.int32)).to(dev)
    arrsac = c.make_params(1e-5, n_hypotheses=256, seed=7, block_size=64, init_blocks=1, max_candidates=64, halve=True)
    tv = ThreeViewInit.params(three_view_patience=64, three_view_filter_loop_iterations=2)
    seed = 12345
    opt = ReconstructionOptimizer(PoseGraph(c))
    u32 = lambda t: t.cpu().numpy().view(np.uint32)

    def device_chain():
        return start_reconstructions(torch, c, d_kps, counts, cap, cam, d_pairs, d_npairs, [0, 0], [1, 2], arrsac, [(0, 1)], [0], [1], [2], 3, 0,
                                     minimum=64, seed=seed, tv_params=tv)

    def host_chain():
        z = lambda dt, *shape: torch.zeros(shape, dtype=dt, device=dev)
        d_pose, d_best, d_inl, d_ninl = z(torch.float64, 2, 12), z(torch.int32, 2), z(torch.int32, 2, cap), z(torch.int32, 2)
        c.model_inliers_batch_device(d_kps, d_kps, cap, [0, 0], [1, 2], d_pairs, d_npairs, cam, cam, arrsac, d_pose, d_best, d_inl, d_ninl,
                                     stream_to_wait=torch.cuda.current_stream(dev))
        c.sync()
        inl, ninl, pose = u32(d_inl), u32(d_ninl), d_pose.cpu().numpy().reshape(2, 3, 4)
        lists = [pairs[k][inl[k, :ninl[k]]] for k in (0, 1)]
        perm = S.shuffle_permutation(seed, 0, len(join_pairs(lists[0], lists[1])[0]))
        host = ThreeViewInit(c).init(torch, [kps[v][:n] for v in range(3)], cam, pose[0], pose[1], lists[0], lists[1], tv, permutation=perm)
        triples, first_only, second_only = join_pairs(lists[0], lists[1], permutation=perm)
        scene = K.scene((0, 1, 2), (n, n, n), triples.tolist(), host.combined.astype(int).tolist(), first_only.tolist(),
                        host.first_ok.astype(int).tolist(), second_only.tolist(), host.second_ok.astype(int).tolist(), pose=host.poses.reshape(24))
        inp = K.add_inputs([scene], cap, 3, 3, 0)
        inp["kps"] = kps.view(np.uint8).reshape(3, cap, 28)
        o = S.add_reconstruction(inp, K.add_outputs(inp))
        rows, n_obs = (int(v) for v in o["counts_out"][:2])
        table = triangulation.LandmarkTable(torch, start=o["obs_start_out"][:rows + 1], obs=o["obs_out"][:n_obs])
        d_dst, d_poses = _lib.device_bytes(torch, o["kps_dst"], dev), torch.from_numpy(o["poses"]).to(dev)
        pg = opt._pg
        edges = pg.edges(torch, o["views_out"], (o["constraint_poses_out"], o["constraint_verdict_out"]))
        rws = pg.rows(torch, torch.from_numpy(o["views_out"].view(np.int32)).to(dev), 3)
        out = opt.run_tensors(torch, d_poses, o["view_start_out"], rws[0], rws[1], edges, table, d_dst, cap, cam, o["recon_start_out"])
        c.sync()
        return out

    res = {}
    for name, fn in (("device", device_chain), ("host_steps", host_chain)):
        fn()
        t = []
        for _ in range(repeat):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e3)
        res[name + "_ms_median"], res[name + "_ms_best"] = round(float(np.median(t)), 3), round(min(t), 3)
    r = device_chain()
    res["bootstrap_verdict"], res["frame_verdict"] = int(u32(r.bootstrap[0])[0]), int(u32(r.start.frame_verdict)[0])
    res["rows"], res["observations"] = (int(v) for v in u32(r.start.counts_out)[:2])
    c.close()
    return res


def step(scenes, n_inliers, repeat):
    import torch
    import bootstrap_table_checker as K
    import test_gpu_bootstrap as T
    from cv_amd import _lib, build
    from cv_amd.bootstrap import PairJoin, ReconstructionStart
    from cv_amd.ransac import EssentialConsensus
    build.build()
    cons = EssentialConsensus(8, 1)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.ExternalStream(cons.stream(), device=dev)
    up = lambda a: None if a is None else _lib.device_bytes(torch, a, dev)
    res = {"inliers_per_list": n_inliers, "cap": n_inliers + n_inliers // 8, "sizes": {}}
    ok = True
    for S in scenes:
        jin, ain = calls(np.random.default_rng(100 + S), S, n_inliers)
        row = {"scenes": S}
        d_j = {k: up(jin[k]) for k in ("pairs", "npairs", "inliers", "n_inliers", "best_id", "pose")}
        d_a = {k: up(ain[k]) for k in T.ADD_INPUTS}
        for shuffle in (False, True):
            jin["flags"], jin["seed"] = int(shuffle), 77
            fill = K.join_outputs(jin)
            d = {k: up(fill[k]) for k in K.JOIN_OUTPUT_NAMES}

            def run_join():
                PairJoin(cons).join_device(*(d_j[k] for k in ("pairs", "npairs", "inliers", "n_inliers", "best_id", "pose")), jin["n_slots"],
                                           jin["cap"], jin["slot_first"], jin["slot_second"], *(d[k] for k in K.JOIN_OUTPUT_NAMES),
                                           minimum=jin["minimum"], shuffle=shuffle, seed=77)

            torch.cuda.synchronize()
            for _ in range(2):
                timed(stream, cons.sync, torch, run_join)
            t = [timed(stream, cons.sync, torch, run_join) for _ in range(repeat)]
            t0 = time.perf_counter()
            want = K.join(jin)
            host_ms = (time.perf_counter() - t0) * 1e3
            got = {k: d[k].cpu().numpy().view(want[k].dtype).reshape(want[k].shape) for k in K.JOIN_OUTPUT_NAMES}
            same = K.same(got, want, K.JOIN_OUTPUT_NAMES) == []
            ok = ok and same
            name = "join_shuffled" if shuffle else "join"
            row[name + "_ms_median"], row[name + "_ms_best"], row["host_" + name + "_ms"] = round(float(np.median(t)), 4), round(min(t), 4), round(host_ms, 2)
            row[name + "_bit_equal"] = bool(same)
        row["triples"] = int(want["ntriples"].sum())
        fill = K.add_outputs(ain)
        d = {k: up(fill[k]) for k in K.ADD_OUTPUT_NAMES}

        def run_add():
            ReconstructionStart(cons).add_device(
                *(d_a[k] for k in T.ADD_INPUTS[:11]), ain["ic"], ain["i_first"], ain["i_second"], d_a["kps"], d_a["counts"], ain["n_src_blocks"],
                ain["cap"], None, None, None, 0, 0, None, None, 0, d["kps_dst"], d["counts_dst"], d["poses"], ain["n_blocks"], 0, ain["obs_room"],
                ain["lm_room"], *(d[k] for k in K.ADD_OUTPUT_NAMES[3:]))

        torch.cuda.synchronize()
        for _ in range(2):
            timed(stream, cons.sync, torch, run_add)
        t = [timed(stream, cons.sync, torch, run_add) for _ in range(repeat)]
        t0 = time.perf_counter()
        want = K.add(ain)
        host_ms = (time.perf_counter() - t0) * 1e3
        got = {k: d[k].cpu().numpy().view(want[k].dtype).reshape(want[k].shape) for k in K.ADD_OUTPUT_NAMES}
        same = K.same(got, want, K.ADD_OUTPUT_NAMES) == []
        ok = ok and same
        row.update(add_ms_median=round(float(np.median(t)), 4), add_ms_best=round(min(t), 4), host_add_ms=round(host_ms, 2), add_bit_equal=bool(same),
                   counts=want["counts_out"].tolist())
        res["sizes"][str(S)] = row
    cons.close()
    res["chain"] = chain(torch, repeat)
    print(json.dumps(res))
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--inliers", type=int, default=2048)
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--step", action="store_true", help="run in this process (the default starts a child under `timeout`)")
    a = ap.parse_args()
    if a.step:
        return step(a.scenes, a.inliers, a.repeat)
    cmd = ["timeout", "-k", "10", "400", sys.executable, os.path.abspath(__file__), "--step", "--inliers", str(a.inliers), "--repeat", str(a.repeat),
           "--scenes"] + [str(s) for s in a.scenes]
    print("#", " ".join(cmd), flush=True)
    return subprocess.run(cmd).returncode


if __name__ == "__main__":
    sys.exit(main())
