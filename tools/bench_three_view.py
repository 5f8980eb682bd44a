#!/usr/bin/env python3
"""Times of the three-view bootstrap (cv_amd/csrc/rs_three_view.hip) at the reference's default settings, against the host
build of the same header on one core.

  python tools/bench_three_view.py [--out DIR]
        chains three steps, each a fresh child process under `timeout`:
          probe   one triple, 1 024 landmarks, patience 512: microseconds per optimiser iteration, from which the limit of
                  the next step is sized (projected time x 3)
          batch   64 triples, 1 024 landmarks each, patience 65 536, 8 filter iterations, one call: wall time, microseconds
                  per optimiser iteration of the longest triple, and a single-triple call of triple 0 (saved with its inputs)
          host    the host build (tests/cpp/three_view_host.c) on triple 0, one core: its time, and poses / verdict / stats
                  against the device's single-triple result (bit equality expected; the tolerance is that of
                  tests/test_three_view_math.py)
  python tools/bench_three_view.py --step probe|batch|host [--out DIR]     one step alone
  python tools/bench_three_view.py --constraints [--out DIR]
        the three-view constraints of the pose graph (cv_amd/csrc/rs_three_view_constraint.hip) at the reference's default
        settings (64 landmarks, 4 096 iterations), one child process under `timeout`: microseconds per iteration of one
        constraint alone and of batches of 256, 2 048 and 8 192, and the host build's time for one (bit equality expected)
Prints one JSON line per step.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CAP, N_COMMON, N_TRIPLES = 1280, 1150, 64
POSE_TOL = 6.6e-14          # tests/test_three_view_math.py FULL_TOL


def scenes(count):
    import three_view_checker as K
    out = []
    for s in range(count):
        rig = K.Rig(9000 + s, N_COMMON, noise=0.5, perturb=2e-3, n_first=60, n_second=60, outliers=40)
        kps, triples, fo, so = rig.scene_arrays(CAP, shuffle_seed=s)
        out.append(dict(kps=kps, triples=triples, n=rig.n, fo=fo, nf=rig.n_first, so=so, ns=rig.n_second, pose_in=rig.pose_in))
    return out


def device_call(torch, cons, sc, prm):
    """-> (seconds of the call from enqueue to completion, verdict [S], stats [S][24], poses [S][24], masks [3][S][cap])"""
    import three_view_checker as K
    from cv_amd import _lib
    from cv_amd.three_view import ThreeViewInit
    S = len(sc)
    dev = torch.device("cuda", 0)
    up = lambda a: _lib.device_bytes(torch, a, dev)
    d_kps = up(np.concatenate([s["kps"] for s in sc]))
    d_pf, d_ps = up(np.stack([s["pose_in"][0] for s in sc])), up(np.stack([s["pose_in"][1] for s in sc]))
    d_t, d_f, d_s = (up(np.stack([s[k] for s in sc])) for k in ("triples", "fo", "so"))
    d_n = up(np.array([[s[k] for s in sc] for k in ("n", "nf", "ns")], np.uint32))
    d_pose = torch.zeros((S, 24), dtype=torch.float64, device=dev)
    d_masks = torch.zeros((3, S, CAP), dtype=torch.uint8, device=dev)
    d_verdict = torch.zeros((S,), dtype=torch.int32, device=dev)
    d_stats = torch.zeros((S, _lib.RS_TV_STATS), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    tv = ThreeViewInit(cons)
    t0 = time.perf_counter()
    tv.init_batch_device(d_kps.data_ptr(), CAP, 3 * S, list(range(0, 3 * S, 3)), list(range(1, 3 * S, 3)), list(range(2, 3 * S, 3)),
                         K.rig_camera_dev(), d_pf.data_ptr(), d_ps.data_ptr(), d_t.data_ptr(), d_n.data_ptr(), d_f.data_ptr(),
                         d_n.data_ptr() + 4 * S, d_s.data_ptr(), d_n.data_ptr() + 8 * S, prm, d_pose.data_ptr(), d_verdict.data_ptr(),
                         d_masks[0].data_ptr(), d_masks[1].data_ptr(), d_masks[2].data_ptr(), d_stats.data_ptr())
    cons.sync()
    sec = time.perf_counter() - t0
    return (sec, d_verdict.cpu().numpy().view(np.uint32), d_stats.cpu().numpy().view(np.uint32), d_pose.cpu().numpy(),
            d_masks.cpu().numpy())


def iterations_of(stats):
    """optimiser iterations a triple made: stop + 1 per run made"""
    from cv_amd import _lib
    stop = stats[_lib.RS_TV_S_RUN_STOP:_lib.RS_TV_S_ROBUST].astype(np.int64)
    return int(np.sum(stop[stop != 0xFFFFFFFF] + 1))


def gpu():
    import torch
    from cv_amd import build
    from cv_amd.ransac import EssentialConsensus
    build.build()
    cons = EssentialConsensus(8, 1)
    cons.reserve(N_TRIPLES)
    return torch, cons


def step_probe(out):
    from cv_amd.three_view import ThreeViewInit
    torch, cons = gpu()
    sc = scenes(1)
    prm = ThreeViewInit.params(three_view_patience=512)
    device_call(torch, cons, sc, prm)                                   # warm-up: module load
    sec, verdict, stats, _, _ = device_call(torch, cons, sc, prm)
    it = iterations_of(stats[0])
    res = {"step": "probe", "triples": 1, "landmarks": int(stats[0][4]), "patience": 512, "verdict": int(verdict[0]), "iterations": it,
           "call_ms": round(sec * 1e3, 2), "us_per_iteration": round(sec * 1e6 / max(it, 1), 2),
           "note": "the call's wall time over its optimiser iterations: the classification passes are inside"}
    with open(os.path.join(out, "probe.json"), "w") as f:
        json.dump(res, f)
    print(json.dumps(res))
    cons.close()


def step_batch(out):
    from cv_amd.three_view import ThreeViewInit
    torch, cons = gpu()
    sc = scenes(N_TRIPLES)
    prm = ThreeViewInit.params()
    device_call(torch, cons, sc[:1], ThreeViewInit.params(three_view_patience=8))
    sec, verdict, stats, _, _ = device_call(torch, cons, sc, prm)
    its = [iterations_of(s) for s in stats]
    one_sec, v1, s1, p1, m1 = device_call(torch, cons, sc[:1], prm)
    np.savez(os.path.join(out, "triple0.npz"), verdict=v1, stats=s1, poses=p1, masks=m1[:, 0])
    res = {"step": "batch", "triples": N_TRIPLES, "landmarks": [int(s[4]) for s in stats][:4], "patience": 65536, "filter_iterations": 8,
           "verdicts": np.bincount(verdict, minlength=7).tolist(), "call_s": round(sec, 3), "iterations_longest_triple": max(its),
           "iterations_all": int(sum(its)), "us_per_iteration_longest_triple": round(sec * 1e6 / max(max(its), 1), 2),
           "single_triple_call_s": round(one_sec, 3), "single_triple_us_per_iteration": round(one_sec * 1e6 / max(iterations_of(s1[0]), 1), 2)}
    print(json.dumps(res))
    cons.close()


def step_host(out):
    import three_view_checker as K
    sc = scenes(1)[0]
    kps = sc["kps"]
    t0 = time.perf_counter()
    h = K.init_scene(kps, 3, [0, 1, 2], K.rig_camera(), sc["pose_in"], sc["triples"], sc["n"], sc["fo"], sc["nf"], sc["so"], sc["ns"], K.settings())
    sec = time.perf_counter() - t0
    it = iterations_of(h["stats"])
    res = {"step": "host", "what": "tests/cpp/three_view_host.c, gcc -O2 -ffp-contract=off, one core", "verdict": h["verdict"], "iterations": it,
           "seconds": round(sec, 2), "us_per_iteration": round(sec * 1e6 / max(it, 1), 2)}
    path = os.path.join(out, "triple0.npz")
    if os.path.exists(path):
        d = np.load(path)
        dev_pose = d["poses"][0]
        res["device_verdict"] = int(d["verdict"][0])
        res["stats_equal"] = bool(np.array_equal(d["stats"][0], h["stats"]))
        ok = h["verdict"] == 0 and res["device_verdict"] == 0
        res["poses_bit_equal"] = bool(ok and dev_pose.tobytes() == h["pose_out"].tobytes())
        res["poses_max_abs_difference"] = float(np.max(np.abs(dev_pose - h["pose_out"]))) if ok else None
        res["masks_equal"] = bool(ok and all(np.array_equal(d["masks"][m], h[k]) for m, k in enumerate(("combined", "first_ok", "second_ok"))))
        res["within_tolerance"] = bool(res["device_verdict"] == h["verdict"] and (not ok or res["poses_max_abs_difference"] <= POSE_TOL))
    print(json.dumps(res))
    return 0 if res.get("within_tolerance", True) else 1


def step_constraints(out):
    import three_view_constraint_checker as T
    from cv_amd import _lib
    from cv_amd.three_view import ThreeViewConstraints
    torch, cons = gpu()
    cap, n_lm, patience = 64, 64, 4096
    pool = [T.scene(9100 + k, n_lm) for k in range(16)]
    dev = torch.device("cuda", 0)
    up = lambda a: _lib.device_bytes(torch, a, dev)
    cam = _lib.Camera(T.K.CAM["fx"], T.K.CAM["fy"], T.K.CAM["cx"], T.K.CAM["cy"], 0.0, 0.0, 0, 0)
    tvc = ThreeViewConstraints(cons)

    def call(n, prm):
        rng = np.random.default_rng(n)
        arrays = T.device_arrays(pool, cap, [(i % len(pool), rng.permutation(n_lm)) for i in range(n)])
        kps, poses, views, lm_start, lm = arrays
        d = [up(a) for a in arrays]
        d_pose = torch.zeros((n, 24), dtype=torch.float64, device=dev)
        d_verdict = torch.zeros((n,), dtype=torch.int32, device=dev)
        d_stats = torch.zeros((n, _lib.RS_TVC_STATS), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tvc.batch_device(d[0].data_ptr(), cap, len(kps), d[1].data_ptr(), cam, d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(), len(lm), n,
                         prm, d_pose.data_ptr(), d_verdict.data_ptr(), d_stats.data_ptr())
        cons.sync()
        sec = time.perf_counter() - t0
        return sec, arrays, d_verdict.cpu().numpy().view(np.uint32), d_stats.cpu().numpy().view(np.uint32), d_pose.cpu().numpy()

    call(1, ThreeViewConstraints.params(constraint_patience=8))                 # warm-up: module load
    prm = ThreeViewConstraints.params()
    res = {"step": "constraints", "landmarks": n_lm, "patience": patience, "batches": {}}
    for n in (1, 256, 2048, 8192):
        sec = min(call(n, prm)[0] for _ in range(3))
        _, arrays, verdict, stats, pose = call(n, prm)
        assert np.all(verdict == 0), np.bincount(verdict)
        res["batches"][str(n)] = {"call_ms": round(sec * 1e3, 3), "us_per_iteration": round(sec * 1e6 / patience, 3),
                                  "us_per_constraint_iteration": round(sec * 1e6 / patience / n, 5)}
        if n == 1:
            t0 = time.perf_counter()
            h = T.constraint_scene(arrays[0], arrays[1], T.K.rig_camera(), arrays[2], arrays[3], arrays[4], 0, T.settings())
            hsec = time.perf_counter() - t0
            res["host"] = {"what": "tests/cpp/three_view_constraint_host.c, gcc -O2 -ffp-contract=off, one core", "seconds": round(hsec, 4),
                           "us_per_iteration": round(hsec * 1e6 / patience, 3), "verdict": h["verdict"],
                           "stats_equal": bool(np.array_equal(stats[0], h["stats"])), "poses_bit_equal": bool(pose[0].tobytes() == h["pose_out"].tobytes())}
    with open(os.path.join(out, "constraints.json"), "w") as f:
        json.dump(res, f)
    print(json.dumps(res))
    cons.close()
    return 0 if res["host"]["stats_equal"] and res["host"]["poses_bit_equal"] else 1


def child(step, out, limit):
    cmd = ["timeout", "-k", "10", str(int(limit)), sys.executable, os.path.abspath(__file__), "--step", step, "--out", out]
    print("#", " ".join(cmd), flush=True)
    return subprocess.run(cmd).returncode


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["probe", "batch", "host", "constraints"])
    ap.add_argument("--constraints", action="store_true", help="time the three-view constraints instead of the bootstrap")
    ap.add_argument("--out", default=os.path.join(tempfile.gettempdir(), "bench_three_view"), help="where the steps leave their files")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    if a.step:
        return {"probe": step_probe, "batch": step_batch, "host": step_host, "constraints": step_constraints}[a.step](a.out) or 0
    if a.constraints:
        return child("constraints", a.out, 300)
    rc = child("probe", a.out, 120)
    if rc:
        return rc
    with open(os.path.join(a.out, "probe.json")) as f:
        us = json.load(f)["us_per_iteration"]
    projected = us * 1e-6 * 9 * 65536
    print(f"# projected time of one default-settings call: {projected:.1f} s", flush=True)
    rc = child("batch", a.out, 60 + 3 * 2 * projected)          # two default-settings calls in the step
    if rc:
        return rc
    return child("host", a.out, 1500)


if __name__ == "__main__":
    sys.exit(main())
