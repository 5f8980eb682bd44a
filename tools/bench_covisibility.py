#!/usr/bin/env python3
"""Times of the covisibility search (cv_amd/csrc/rs_covisibility.hip) at the reference's default settings, against the host build
of the same header on one core.  It has no part in bench.py.

  python tools/bench_covisibility.py [--recons 1 64] [--views 256] [--landmarks 50000] [--repeat 5]
        one child process under `timeout`.  A table of --landmarks landmarks over --views views, lists of 0 to 32 observations
        (about 16 a landmark: some 806 000 observations for the defaults), a tenth of the landmarks not robust; every view is a
        target.  For every R of --recons the table R times side by side (blocks and landmarks shifted):
          candidates   rs_covisibility_candidates_device, HIP-event time on rs_stream(): best and median of --repeat calls
          rows         rs_pose_graph_rows_device on the views it wrote
          record       rs_covisibility_record_device on verdicts that accept every filled slot
        and, for one reconstruction, the host build's wall time for the candidates and every output compared in bytes.
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


def side_by_side(tab, r):
    """the table r times: blocks and landmarks of copy i shifted behind those of copy i - 1"""
    n_obs, nb = len(tab["obs"]), tab["n_blocks"]
    start = np.concatenate([[0]] + [tab["start"][1:].astype(np.int64) + n_obs * i for i in range(r)]).astype(np.uint32)
    obs = np.concatenate([tab["obs"] + np.array([nb * i, 0], np.uint32) for i in range(r)])
    return dict(start=start, obs=obs, reason=np.tile(tab["reason"], r), n_blocks=nb * r, cap=tab["cap"])


def step(recons, views, landmarks, repeat):
    import torch
    import covisibility_checker as K
    import covisibility_statement as S
    from cv_amd import _lib, build
    from cv_amd.covisibility import Covisibility
    from cv_amd.pose_graph import PoseGraph
    from cv_amd.ransac import EssentialConsensus
    build.build()
    cons = EssentialConsensus(8, 1)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.ExternalStream(cons.stream(), device=dev)
    up = lambda a: _lib.device_bytes(torch, a, dev)
    cov, pg = Covisibility(cons), PoseGraph(cons)
    prm, p = Covisibility.params(), S.settings()
    one = K.random_table(0xC0715, n_views=views, n_landmarks=landmarks, lengths=(0, 32))
    res, ok = {"views": views, "landmarks": landmarks, "observations": int(len(one["obs"])), "cap": one["cap"], "sizes": {}}, True
    for r in recons:
        tab = side_by_side(one, r)
        n_targets, n_slots = tab["n_blocks"], tab["n_blocks"] * p["limit"]
        targets = np.arange(n_targets, dtype=np.uint32)
        d_start, d_obs, d_reason, d_targets = up(tab["start"]), up(tab["obs"]), up(tab["reason"]), up(targets)
        d_gs = up((np.arange(r + 1) * views).astype(np.uint32))
        z = lambda n: torch.zeros((n,), dtype=torch.int32, device=dev)
        o = dict(views=z(3 * n_slots), lm_start=z(n_slots + 1), lm=z(3 * n_slots * p["max_lm"]), slot_count=z(n_slots), verdict=z(n_targets),
                 stats=z(n_targets * K.STATS))
        d_rs, d_re, d_flag, d_rec, d_cv = z(n_targets + 1), z(6 * n_slots), z(1), z(n_slots), z(n_slots)

        def candidates():
            cov.candidates_device(d_start.data_ptr(), d_obs.data_ptr(), len(tab["obs"]), len(tab["start"]) - 1, tab["cap"], tab["n_blocks"],
                                  d_reason.data_ptr(), d_targets.data_ptr(), n_targets, prm, o["views"].data_ptr(), o["lm_start"].data_ptr(),
                                  o["lm"].data_ptr(), o["slot_count"].data_ptr(), o["verdict"].data_ptr(), o["stats"].data_ptr())

        def rows():
            pg.rows_device(o["views"].data_ptr(), n_slots, n_targets, d_rs.data_ptr(), d_re.data_ptr(), d_flag.data_ptr())

        def record():
            cov.record_device(d_cv.data_ptr(), d_targets.data_ptr(), n_targets, d_gs.data_ptr(), r, prm, d_rec.data_ptr(), o["verdict"].data_ptr(),
                              o["stats"].data_ptr())

        torch.cuda.synchronize()
        t = {}
        for name, fn in (("candidates", candidates), ("rows", rows), ("record", record)):
            timed(stream, cons.sync, torch, fn)                                  # warm-up: module load, scratch
            t[name] = [timed(stream, cons.sync, torch, fn) for _ in range(repeat)]
        stats = o["stats"].cpu().numpy().view(np.uint32).reshape(-1, K.STATS)
        size = {k + "_ms_best": round(min(v), 4) for k, v in t.items()}
        size.update({k + "_ms_median": round(float(np.median(v)), 4) for k, v in t.items()})
        size.update(targets=n_targets, slots_filled=int(stats[:, K.S_EMITTED].sum()), list_entries=int(o["lm_start"][-1].item()),
                    capped_targets=int((stats[:, K.S_FLAGS] & K.F_CAPPED != 0).sum()), stats_first=stats[0].tolist())
        if r == recons[0]:
            t0 = time.perf_counter()
            h = K.candidates(tab, targets, p)
            size["host_candidates_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            same = all(o[k].cpu().numpy().tobytes() == h[k].tobytes() for k in ("views", "lm_start", "lm", "slot_count", "verdict"))
            hs, he, hf = K.rows(h["views"], n_targets)
            same = same and d_rs.cpu().numpy().tobytes() == hs.tobytes() and d_re.cpu().numpy().tobytes() == he.tobytes()
            size["byte_equal"] = bool(same)
            ok = ok and same
        res["sizes"][str(r)] = size
    print(json.dumps(res))
    cons.close()
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--recons", type=int, nargs="+", default=[1, 64])
    ap.add_argument("--views", type=int, default=256)
    ap.add_argument("--landmarks", type=int, default=50000)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--step", action="store_true", help="run in this process (the default starts a child under `timeout`)")
    a = ap.parse_args()
    if a.step:
        return step(a.recons, a.views, a.landmarks, a.repeat)
    cmd = ["timeout", "-k", "10", "400", sys.executable, os.path.abspath(__file__), "--step", "--views", str(a.views), "--landmarks", str(a.landmarks),
           "--repeat", str(a.repeat), "--recons"] + [str(r) for r in a.recons]
    print("#", " ".join(cmd), flush=True)
    return subprocess.run(cmd).returncode


if __name__ == "__main__":
    sys.exit(main())
