#!/usr/bin/env python3
"""Times of the pose-graph relaxation (cv_amd/csrc/rs_pose_graph.hip) at the reference's default settings (1 024 rounds, rate
1e-3), against the host build of the same header on one core.  It has no part in bench.py.

  python tools/bench_pose_graph.py [--views N ...] [--graphs G] [--rounds R]
        one child process under `timeout`.  For every N: G ring graphs of N views, every view in 3 constraints (18 edges a
        row), relaxed in one call
          - by the resident form (N <= 256), HIP-event time on rs_stream(), the best of three calls;
          - by the swept form (the resident limit set to 0), the same way;
          - by the host build (tests/cpp/pose_graph_host.c, gcc -O2 -ffp-contract=off, one core), one graph, wall time.
        The three results are compared in bytes.
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


def step(views, graphs, rounds):
    import torch
    import pose_graph_checker as P
    from cv_amd import _lib, build
    from cv_amd.pose_graph import PoseGraph
    from cv_amd.ransac import EssentialConsensus
    build.build()
    cons = EssentialConsensus(8, 1)
    pg = PoseGraph(cons)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.ExternalStream(cons.stream(), device=dev)
    up = lambda a: _lib.device_bytes(torch, a, dev)
    prm = PoseGraph.params(optimization_iterations=rounds)
    res = {"rounds": rounds, "rate": prm.graph_optimization_rate, "graphs_per_call": graphs, "edges_per_view": 18, "sizes": {}}
    ok = True
    for n in views:
        one = P.Graph(7000 + n, n, triples=[(i, (i + 1) % n, (i + 2) % n) for i in range(n)])
        A = P.batch([one] * graphs)
        d = {k: up(A[k]) for k in ("graph_start", "row_start", "row_edges", "views", "cverdict", "edges")}
        n_views, n_c = len(A["poses"]), len(A["views"])
        d_out = torch.zeros((graphs * (1 + P.STATS) + n_views,), dtype=torch.int32, device=dev)

        def call(resident):
            d_poses = up(A["poses"])
            torch.cuda.synchronize()
            pg.resident_views(resident)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(stream)
            pg.relax_batch_device(d_poses.data_ptr(), n_views, d["graph_start"].data_ptr(), graphs, d["row_start"].data_ptr(),
                                  d["row_edges"].data_ptr(), len(A["row_edges"]), d["views"].data_ptr(), d["cverdict"].data_ptr(),
                                  d["edges"].data_ptr(), n_c, prm, d_out.data_ptr(), d_out.data_ptr() + 4 * graphs * (1 + P.STATS),
                                  d_out.data_ptr() + 4 * graphs)
            t1.record(stream)
            cons.sync()
            pg.resident_views()
            verdict = d_out[:graphs].cpu().numpy()
            assert np.all(verdict == _lib.RS_PG_OK), verdict
            return t0.elapsed_time(t1), d_poses.cpu().numpy().view(np.float64).reshape(-1, 12)

        entry = {}
        results = []
        for name, resident in (("resident", 256), ("swept", 0)):
            if name == "resident" and n > 256:
                continue
            call(resident)                                                     # warm-up: module load, scratch
            ms, poses = min((call(resident) for _ in range(3)), key=lambda r: r[0])
            results.append(poses)
            entry[name + "_ms"] = round(ms, 3)
            entry[name + "_us_per_round"] = round(ms * 1e3 / max(rounds, 1), 3)
            entry[name + "_ns_per_edge_round"] = round(ms * 1e6 / max(rounds, 1) / len(A["row_edges"]), 3)
        H = P.batch([one])
        t0 = time.perf_counter()
        h = P.relax(H, P.settings(rounds))
        sec = time.perf_counter() - t0
        entry["host_one_graph_ms"] = round(sec * 1e3, 3)
        entry["host_ns_per_edge_round"] = round(sec * 1e9 / max(rounds, 1) / len(H["row_edges"]), 3)
        entry["bit_equal"] = bool(all(r[:n].tobytes() == h["poses"].tobytes() and r.tobytes() == results[0].tobytes() for r in results))
        ok = ok and entry["bit_equal"]
        res["sizes"][str(n)] = entry
    print(json.dumps(res))
    cons.close()
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, nargs="+", default=[16, 64, 256, 1024])
    ap.add_argument("--graphs", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=1024)
    ap.add_argument("--step", action="store_true", help="run in this process (the default starts a child under `timeout`)")
    a = ap.parse_args()
    if a.step:
        return step(a.views, a.graphs, a.rounds)
    cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--step", "--graphs", str(a.graphs), "--rounds", str(a.rounds),
           "--views"] + [str(v) for v in a.views]
    print("#", " ".join(cmd), flush=True)
    return subprocess.run(cmd).returncode


if __name__ == "__main__":
    sys.exit(main())
