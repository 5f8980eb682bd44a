"""The pose-graph kernels (cv_amd/csrc/rs_pose_graph.hip) against the host build of the same header
(tests/pose_graph_checker.py): edges, poses, verdicts, view states and every stats word in bit patterns (the bytes are
compared).  What a call does not write keeps the pattern it was filled with, on both sides.  Run with -m gpu.

Forms: the resident form (one persistent workgroup a graph) can take RS_PG_RESIDENT_VIEWS = 256 views and by default takes
graphs of at most 8, the others go through a launch per round; PoseGraph.resident_views moves the limit, so that both forms
are tested at every size up to 256 and 257."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import host_build
import pose_graph_checker as P

pytestmark = pytest.mark.gpu

FILL = 0xA5


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cv_amd import build
    build.build()
    return torch


@pytest.fixture(scope="module")
def cons(gpu):
    from cv_amd.ransac import EssentialConsensus
    c = EssentialConsensus(64, 64)
    yield c
    c.close()


def run(torch, cons, A, st, resident=None, n_rows=None, n_constraints=None):
    """rs_pose_graph_edges_device and rs_pose_graph_relax_batch_device on the arrays of P.batch, and the host build on the
    same: everything the calls may write is compared in bytes.  `resident`: the largest graph the resident form takes (default:
    the library's own limit).
    -> the host result."""
    from cv_amd import _lib
    from cv_amd.pose_graph import PoseGraph
    dev = torch.device("cuda", 0)
    up = lambda a: _lib.device_bytes(torch, a, dev)
    n_views, n_graphs, n_c = len(A["poses"]), len(A["graph_start"]) - 1, len(A["views"])
    d_poses, d_gs, d_rs, d_re, d_views, d_cposes, d_cverdict = (up(A[k]) for k in ("poses", "graph_start", "row_start", "row_edges", "views", "cposes", "cverdict"))
    d_edges = torch.full((n_c * 72 * 8,), FILL, dtype=torch.uint8, device=dev)
    d_verdict = torch.full((n_graphs * 4,), FILL, dtype=torch.uint8, device=dev)
    d_state = torch.full((max(n_views, 1) * 4,), FILL, dtype=torch.uint8, device=dev)
    d_stats = torch.full((n_graphs * P.STATS * 4,), FILL, dtype=torch.uint8, device=dev)
    pg = PoseGraph(cons)
    wait = _lib.wait_handle(torch.cuda.current_stream(dev))
    if resident is not None:
        pg.resident_views(resident)
    try:
        pg.edges_device(d_views.data_ptr(), d_cposes.data_ptr(), d_cverdict.data_ptr(), n_c, d_edges.data_ptr(), wait)
        pg.relax_batch_device(d_poses.data_ptr(), n_views, d_gs.data_ptr(), n_graphs, d_rs.data_ptr(), d_re.data_ptr(),
                              len(A["row_edges"]) if n_rows is None else n_rows, d_views.data_ptr(), d_cverdict.data_ptr(), d_edges.data_ptr(),
                              n_c if n_constraints is None else n_constraints,
                              PoseGraph.params(optimization_iterations=st.optimization_iterations, graph_optimization_rate=st.graph_optimization_rate),
                              d_verdict.data_ptr(), d_state.data_ptr(), d_stats.data_ptr(), wait)
        cons.sync()
    finally:
        pg.resident_views()
    edges = d_edges.cpu().numpy().view(np.float64).reshape(n_c, 6, 12)
    assert edges.tobytes() == A["edges"].tobytes(), np.nonzero((edges.view(np.uint64) != A["edges"].view(np.uint64)).any((1, 2)))[0][:10]
    h = P.relax(A, st, n_rows=n_rows, n_constraints=n_constraints)
    verdict = d_verdict.cpu().numpy().view(np.uint32)
    state = d_state.cpu().numpy().view(np.uint32)[:n_views]
    stats = d_stats.cpu().numpy().view(np.uint32).reshape(n_graphs, P.STATS)
    poses = d_poses.cpu().numpy().view(np.float64).reshape(n_views, 12)
    assert verdict.tolist() == h["verdict"].tolist(), (verdict, h["verdict"], stats, h["stats"])
    assert np.array_equal(stats, h["stats"]), (stats, h["stats"])
    assert np.array_equal(state, h["state"]), np.nonzero(state != h["state"])[0][:10]
    bad = np.nonzero((poses.view(np.uint64) != h["poses"].view(np.uint64)).any(1))[0]
    assert len(bad) == 0, (len(bad), bad[:10], poses[bad[:2]], h["poses"][bad[:2]])
    return h


def small_graphs():
    """3 views with 1 constraint; 5 views with 4; a view without a constraint; a view all of whose constraints are refused"""
    return [P.Graph(1, 3, triples=[(0, 1, 2)]), P.Graph(2, 5, triples=[(0, 1, 2), (1, 2, 3), (2, 3, 4), (4, 0, 2)]), P.Graph(3, 5, triples=[(0, 1, 2), (1, 2, 3)]),
            P.Graph(4, 6, triples=[(0, 1, 2), (1, 2, 3), (2, 3, 0), (3, 4, 5), (4, 5, 0)], refused=[3, 4])]


@pytest.mark.parametrize("resident", [256, 0])
def test_small_graphs(gpu, cons, resident):
    h = run(gpu, cons, P.batch(small_graphs()), P.settings(8), resident)
    assert h["verdict"].tolist() == [P.OK] * 4
    assert h["stats"][:, :4].tolist() == [[3, 3, 6, 8], [5, 5, 24, 8], [5, 4, 12, 8], [6, 4, 18, 8]]
    assert h["state"].tolist() == [0] * 3 + [0] * 5 + [0, 0, 0, 0, 1] + [0, 0, 0, 0, 1, 1]


@pytest.mark.parametrize("resident", [256, 0])
def test_row_lengths(gpu, cons, resident):
    """rows of 1, 63, 64, 65, 128 and 129 edges: the lane stride and its tail (a row may name an edge more than once)"""
    g = P.Graph(7, 6)
    lengths = [1, 63, 64, 65, 128, 129]
    g.rows = [[row[i % len(row)] for i in range(n)] for row, n in zip(g.rows, lengths)]
    h = run(gpu, cons, P.batch([g]), P.settings(4), resident)
    assert h["verdict"].tolist() == [P.OK] and h["stats"][0].tolist() == [6, 6, sum(lengths), 4, 2, P.NO_VIEW, 0, 0]


@pytest.mark.parametrize("n", [256, 257])
def test_the_largest_resident_and_the_smallest_swept_graph(gpu, cons, n):
    h = run(gpu, cons, P.batch([P.Graph(n, n)]), P.settings(8), 256)
    assert h["verdict"].tolist() == [P.OK] and h["stats"][0, :4].tolist() == [n, n, 6 * n, 8]


def test_one_graph_through_both_forms(gpu, cons):
    A = P.batch([P.Graph(40, 40)])
    a = run(gpu, cons, A, P.settings(16), 256)
    b = run(gpu, cons, A, P.settings(16), 39)          # one view more than the resident form takes now
    assert a["poses"].tobytes() == b["poses"].tobytes() and a["poses"].tobytes() != A["poses"].tobytes()


@pytest.mark.parametrize("rounds", [0, 1, 2, 3, 64])
def test_rounds(gpu, cons, rounds):
    """the parity of the ping-pong, in both forms: 12 views resident, 20 swept"""
    A = P.batch([P.Graph(12, 12), P.Graph(20, 20)])
    h = run(gpu, cons, A, P.settings(rounds), 16)
    assert h["verdict"].tolist() == [P.OK, P.OK] and h["stats"][:, P.S_ROUNDS].tolist() == [rounds, rounds]
    assert (h["poses"].tobytes() == A["poses"].tobytes()) == (rounds == 0)


@pytest.mark.parametrize("n", [1, 2, 17])
def test_batches(gpu, cons, n):
    """graphs of both forms side by side (the limit at 16 views: one swept graph alone, a swept and a resident one, and 17 with
    one graph beyond 256 and one refused)"""
    sizes = [30, 9, 3, 16, 17, 5, 260, 8, 12, 40, 3, 6, 25, 4, 16, 7, 33]
    graphs = [P.Graph(100 + i, s) for i, s in enumerate(sizes[:n])]
    if n > 2:
        graphs[2] = P.Graph(102, sizes[2], triples=[(0, 1, 2)], refused=[0])       # no view would be updated
    h = run(gpu, cons, P.batch(graphs), P.settings(5), 16)
    assert h["verdict"].tolist() == [P.FEW_VIEWS if i == 2 else P.OK for i in range(n)]


@pytest.mark.parametrize("n", [8, 9])
def test_the_default_limit(gpu, cons, n):
    """at the library's own limit between the forms (the result does not show which form ran: the bits are equal)"""
    h = run(gpu, cons, P.batch([P.Graph(50 + n, n), P.Graph(60 + n, 3)]), P.settings(7))
    assert h["verdict"].tolist() == [P.OK, P.OK] and h["stats"][:, P.S_ROUNDS].tolist() == [7, 7]


def test_each_bad_index_refuses_its_own_graph_only(gpu, cons):
    graphs = [P.Graph(200 + i, 6) for i in range(6)]
    good = run(gpu, cons, P.batch(graphs), P.settings(4))
    assert good["verdict"].tolist() == [P.OK] * 6
    # graph 2: constraint 1 = views (1, 2, 3) of it gets a view of graph 3 as its third.  The two edges whose TARGET is that
    # third view (slots 4, 5) leave the rows, so every remaining entry's target is still its row's view and the only thing
    # wrong is the OTHER view of slots 0 and 3
    outside = P.Graph(202, 6)
    assert outside.views[1].tolist() == [1, 2, 3] and {6 + 4, 6 + 5} <= set(outside.rows[3])
    outside.rows[3] = [e for e in outside.rows[3] if e not in (6 + 4, 6 + 5)]
    A = P.batch(graphs[:2] + [outside] + graphs[3:])
    rs, gs = A["row_start"], A["graph_start"]
    A["row_edges"][rs[gs[0] + 2] + 1] = 6 * len(A["views"])            # graph 0: an entry >= 6 n_constraints
    A["row_edges"][rs[gs[1] + 3]] = A["row_edges"][rs[gs[1] + 4]]       # graph 1: an entry whose target is another view
    A["views"][6 * 2 + 1, 2] = gs[3]
    for v in range(int(gs[2]), int(gs[3])):                             # (every target of graph 2's rows still matches)
        assert all(A["views"][e // 6, P.SLOT_TARGET[e % 6]] == v for e in A["row_edges"][rs[v]:rs[v + 1]])
    rs[gs[3] + 2] = rs[gs[3] + 3] + 1                                   # graph 3: a row that runs backwards
    h = run(gpu, cons, A, P.settings(4), n_rows=len(A["row_edges"]) - 1)   # graph 5: its last row leaves [0, n_rows]
    assert h["verdict"].tolist() == [P.BAD_INDEX] * 4 + [P.OK, P.BAD_INDEX]
    assert h["poses"][gs[4]:gs[5]].tobytes() == good["poses"][gs[4]:gs[5]].tobytes()
    for g in (0, 1, 2, 3, 5):
        assert h["poses"][gs[g]:gs[g + 1]].tobytes() == A["poses"][gs[g]:gs[g + 1]].tobytes() and np.all(h["state"][gs[g]:gs[g + 1]] == P.FILL32)
        assert h["stats"][g].tolist() == [0, 0, 0, 0, 0, P.NO_VIEW, 0, 0]
    # the graph ranges: one that runs backwards, one that leaves [0, n_views]
    for last in (int(gs[5]) - 1, int(gs[6]) + 1):
        B = P.batch(graphs)
        B["graph_start"][6] = last
        h = run(gpu, cons, B, P.settings(4))
        assert h["verdict"].tolist() == [P.OK] * 5 + [P.BAD_INDEX] and h["poses"][:gs[5]].tobytes() == good["poses"][:gs[5]].tobytes()
    # a start array that runs backwards in the middle: graph 1 = [6, 4) is refused, and so is graph 2 = [4, 18), which begins
    # below a start in front of it and would share views 4 and 5 with graph 0 — graph 0 itself is untouched by either
    B = P.batch(graphs)
    B["graph_start"][2] = 4
    h = run(gpu, cons, B, P.settings(4))
    assert h["verdict"].tolist() == [P.OK, P.BAD_INDEX, P.BAD_INDEX, P.OK, P.OK, P.OK]
    assert h["poses"][:6].tobytes() == good["poses"][:6].tobytes() and h["poses"][18:].tobytes() == good["poses"][18:].tobytes()
    assert h["poses"][6:18].tobytes() == B["poses"][6:18].tobytes() and np.all(h["state"][6:18] == P.FILL32)
    # fewer constraints than the rows name
    h = run(gpu, cons, P.batch(graphs), P.settings(4), n_constraints=len(A["views"]) - 1)
    assert h["verdict"].tolist() == [P.OK] * 5 + [P.BAD_INDEX]


@pytest.mark.parametrize("resident", [256, 4])
def test_a_pose_that_is_not_finite(gpu, cons, resident):
    """a NaN in one view's pose: RS_PG_NONFINITE at round 0 for its graph, the other graphs of the batch as without it"""
    graphs = [P.Graph(300, 6), P.Graph(301, 8), P.Graph(302, 5)]
    good = run(gpu, cons, P.batch(graphs), P.settings(6), resident)
    A = P.batch(graphs)
    A["poses"][6 + 3, 5] = np.nan                      # view 3 of the ring of 8: views 1 - 5 share a constraint with it
    h = run(gpu, cons, A, P.settings(6), resident)
    assert h["verdict"].tolist() == [P.OK, P.NONFINITE, P.OK]
    assert h["stats"][1].tolist() == [8, 8, 48, 1, 2, 6 + 1, 0, 0]
    assert h["state"][6:14].tolist() == [0, 2, 2, 2, 2, 2, 0, 0]
    assert h["poses"][7:12].tobytes() == A["poses"][7:12].tobytes()                 # not finite: as they were
    assert np.all((h["poses"][[6, 12, 13]] != A["poses"][[6, 12, 13]]).any(1))             # the finite views' updates are installed
    for lo, hi in ((0, 6), (14, 19)):
        assert h["poses"][lo:hi].tobytes() == good["poses"][lo:hi].tobytes()


def test_the_parameters_are_checked_with_a_live_context(gpu, cons):
    """a struct_size that is off and a rate that is not finite are refused although everything else is in order, and nothing
    is written: poses, verdicts, view states and stats keep their bytes"""
    from cv_amd import _lib
    from cv_amd.pose_graph import PoseGraph
    torch = gpu
    A = P.batch([P.Graph(400, 6)])
    dev = torch.device("cuda", 0)
    up = lambda a: _lib.device_bytes(torch, a, dev)
    d = {k: up(A[k]) for k in ("poses", "graph_start", "row_start", "row_edges", "views", "cverdict", "edges")}
    d_out = torch.full((4 * (1 + P.STATS + 6),), FILL, dtype=torch.uint8, device=dev)
    L = _lib.lib()

    def call(prm):
        return L.rs_pose_graph_relax_batch_device(cons._h, d["poses"].data_ptr(), 6, d["graph_start"].data_ptr(), 1, d["row_start"].data_ptr(),
                                                  d["row_edges"].data_ptr(), len(A["row_edges"]), d["views"].data_ptr(),
                                                  d["cverdict"].data_ptr(), d["edges"].data_ptr(), len(A["views"]), prm,
                                                  d_out.data_ptr(), d_out.data_ptr() + 4, d_out.data_ptr() + 4 * 7, None)

    small = PoseGraph.params(optimization_iterations=3)
    small.struct_size -= 4
    bad = [small] + [PoseGraph.params(optimization_iterations=3, graph_optimization_rate=r) for r in (float("nan"), float("inf"), float("-inf"))]
    for prm in bad:
        assert call(C.byref(prm)) == -1          # AKZ_E_INVALID
    assert call(None) == -1
    cons.sync()
    assert d["poses"].cpu().numpy().tobytes() == A["poses"].tobytes() and np.all(d_out.cpu().numpy() == FILL)
    # the same call with parameters in order runs
    assert call(C.byref(PoseGraph.params(optimization_iterations=3))) == 0
    cons.sync()
    out = d_out.cpu().numpy().view(np.uint32)
    h = P.relax(A, P.settings(3))
    assert out[0] == P.OK and out[1:7].tolist() == [0] * 6 and out[7:].tolist() == h["stats"][0].tolist()
    assert d["poses"].cpu().numpy().tobytes() == h["poses"].tobytes()


def test_the_chain_stays_on_the_device(gpu, cons):
    """ThreeViewConstraints.run_tensors -> PoseGraph.edges -> PoseGraph.relax -> triangulate_landmarks_device on torch tensors,
    no host copy between them, against the same chain through the host builds.  Two tiny scenes of
    three_view_constraint_checker, patience 8, 4 rounds; a graph of 3 views and 1 constraint each."""
    import three_view_constraint_checker as T
    import triangulate_checker as tc
    from cv_amd import _lib, triangulation
    from cv_amd.pose_graph import PoseGraph, flatten
    from cv_amd.three_view import ThreeViewConstraints
    torch = gpu
    cap = 160
    scenes = [T.scene(501, 140), T.scene(502, 140)]
    kps, poses, views, lm_start, lm = T.device_arrays(scenes, cap, [(0, np.arange(64)), (1, np.arange(64))])
    st = T.settings(constraint_patience=8)
    lists = [[(3 * k + v, i) for v in range(3)] for k in range(2) for i in range(0, 140, 7)]
    start = np.arange(len(lists) + 1, dtype=np.uint32) * 3
    obs = np.array(lists, np.uint32).reshape(-1, 2)
    graph_start = np.array([0, 3, 6], np.uint32)
    row_start, row_edges = flatten(views, 6)
    # ---- the host builds ----
    hc = [T.constraint_scene(kps, poses, T.K.rig_camera(), views, lm_start, lm, s, st) for s in range(2)]
    assert [h["verdict"] for h in hc] == [T.OK, T.OK]
    A = dict(poses=poses.copy(), graph_start=graph_start, row_start=row_start, row_edges=row_edges, views=views,
             cverdict=np.array([h["verdict"] for h in hc], np.uint32), cposes=np.stack([h["pose_out"] for h in hc]))
    A["edges"] = P.edges(A["cposes"], A["cverdict"])
    hr = P.relax(A, P.settings(4))
    assert hr["verdict"].tolist() == [P.OK, P.OK] and hr["poses"].tobytes() != poses.tobytes()
    want, want_r = tc.landmarks(kps, hr["poses"], T.K.rig_camera(), start, obs)
    assert np.count_nonzero(want_r == 0) > len(lists) // 2
    # ---- the device ----
    dev = torch.device("cuda", 0)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)
    cam = _lib.Camera(T.K.CAM["fx"], T.K.CAM["fy"], T.K.CAM["cx"], T.K.CAM["cy"], 0.0, 0.0, 0, 0)
    d_kps, d_poses, d_views = t(kps, np.uint8).reshape(len(kps), cap, 28), t(poses, np.float64), t(views, np.int32)
    d_verdict, d_cposes, _ = ThreeViewConstraints(cons).run_tensors(torch, d_kps, d_poses, cam, d_views, t(lm_start, np.int32), t(lm, np.int32),
                                                                    ThreeViewConstraints.params(constraint_patience=8))
    pg = PoseGraph(cons)
    edges = pg.edges(torch, d_views, (d_cposes, d_verdict))
    res = pg.relax(torch, d_poses, t(graph_start, np.int32), t(row_start, np.int32), t(row_edges, np.int32), edges,
                   PoseGraph.params(optimization_iterations=4))
    table = triangulation.LandmarkTable(torch, start=start, obs=obs)
    d_world = table.new_world()
    d_reason = torch.full((len(lists),), 99, dtype=torch.uint8, device=dev)
    triangulation.triangulate_landmarks_device(cons._h, table, d_kps, cap, len(kps), d_poses, cam, triangulation.make_params(), d_world, d_reason)
    cons.sync()
    assert res.verdicts.tolist() == [P.OK, P.OK] and res.rounds(0) == 4 and res.view_states.tolist() == [0] * 6
    assert np.array_equal(res.stats, hr["stats"])
    assert d_poses.cpu().numpy().tobytes() == hr["poses"].tobytes()
    assert edges[0].cpu().numpy().tobytes() == A["edges"].tobytes()
    assert np.array_equal(d_reason.cpu().numpy(), want_r) and d_world.cpu().numpy().tobytes() == want.tobytes()
    # numpy arrays in: the same result, the caller's array left alone
    res2 = pg.relax(torch, poses, graph_start, row_start, row_edges, pg.edges(torch, views, (A["cposes"], A["cverdict"])),
                    PoseGraph.params(optimization_iterations=4))
    assert res2.poses.tobytes() == hr["poses"].tobytes() and res2.verdicts.tolist() == [P.OK, P.OK]


def test_a_torch_stream_object_is_waited_for(gpu, cons):
    """The case cv_amd/_device.py exists for: the producer runs on the current torch stream — the legacy default stream, whose
    handle is 0, which the ABI reads as "nothing to wait for" — and rows_device gets the tensors themselves and the stream
    OBJECT.  A few milliseconds of matmuls keep the stream busy in front of an asynchronous copy of views [64][3] from pinned
    memory; nothing waits on the host.  A call that did not wait would read the zeros the tensor held before, which are valid
    view indices: a wrong answer, never a fault."""
    from cv_amd import _device, _lib
    from cv_amd.pose_graph import PoseGraph, flatten
    torch = gpu
    dev = torch.device("cuda", 0)
    n, n_views = 64, 16
    views = np.random.default_rng(0x57A3).integers(0, n_views, (n, 3)).astype(np.int32)
    pinned = torch.from_numpy(views).pin_memory()
    a = torch.ones((2048, 2048), dtype=torch.float32, device=dev)
    d_views = torch.zeros((n, 3), dtype=torch.int32, device=dev)
    d_row_start = torch.zeros((n_views + 1,), dtype=torch.int32, device=dev)
    d_row_edges = torch.zeros((6 * n,), dtype=torch.int32, device=dev)
    d_flags = torch.zeros((1,), dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)                        # the zeros are there: from here on nothing waits on the host
    cur = torch.cuda.current_stream(dev)
    assert _device.wait(cur) == _lib.STREAM_LEGACY or cur.cuda_stream != 0
    for _ in range(8):
        a = (a @ a) * (1.0 / 2048)
    d_views.copy_(pinned, non_blocking=True)
    PoseGraph(cons).rows_device(d_views, n, n_views, d_row_start, d_row_edges, d_flags, stream_to_wait=cur)
    cons.sync()
    row_start, row_edges = flatten(views, n_views)
    assert np.array_equal(d_row_start.cpu().numpy().view(np.uint32), row_start)
    assert np.array_equal(d_row_edges.cpu().numpy().view(np.uint32), row_edges)
    assert int(d_flags.cpu()[0]) == 0


def test_cpp_host_mirror_pose_graph(gpu, cons, tmp_path):
    """cv_sfm::PoseGraph of include/akaze.hpp from a native process (tests/cpp/pose_graph.cpp): its flatten and its printed
    verdicts, states, stats and poses equal the ctypes path's."""
    exe = host_build.native(tmp_path, "pose_graph.cpp", hip=True)
    A = P.batch(small_graphs() + [P.Graph(9, 4, triples=[(0, 1, 2)], refused=[0])])
    rounds = 7
    with open(tmp_path / "batch.bin", "wb") as f:
        f.write(np.array([len(A["poses"]), len(A["graph_start"]) - 1, len(A["views"]), rounds], np.uint32).tobytes())
        for k in ("poses", "graph_start", "views", "cverdict", "cposes"):
            f.write(np.ascontiguousarray(A[k]).tobytes())
    r = subprocess.run([str(exe), str(tmp_path / "batch.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "pose_graph ok" in r.stdout
    h = run(gpu, cons, A, P.settings(rounds))
    lines = dict(l.split(" ", 1) for l in r.stdout.strip().splitlines() if " " in l)
    assert [int(x) for x in lines["rows"].split()] == A["row_edges"].tolist()
    assert [int(x) for x in lines["verdicts"].split()] == h["verdict"].tolist() == [0, 0, 0, 0, 1]
    assert [int(x) for x in lines["stats"].split()] == h["stats"].reshape(-1).tolist()
    assert [int(x) for x in lines["states"].split()] == h["state"].tolist()
    assert lines["poses"].split() == [f"{int(u):016x}" for u in h["poses"].view(np.uint64).reshape(-1)]
