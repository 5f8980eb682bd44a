"""The covisibility kernels (cv_amd/csrc/rs_covisibility.hip) against the host build of the same header
(tests/covisibility_checker.py): every output buffer is compared in bytes, WHOLE — both sides start from the same fill pattern,
so a word a call should have written and did not shows.  Run with -m gpu.

Shapes: a workgroup is 256 threads and compacts a target's features 256 at a time, a bit row is 64 features per word, the
candidate views are compacted 256 blocks at a time, the scan over the targets takes a second pass beyond 256 targets."""
import numpy as np
import pytest

import covisibility_checker as K
import covisibility_statement as S

pytestmark = pytest.mark.gpu

SMALL = dict(min_cov=1, min_lm=1, min_new=1)
NAMES = ("views", "lm_start", "lm", "slot_count", "verdict", "stats")


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


def cv_params(p):
    from cv_amd.covisibility import Covisibility
    return Covisibility.params(optimization_robust_covisibility_minimum_landmarks=p["min_cov"],
                               optimization_maximum_three_view_constraints=p["max_constraints"], optimization_minimum_new_constraints=p["min_new"],
                               optimization_minimum_landmarks=p["min_lm"], optimization_maximum_landmarks=p["max_lm"],
                               candidate_limit=p["limit"], shuffle_seed=p["seed"])


def device_candidates(torch, cons, table, targets, p):
    """rs_covisibility_candidates_device on a table -> dict of the output buffers as the host checker shapes them"""
    from cv_amd import _lib
    from cv_amd.covisibility import Covisibility
    dev = torch.device("cuda", 0)
    up = lambda a: _lib.device_bytes(torch, a, dev)
    targets = np.asarray(targets, np.uint32)
    d_start, d_obs, d_reason, d_targets = up(table["start"]), up(table["obs"]), up(table["reason"]), up(targets)
    want = K.outputs(len(targets), p)
    d = {k: torch.full((want[k].nbytes,), K.FILL8, dtype=torch.uint8, device=dev) for k in NAMES}
    Covisibility(cons).candidates_device(d_start.data_ptr(), d_obs.data_ptr(), len(table["obs"]), len(table["start"]) - 1, table["cap"],
                                         table["n_blocks"], d_reason.data_ptr(), d_targets.data_ptr(), len(targets), cv_params(p),
                                         *(d[k].data_ptr() for k in NAMES), _lib.wait_handle(torch.cuda.current_stream(dev)))
    cons.sync()
    return {k: d[k].cpu().numpy().view(np.uint32).reshape(want[k].shape) for k in NAMES}


def check(torch, cons, table, targets, p):
    """device == host build in every byte of every output buffer -> the host result"""
    got = device_candidates(torch, cons, table, targets, p)
    want = K.candidates(table, targets, p)
    for k in NAMES:
        if not np.array_equal(got[k], want[k]):
            bad = np.flatnonzero((got[k] != want[k]).reshape(len(want[k]), -1).any(1))
            raise AssertionError((k, len(bad), bad[:10], got[k][bad[:4]], want[k][bad[:4]]))
    return want


@pytest.mark.parametrize("robust", [1, 63, 64, 65, 129])
def test_robust_features_around_a_word_of_a_bit_row(gpu, cons, robust):
    tab = K.star_table(4, [robust, robust, max(robust - 1, 1), robust], robust, 100 if robust <= 100 else 131)
    h = check(gpu, cons, tab, [0], S.settings(limit=8, seed=5, **SMALL))
    assert h["stats"][0, K.S_ROBUST] == robust and h["slot_count"][0] == robust and h["stats"][0, K.S_EMITTED] == 6


@pytest.mark.parametrize("n", [0, 1, 2, 3, 64, 65, K.MAX_CANDIDATE_VIEWS, K.MAX_CANDIDATE_VIEWS + 1])
def test_candidate_views_up_to_the_cap_and_one_beyond(gpu, cons, n):
    per = [3 + (k % 4) for k in range(n)]
    tab = K.star_table(n, per, 6, 100, target=min(1, n), extra_blocks=2)
    h = check(gpu, cons, tab, [min(1, n)], S.settings(limit=K.MAX_SLOTS, max_constraints=K.MAX_SLOTS, **SMALL))
    assert h["stats"][0, K.S_CANDIDATES] == min(n, K.MAX_CANDIDATE_VIEWS)
    assert bool(h["stats"][0, K.S_FLAGS] & K.F_CAPPED) == (n > K.MAX_CANDIDATE_VIEWS)
    assert h["stats"][0, K.S_EMITTED] == min(n * (n - 1) // 2, K.MAX_SLOTS)


def test_more_blocks_than_a_workgroup_compacts_at_once(gpu, cons):
    # 300 blocks, the candidates on both sides of block 256
    n = 299
    per = [4 if k in (3, 200, 254, 255, 256, 257, 298) else 0 for k in range(n)]
    tab = K.star_table(n, per, 5, 16)
    h = check(gpu, cons, tab, [0, 257], S.settings(limit=32, **SMALL))
    assert h["stats"][0, K.S_CANDIDATES] == 7 and h["stats"][1, K.S_CANDIDATES] == 7


@pytest.mark.parametrize("targets", [[4], [0, 7, 7, 99, 3]])
@pytest.mark.parametrize("kw", [dict(limit=1), dict(limit=8), dict(seed=9), dict(max_constraints=2, limit=6)])
def test_random_tables(gpu, cons, targets, kw):
    tab = K.random_table(11)
    h = check(gpu, cons, tab, targets, S.settings(**kw))
    assert h["stats"][0, K.S_EMITTED] > 0
    if len(targets) > 1:
        assert h["verdict"].tolist() == [K.OK, K.OK, K.OK, K.BAD_INDEX, K.OK]
        lim = S.settings(**kw)["limit"]
        assert np.array_equal(h["views"][lim:2 * lim], h["views"][2 * lim:3 * lim])          # the repeated target


def test_the_scan_over_the_targets_takes_a_second_pass(gpu, cons):
    tab = K.random_table(12)
    targets = (list(range(12)) * 26)[:300]
    h = check(gpu, cons, tab, targets, S.settings(limit=2))
    assert (h["stats"][:, K.S_EMITTED] == 2).all() and h["lm_start"][-1] >= 300 * 2 * 24 and len(h["lm_start"]) == 601


def test_a_cap_that_is_no_multiple_of_64_and_scattered_features(gpu, cons):
    tab = K.random_table(13, cap=200)
    check(gpu, cons, tab, list(range(12)), S.settings(limit=K.MAX_SLOTS, max_constraints=K.MAX_SLOTS))


def test_bad_tables_refuse_and_read_nothing_out_of_bounds(gpu, cons):
    tab = K.random_table(14, n_landmarks=120)
    tab["obs"][5] = (12, 0)                                   # a block == n_blocks
    tab["obs"][40] = (tab["obs"][40][0], tab["cap"])          # a feature == cap
    h = check(gpu, cons, tab, list(range(12)), S.settings(limit=4))
    assert K.BAD_INDEX in h["verdict"].tolist() and K.OK in h["verdict"].tolist()
    tab = K.random_table(14, n_landmarks=120)
    tab["start"][7] = tab["start"][6] - 1                     # a start that descends: everyone is refused
    h = check(gpu, cons, tab, [0, 1], S.settings(limit=4))
    assert h["verdict"].tolist() == [K.BAD_INDEX] * 2


def test_record_and_rows(gpu, cons):
    torch = gpu
    from cv_amd import _lib
    from cv_amd.covisibility import Covisibility
    from cv_amd.pose_graph import PoseGraph, flatten
    dev = torch.device("cuda", 0)
    up = lambda a: _lib.device_bytes(torch, a, dev)
    rng = np.random.default_rng(3)
    p = S.settings(limit=6, min_new=4, max_constraints=5)
    n_targets = 300
    targets = rng.integers(0, 40, n_targets).astype(np.uint32)
    gs = np.array([0, 3, 8, 8, 30], np.uint32)
    cv = rng.choice([0, 0, 0, 1, 2, 3], n_targets * 6).astype(np.uint32)
    tv = rng.choice([K.OK, K.OK, K.OK, K.BAD_INDEX], n_targets).astype(np.uint32)
    stats = rng.integers(0, 50, (n_targets, K.STATS)).astype(np.uint32)
    want = K.record(cv, targets, tv, stats, gs, p)
    assert set(want[1].tolist()) == {K.OK, K.FEW_CONSTRAINTS, K.BAD_INDEX, K.NO_GRAPH}
    d_rec = torch.full((4 * len(cv),), K.FILL8, dtype=torch.uint8, device=dev)
    d_tv, d_stats, d_cv, d_targets, d_gs = up(tv), up(stats), up(cv), up(targets), up(gs)
    Covisibility(cons).record_device(d_cv.data_ptr(), d_targets.data_ptr(), n_targets, d_gs.data_ptr(), len(gs) - 1, cv_params(p),
                                     d_rec.data_ptr(), d_tv.data_ptr(), d_stats.data_ptr(), _lib.wait_handle(torch.cuda.current_stream(dev)))
    cons.sync()
    for got, w in zip((d_rec, d_tv, d_stats), want):
        assert got.cpu().numpy().tobytes() == w.tobytes()
    # rows: more views than one pass of the scan, an unused slot, a triple outside; then MOST slots unused — all their entries
    # in view 0's row — at one chunk of the sort's keys (2 048), several chunks, and more keys than a power of two holds
    for n, n_views, bad, unused in ((1, 3, False, 0.0), (700, 300, False, 0.0), (50, 9, True, 0.0), (341, 12, False, 0.8), (3000, 40, False, 0.8),
                                    (45000, 300, True, 0.9)):
        views = np.sort(np.stack([rng.permutation(n_views)[:3] for _ in range(n)]), 1).astype(np.uint32)
        if n > 2:
            views[1] = 0
        views[rng.random(n) < unused] = 0
        if bad:
            views[7, 2] = n_views
        rs, re, flag = K.rows(views, n_views)
        d_views = up(views)
        d_rs, d_re, d_flag = (torch.full((4 * k,), K.FILL8, dtype=torch.uint8, device=dev) for k in (n_views + 1, 6 * n, 1))
        PoseGraph(cons).rows_device(d_views.data_ptr(), n, n_views, d_rs.data_ptr(), d_re.data_ptr(), d_flag.data_ptr(),
                                    _lib.wait_handle(torch.cuda.current_stream(dev)))
        cons.sync()
        assert d_rs.cpu().numpy().tobytes() == rs.tobytes() and d_re.cpu().numpy().tobytes() == re.tobytes()
        assert d_flag.cpu().numpy().view(np.uint32)[0] == flag == int(bad)
        if not bad:
            fs, fe = flatten(views, n_views)
            assert rs.tolist() == fs.tolist() and re.tolist() == fe.tolist()


def test_regenerate_equals_the_chain_driven_from_the_host(gpu, cons):
    """candidates -> constraints -> record -> edges -> rows -> optimize_reconstruction on the device, against the same chain with
    the lists from the host build, the record on the host and the rows from flatten: equal bytes in the relaxed poses, the
    verdicts and the world table."""
    torch = gpu
    import observation_filter_checker as F
    from cv_amd import _lib, triangulation
    from cv_amd.covisibility import Covisibility
    from cv_amd.pose_graph import PoseGraph, flatten
    from cv_amd.reconstruction import ObservationFilter, ReconstructionOptimizer, regenerate
    from cv_amd.three_view import ThreeViewConstraints
    sc = F.scene(21, n_views=12, n_landmarks=320, lengths=(3, 8), outlier_fraction=0.1)
    n_views, cap, n_lm = 12, sc["kps"].shape[1], len(sc["start"]) - 1
    dev = torch.device("cuda", 0)
    up = lambda a: _lib.device_bytes(torch, a, dev)
    c = sc["cam"]
    cam = _lib.Camera(c.fx, c.fy, c.cx, c.cy, c.skew, c.k1, c.use_k1, 0)
    d_kps = up(sc["kps"].view(np.uint8))
    table = triangulation.LandmarkTable(torch, start=sc["start"], obs=sc["obs"])
    graph_start, recon_start = np.array([0, n_views], np.uint32), np.array([0, n_lm], np.uint32)
    p = S.settings(limit=12)
    cvp, tvcp = cv_params(p), ThreeViewConstraints.params(constraint_patience=8)
    pgp, ofp = PoseGraph.params(optimization_iterations=16), ObservationFilter.params(minimum_robust_landmarks=8)
    ofp.triangulate.n_views = n_views
    # the reason bytes both chains read
    d_pose0 = torch.from_numpy(sc["poses"].copy()).to(dev)
    d_reason = torch.zeros((n_lm,), dtype=torch.uint8, device=dev)
    d_world0 = table.new_world()
    triangulation.triangulate_landmarks_device(cons._h, table, d_kps, cap, n_views, d_pose0, cam, ofp.triangulate, d_world0, d_reason,
                                               _lib.wait_handle(torch.cuda.current_stream(dev)))
    cons.sync()
    reason = d_reason.cpu().numpy()
    assert (reason == 0).sum() > 200
    # on the device
    d_poses = d_pose0.clone()
    r = regenerate(torch, cons, table, d_kps, cap, cam, d_poses, graph_start, recon_start, reason=d_reason, cv_params=cvp, tvc_params=tvcp,
                   pg_params=pgp, params=ofp)
    # from the host
    tab = dict(start=sc["start"], obs=sc["obs"], reason=reason, n_blocks=n_views, cap=cap)
    targets = np.arange(n_views, dtype=np.uint32)
    h = K.candidates(tab, targets, p)
    assert h["stats"][:, K.S_EMITTED].sum() > 20
    for k, got in (("views", r.candidates.views), ("lm_start", r.candidates.lm_start), ("lm", r.candidates.lm), ("slot_count", r.candidates.slot_count)):
        assert got.cpu().numpy().tobytes() == h[k].tobytes(), k
    d_poses2 = d_pose0.clone()
    as_i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).to(dev)
    d_views, d_lm_start, d_lm = as_i32(h["views"]), as_i32(h["lm_start"]), as_i32(h["lm"])
    cver, cpose, cstats = ThreeViewConstraints(cons).run_tensors(torch, d_kps.reshape(n_views, cap, 28), d_poses2, cam, d_views, d_lm_start, d_lm, tvcp)
    cons.sync()
    ver = cver.cpu().numpy().view(np.uint32)
    assert (ver == 0).sum() > 10
    recorded, tver, tstats = K.record(ver, targets, h["verdict"], h["stats"], graph_start, p)
    assert r.recorded.cpu().numpy().tobytes() == recorded.tobytes()
    assert r.candidates.target_verdict.cpu().numpy().tobytes() == tver.tobytes() and r.candidates.stats.cpu().numpy().tobytes() == tstats.tobytes()
    pg = PoseGraph(cons)
    edges = pg.edges(torch, d_views, (cpose, as_i32(recorded)))
    row_start, row_edges = flatten(h["views"], n_views)
    assert r.rows[0].cpu().numpy().tobytes() == row_start.tobytes() and r.rows[1].cpu().numpy().tobytes() == row_edges.tobytes()
    out = ReconstructionOptimizer(pg).run(torch, d_poses2, graph_start, row_start, row_edges, edges, table, d_kps, cap, cam, recon_start, pgp, ofp)
    assert r.verdict.cpu().numpy().view(np.uint32)[:1].tolist() == out.verdicts.tolist()
    assert d_poses.cpu().numpy().tobytes() == d_poses2.cpu().numpy().tobytes()
    assert not np.array_equal(d_poses.cpu().numpy(), sc["poses"])                             # the relaxation moved them
    assert r.pose_graph[0].cpu().numpy().view(np.uint32)[:1].tolist() == out.pose_graph.verdicts.tolist()
    assert r.world.cpu().numpy().tobytes() == out.world.cpu().numpy().tobytes()
    assert r.world_reason.cpu().numpy().tobytes() == out.world_reason.cpu().numpy().tobytes()
    assert r.filter.recon_verdict.cpu().numpy().tobytes() == out.tensors.recon_verdict.cpu().numpy().tobytes()
    # regenerate with the reason bytes left to it: it triangulates under the same poses first, and everything after is the same
    d_poses3 = d_pose0.clone()
    q = regenerate(torch, cons, table, d_kps, cap, cam, d_poses3, graph_start, recon_start, cv_params=cvp, tvc_params=tvcp, pg_params=pgp, params=ofp)
    assert d_poses3.cpu().numpy().tobytes() == d_poses.cpu().numpy().tobytes()
    for a, b in ((q.candidates.views, r.candidates.views), (q.candidates.lm, r.candidates.lm), (q.candidates.targets, r.candidates.targets),
                 (q.recorded, r.recorded), (q.rows[1], r.rows[1]), (q.verdict, r.verdict), (q.world, r.world), (q.world_reason, r.world_reason)):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def test_the_native_mirror_gives_the_same_candidates_and_rows(gpu, cons, tmp_path):
    """cv_sfm::ViewConstraints and cv_sfm::PoseGraph::rows of include/akaze.hpp from a process without Python
    (tests/cpp/covisibility.cpp): every array it prints against the host build"""
    import subprocess
    import host_build
    from cv_amd import _lib
    tab = K.random_table(15)
    targets = np.array([0, 5, 5, 40, 11], np.uint32)
    p = S.settings(limit=5, seed=3)
    path = tmp_path / "table.bin"
    with open(path, "wb") as f:
        f.write(np.array([tab["n_blocks"], tab["cap"], len(tab["start"]) - 1, len(tab["obs"]), len(targets)], np.uint32).tobytes())
        f.write(bytes(cv_params(p)))
        for a in (tab["start"], np.ascontiguousarray(tab["obs"], np.uint32), tab["reason"], targets):
            f.write(a.tobytes())
    exe = host_build.native(tmp_path, "covisibility.cpp", hip=True)
    run = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stderr
    lines = run.stdout.strip().split("\n")
    assert lines[-1] == "covisibility ok"
    got = {l.split()[0]: np.array(l.split()[1:], np.uint32) for l in lines[:-1]}
    h = K.candidates(tab, targets, p)
    rs, re, flag = K.rows(h["views"], tab["n_blocks"])
    assert h["verdict"].tolist() == [K.OK, K.OK, K.OK, K.BAD_INDEX, K.OK] and h["stats"][:, K.S_EMITTED].sum() > 10
    want = dict(views=h["views"], lm_start=h["lm_start"], lm=h["lm"][:h["lm_start"][-1]], counts=h["slot_count"], verdicts=h["verdict"],
                stats=h["stats"], row_start=rs, row_edges=re, flags=np.array([flag], np.uint32))
    assert set(got) == set(want)
    for k, w in want.items():
        assert np.array_equal(got[k], np.asarray(w).reshape(-1)), k
