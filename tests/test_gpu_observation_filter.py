"""The observation-filter kernels (cv_amd/csrc/rs_observation_filter.hip) and the optimize_reconstruction chain against the host
builds of the same headers (tests/observation_filter_checker.py, tests/pose_graph_checker.py): every output array is compared
in bytes, WHOLE — what a call does not write keeps the pattern it was filled with on both sides, so the rows behind the valid
ones are held untouched by the same comparison.  Run with -m gpu.

The scan: a tile is 1 024 observations (kOfTile), one workgroup scans the tile sums 256 at a time with a carry, so there is no
third level; the second pass of that loop starts at 256 tiles = 262 144 observations, which one scene here passes."""
import ctypes as C

import numpy as np
import pytest

import observation_filter_checker as F
import pose_graph_checker as P
import triangulate_checker as T

pytestmark = pytest.mark.gpu

TILE = 1024
OUT8 = ("keep", "state", "reason", "robust")
OUT32 = ("start_out", "obs_out", "split_out", "counts", "verdict", "stats")


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


def rs_camera(cam):
    from cv_amd import _lib
    return _lib.Camera(cam.fx, cam.fy, cam.cx, cam.cy, cam.skew, cam.k1, cam.use_k1, 0)


def device_filter(torch, cons, sc, recon_start, view_start, skip=None, n_obs=None, params=None, obs=None, start=None):
    """rs_filter_observations_device on the arrays of a scene -> dict of the output buffers as the host checker shapes them"""
    from cv_amd import _lib
    from cv_amd.reconstruction import ObservationFilter
    dev = torch.device("cuda", 0)
    up = lambda a: _lib.device_bytes(torch, a, dev)
    obs = sc["obs"] if obs is None else obs
    start = sc["start"] if start is None else start
    n_lm, n_rec = len(start) - 1, len(recon_start) - 1
    n_obs = len(obs) if n_obs is None else n_obs
    room = max(n_obs, 1)
    kps = sc["kps"]
    d_kps, d_poses, d_start, d_obs = up(kps.view(np.uint8)), up(sc["poses"]), up(start), up(obs)
    d_rs, d_vs = up(np.asarray(recon_start, np.uint32)), up(np.asarray(view_start, np.uint32))
    d_skip = None if skip is None else up(np.asarray(skip, np.uint32))
    fill = lambda n: torch.full((n,), F.FILL8, dtype=torch.uint8, device=dev)
    size = dict(keep=room, state=max(n_lm, 1), reason=max(n_lm, 1), robust=max(n_lm, 1), start_out=4 * (n_lm + 1), obs_out=8 * room,
                split_out=8 * room, counts=8, verdict=4 * max(n_rec, 1), stats=4 * F.STATS * max(n_rec, 1))
    d = {k: fill(n) for k, n in size.items()}
    ObservationFilter(cons).filter_device(
        d_kps.data_ptr(), kps.shape[1], kps.shape[0], d_poses.data_ptr(), rs_camera(sc["cam"]), d_start.data_ptr(), d_obs.data_ptr(), n_obs,
        n_lm, d_rs.data_ptr(), d_vs.data_ptr(), n_rec, None if d_skip is None else d_skip.data_ptr(), params or ObservationFilter.params(),
        d["keep"].data_ptr(), d["state"].data_ptr(), d["reason"].data_ptr(), d["robust"].data_ptr(), d["start_out"].data_ptr(),
        d["obs_out"].data_ptr(), d["split_out"].data_ptr(), d["counts"].data_ptr(), d["verdict"].data_ptr(), d["stats"].data_ptr(),
        _lib.wait_handle(torch.cuda.current_stream(dev)))
    cons.sync()
    out = {k: d[k].cpu().numpy() for k in OUT8}
    out.update({k: d[k].cpu().numpy().view(np.uint32) for k in OUT32})
    out["obs_out"], out["split_out"], out["stats"] = out["obs_out"].reshape(-1, 2), out["split_out"].reshape(-1, 2), out["stats"].reshape(-1, F.STATS)
    return out


def assert_same(got, want):
    for k in OUT8 + OUT32:
        if not np.array_equal(got[k], want[k]):
            bad = np.flatnonzero((got[k] != want[k]).reshape(len(want[k]), -1).any(1))
            raise AssertionError((k, len(bad), bad[:10], got[k][bad[:4]], want[k][bad[:4]]))


def check(torch, cons, sc, recon_start, view_start, skip=None, n_obs=None, obs=None, start=None, **kw):
    """device == host build in every byte of every output buffer -> the host result"""
    from cv_amd.reconstruction import ObservationFilter
    obs = sc["obs"] if obs is None else obs
    start = sc["start"] if start is None else start
    tri = {k: kw.pop(k) for k in ("max_sweeps",) if k in kw}
    prm = ObservationFilter.params(**kw)
    for k, v in tri.items():
        setattr(prm.triangulate, k, v)
    got = device_filter(torch, cons, sc, recon_start, view_start, skip, n_obs, prm, obs, start)
    want = F.filter_table(sc["kps"], sc["poses"], sc["cam"], start, obs, recon_start, view_start, F.settings(**kw, **tri), skip=skip, n_obs=n_obs)
    assert_same(got, want)
    return want


def one(n_lm, n_views=12):
    return np.array([0, n_lm], np.uint32), np.array([0, n_views], np.uint32)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_landmark_counts_around_a_wave_and_a_workgroup(gpu, cons, n):
    sc = F.scene(100 + n, n_landmarks=n, lengths=(0, 8))
    h = check(gpu, cons, sc, *one(n), minimum_robust_landmarks=1)
    assert h["stats"][0, F.S_LANDMARKS] == n


def special_scene(seed, n_landmarks=3000):
    """48 ordinary views, lists of 0 to 8 mixed inside every wave and 40 lists of 33 to 48, plus view 48 with a NaN pose (the
    triangulator's reason 4) and view 49, a camera that looks the other way (reason 5), each added to 60 lists of 3 or more;
    40 bad indices."""
    sc = F.scene(seed, n_views=48, n_landmarks=n_landmarks, lengths=(0, 8), long_lists=40)
    rng = np.random.default_rng(seed + 1)
    cap = sc["kps"].shape[1]
    kps = np.concatenate([sc["kps"], np.zeros((2, cap), F.KP_DTYPE)])
    poses = np.concatenate([sc["poses"], np.zeros((2, 12))])
    poses[48] = poses[0]
    poses[48, 7] = np.nan
    back = np.hstack([np.diag([-1.0, 1.0, -1.0]), np.array([[0.0], [0.0], [1.0]])])
    poses[49] = back.reshape(12)
    start, obs = sc["start"], sc["obs"]
    lists = [obs[start[l]:start[l + 1]].tolist() for l in range(n_landmarks)]
    lens = np.diff(start.astype(np.int64))
    pick = rng.choice(np.flatnonzero(lens >= 3), 160, replace=False)
    for k, l in enumerate(pick[:60]):
        kps[48, k]["x"], kps[48, k]["y"] = 900.0, 500.0
        lists[l].insert(int(rng.integers(0, len(lists[l]) + 1)), [48, k])
    for k, l in enumerate(pick[60:120]):
        kps[49, k]["x"], kps[49, k]["y"] = T.project(back, sc["points"][l], 1000.0, 960.0, 540.0)
        lists[l].append([49, k])
    for k, l in enumerate(pick[120:160]):                      # a block == n_blocks, a feature == cap
        lists[l][k % len(lists[l])] = [50, 0] if k % 2 else [0, cap]
    sc = dict(sc, kps=kps, poses=poses, start=np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.uint32),
              obs=np.array([o for l in lists for o in l], np.uint32).reshape(-1, 2))
    return sc, pick[120:160]


def test_every_state_and_every_reason_in_one_table(gpu, cons):
    sc, bad = special_scene(0x0F17)
    n = len(sc["start"]) - 1
    # three reconstructions whose boundaries fall inside a wave; the last 101 landmarks belong to none
    rs, vs = np.array([0, 1001, 2099, 2899], np.uint32), np.array([0, 50, 50, 50], np.uint32)
    h = check(gpu, cons, sc, rs, vs)
    states, reasons = np.bincount(h["state"][:n], minlength=7), np.bincount(h["reason"][:n], minlength=256)
    print("states 0..6:", states.tolist(), "reasons 0, 4, 5, 6, 255:", reasons[[0, 4, 5, 6, 255]].tolist(), "stats", h["stats"][:3].tolist())
    assert (states > 0).all() and (reasons[[0, 4, 5, 6, 255]] > 0).all() and reasons[[1, 2, 3]].sum() == 0
    in_recon = bad[bad < 2899]
    assert states[F.BAD_INDEX] == len(in_recon) == reasons[6] and np.all(h["state"][in_recon] == F.BAD_INDEX)
    assert np.all(h["state"][2899:n] == F.SKIPPED) and list(h["verdict"][:3]) == [F.OK, F.OK, F.OK]
    lens = np.diff(sc["start"].astype(np.int64))
    assert (lens[h["state"][:n] == F.KICKED] > 32).any() and lens.max() >= 48
    # bad indices leave their neighbours' decisions as they are in the table without them
    for l in in_recon[:10]:
        assert np.all(h["keep"][sc["start"][l]:sc["start"][l + 1]] == 1) and h["robust"][l] == 0
    # the eigen-solver's own failure (reason 3): a sweep limit of 1 on a prefix of the table
    m = 300
    h3 = check(gpu, cons, sc, *one(m, 50), n_obs=int(sc["start"][m]), start=sc["start"][:m + 1], obs=sc["obs"][:sc["start"][m]], max_sweeps=1)
    assert (h3["reason"][:m] == 3).sum() > 20 and np.all(h3["state"][:m][h3["reason"][:m] == 3] == F.NO_POINT)


def pairs_scene(seed, n_obs, outlier_fraction=0.3):
    """n_obs observations in lists of two (and one of one when n_obs is odd): cheap for the host, and every flag is a decision.
    Built with array operations (F.scene walks the landmarks one by one): 12 views, the second observation of outlier_fraction
    of the pairs displaced by 40 to 120 px."""
    rng = np.random.default_rng(seed)
    n, f, cx, cy = n_obs // 2, 1000.0, 960.0, 540.0
    poses = T.random_poses(rng, 12)
    pts = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(2, 10, n)], 1)
    va = rng.integers(0, 12, n)
    view = np.stack([va, (va + rng.integers(1, 12, n)) % 12], 1).reshape(-1)                # [2n]: a, b, a, b, ...
    q = np.einsum("nij,nj->ni", poses[view][:, :, :3], np.repeat(pts, 2, 0)) + poses[view][:, :, 3]
    xy = f * q[:, :2] / q[:, 2:3] + [cx, cy] + rng.uniform(-0.5, 0.5, (2 * n, 2))
    off = (rng.random(n) < outlier_fraction) * rng.uniform(40.0, 120.0, n)
    ang = rng.uniform(0, 2 * np.pi, n)
    xy[1::2] += np.stack([off * np.cos(ang), off * np.sin(ang)], 1)
    order = np.argsort(view, kind="stable")
    feature = np.empty(2 * n, np.int64)
    first = np.searchsorted(view[order], np.arange(12))
    feature[order] = np.arange(2 * n) - first[view[order]]
    kps = np.zeros((12, max(int(feature.max()) + 1 if n else 1, 1)), F.KP_DTYPE)
    kps["x"][view, feature], kps["y"][view, feature] = xy[:, 0], xy[:, 1]
    start, obs = 2 * np.arange(n + 1, dtype=np.uint32), np.stack([view, feature], 1).astype(np.uint32)
    if n_obs % 2:
        start, obs = np.append(start, np.uint32(n_obs)), np.concatenate([obs, np.array([[0, 0]], np.uint32)])
    return dict(kps=kps, poses=poses.reshape(12, 12), cam=F.camera(f, f, cx, cy), start=start, obs=obs)


@pytest.mark.parametrize("n_obs", [TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1])
def test_the_scan_around_one_and_two_tiles(gpu, cons, n_obs):
    sc = pairs_scene(n_obs, n_obs)
    h = check(gpu, cons, sc, *one(len(sc["start"]) - 1), minimum_robust_landmarks=0, maximum_sine_distance=1e-2)
    assert h["counts"].sum() == n_obs and h["counts"][1] > 50


def test_the_scan_of_the_tile_sums_takes_a_second_pass(gpu, cons):
    """more than 256 tiles: the one workgroup of k_of_scan_sums goes round its loop twice and carries"""
    n_obs = 256 * TILE + 3 * TILE + 5
    sc = pairs_scene(77, n_obs)
    h = check(gpu, cons, sc, *one(len(sc["start"]) - 1), maximum_sine_distance=1e-2)
    assert h["counts"].sum() == n_obs and h["counts"][1] > 10000 and h["start_out"][-1] == h["counts"][0]


def test_everything_kept_and_everything_split(gpu, cons):
    sc = F.scene(31, n_landmarks=700, lengths=(0, 8), outlier_fraction=0.0)
    n = 700
    h = check(gpu, cons, sc, *one(n), maximum_cosine_distance=1.0, maximum_sine_distance=2.0)
    assert h["counts"][1] == 0 and np.array_equal(h["obs_out"][:len(sc["obs"])], sc["obs"]) and np.array_equal(h["start_out"], sc["start"])
    assert np.all(h["split_out"] == F.FILL32)
    # a threshold nothing can meet: every list keeps one observation
    h = check(gpu, cons, sc, *one(n), maximum_cosine_distance=-1.0, maximum_sine_distance=-1.0)
    lens = np.diff(sc["start"].astype(np.int64))
    assert np.array_equal(np.diff(h["start_out"].astype(np.int64)), np.minimum(lens, 1)) and h["counts"][0] == (lens > 0).sum()
    # a capacity beyond the table's fill: the rows past d_obs_start[n_landmarks] are not the table's
    short = int(sc["start"][650])
    check(gpu, cons, sc, *one(650), start=sc["start"][:651])
    assert short < len(sc["obs"])


def test_three_reconstructions_one_rejected_by_one_landmark_one_at_the_minimum_one_skipped(gpu, cons):
    sc = F.scene(41, n_landmarks=400, lengths=(2, 8))
    rs, vs = np.array([0, 130, 270, 400], np.uint32), np.array([0, 12, 12, 12], np.uint32)
    base = F.filter_table(sc["kps"], sc["poses"], sc["cam"], sc["start"], sc["obs"], rs, vs)
    after = base["stats"][:3, F.S_ROBUST_AFTER].astype(int)
    # the minimum is set from the smaller of the two counts: one above it rejects that reconstruction by one landmark
    lo, hi = sorted(after[:2])
    assert lo < hi
    first, second = (0, 1) if after[0] < after[1] else (1, 0)
    h = check(gpu, cons, sc, rs, vs, skip=[0, 0, 1], minimum_robust_landmarks=lo + 1)
    assert h["verdict"][first] == F.FEW_LANDMARKS and h["verdict"][2] == F.RECON_SKIPPED
    assert h["stats"][first, F.S_ROBUST_AFTER] == lo and h["verdict"][second] == F.OK   # rejected by one landmark
    h = check(gpu, cons, sc, rs, vs, skip=[0, 0, 1], minimum_robust_landmarks=lo)
    assert h["verdict"][first] == F.OK and h["verdict"][second] == F.OK       # accepted at exactly the minimum
    assert np.all(h["state"][270:400] == F.SKIPPED) and h["stats"][2].tolist() == [130, 0, 0, 0, 0, 0, 0, 0]


def test_start_arrays_that_do_not_ascend_are_refused_per_reconstruction(gpu, cons):
    sc = F.scene(43, n_landmarks=300, lengths=(0, 8))
    vs = np.array([0, 12, 12, 12], np.uint32)
    h = check(gpu, cons, sc, np.array([0, 200, 100, 300], np.uint32), vs, minimum_robust_landmarks=1)
    assert list(h["verdict"][:3]) == [F.OK, F.BAD_RANGE, F.BAD_RANGE] and np.all(h["state"][200:300] == F.SKIPPED)
    h = check(gpu, cons, sc, np.array([0, 100, 200, 301], np.uint32), vs, minimum_robust_landmarks=1)
    assert list(h["verdict"][:3]) == [F.OK, F.OK, F.BAD_RANGE]
    h = check(gpu, cons, sc, np.array([0, 100, 200, 300], np.uint32), np.array([0, 12, 11, 13], np.uint32), minimum_robust_landmarks=1)
    assert list(h["verdict"][:3]) == [F.OK, F.BAD_RANGE, F.BAD_RANGE]
    start = sc["start"].copy()
    start[150], start[151] = start[151] + 1, start[150]                       # a descent inside reconstruction 1's starts
    h = check(gpu, cons, sc, np.array([0, 100, 200, 300], np.uint32), vs, start=start, minimum_robust_landmarks=1)
    assert list(h["verdict"][:3]) == [F.OK, F.BAD_RANGE, F.OK]
    start = sc["start"].copy()
    start[300] = len(sc["obs"]) + 1                                           # the last range leaves the observations
    h = check(gpu, cons, sc, np.array([0, 100, 200, 300], np.uint32), vs, start=start, minimum_robust_landmarks=1)
    assert list(h["verdict"][:3]) == [F.OK, F.OK, F.BAD_RANGE]


def test_aliased_tables_are_refused_and_nothing_is_launched(gpu, cons):
    torch = gpu
    from cv_amd import _lib
    from cv_amd.reconstruction import ObservationFilter
    sc = F.scene(45, n_landmarks=64, lengths=(0, 8))
    dev = torch.device("cuda", 0)
    up = lambda a: _lib.device_bytes(torch, a, dev)
    n_lm, n_obs = 64, len(sc["obs"])
    d_kps, d_poses, d_start, d_obs = up(sc["kps"].view(np.uint8)), up(sc["poses"]), up(sc["start"]), up(sc["obs"])
    d_rs, d_vs = up(np.array([0, n_lm], np.uint32)), up(np.array([0, 12], np.uint32))
    buf = {k: torch.full((8 * n_obs + 64,), F.FILL8, dtype=torch.uint8, device=dev) for k in ("keep", "state", "reason", "robust", "start_out", "obs_out", "split_out", "counts", "verdict", "stats")}
    L, prm, cam = _lib.lib(), ObservationFilter.params(), rs_camera(sc["cam"])

    def call(**alias):
        p = {k: alias.get(k, v.data_ptr()) for k, v in buf.items()}
        return L.rs_filter_observations_device(cons._h, d_kps.data_ptr(), sc["kps"].shape[1], 12, d_poses.data_ptr(), C.byref(cam), d_start.data_ptr(),
                                               d_obs.data_ptr(), n_obs, n_lm, d_rs.data_ptr(), d_vs.data_ptr(), 1, None, C.byref(prm), p["keep"],
                                               p["state"], p["reason"], p["robust"], p["start_out"], p["obs_out"], p["split_out"], p["counts"],
                                               p["verdict"], p["stats"], None)
    for alias in (dict(obs_out=d_obs.data_ptr()), dict(start_out=d_start.data_ptr()), dict(obs_out=d_obs.data_ptr() + 8 * (n_obs - 1)),
                  dict(split_out=d_obs.data_ptr()), dict(start_out=d_obs.data_ptr()), dict(obs_out=d_start.data_ptr() + 4)):
        assert call(**alias) == -1
    cons.sync()
    assert all((b.cpu().numpy() == F.FILL8).all() for b in buf.values())
    assert d_obs.cpu().numpy().tobytes() == sc["obs"].tobytes() and d_start.cpu().numpy().tobytes() == sc["start"].tobytes()
    assert call() == 0
    cons.sync()
    assert (buf["counts"].cpu().numpy()[:8].view(np.uint32).sum()) == n_obs


# ---- the chain ---------------------------------------------------------------------------------------------------------
def chain_scene(seed=3):
    """Four reconstructions side by side: a ring of 8 views (the resident form of the relaxation with the limit at 12) and a ring
    of 16 (the swept form) with a few hundred landmarks each; a ring of 5 with 20 landmarks, which the filter rejects in round 0
    (fewer than 32 robust); three views without a constraint (RS_PG_FEW_VIEWS) and 30 landmarks that pass through."""
    rng = np.random.default_rng(seed)
    graphs = [P.Graph(11, 8, noise=1e-3), P.Graph(12, 16, noise=1e-3), P.Graph(13, 5, noise=1e-3), P.Graph(14, 3, triples=[], noise=1e-3)]
    A = P.batch(graphs)
    counts = [300, 400, 20, 30]
    n_views, n_lm = len(A["poses"]), sum(counts)
    f, cx, cy = 1000.0, 960.0, 540.0
    kps = np.zeros((n_views, n_lm), F.KP_DTYPE)
    used = np.zeros(n_views, np.int64)
    start, obs, recon_start = [0], [], [0]
    v0 = 0
    for gr, n in zip(graphs, counts):
        for _ in range(n):
            while True:                                         # a point at least one unit in front of two views or more
                X = rng.uniform(-5.0, 5.0, 3)
                depth = gr.truth[:, 2, :3] @ X + gr.truth[:, 2, 3]
                visible = np.flatnonzero(depth > 1.0)
                if len(visible) >= 2:
                    break
            views = rng.permutation(visible)[:rng.integers(2, min(len(visible), 7) + 1)]
            bad = rng.integers(0, len(views)) if rng.random() < 0.2 else -1
            for k, v in enumerate(views):
                q = gr.truth[v][:, :3] @ X + gr.truth[v][:, 3]
                x, y = f * q[0] / q[2] + cx + rng.uniform(-0.5, 0.5), f * q[1] / q[2] + cy + rng.uniform(-0.5, 0.5)
                if k == bad:
                    x += rng.uniform(40, 120)
                b = v0 + int(v)
                kps[b, used[b]]["x"], kps[b, used[b]]["y"] = x, y
                obs.append((b, used[b]))
                used[b] += 1
            start.append(len(obs))
        v0 += gr.n
        recon_start.append(len(start) - 1)
    return dict(A=A, kps=kps, cam=F.camera(f, f, cx, cy), start=np.array(start, np.uint32), obs=np.array(obs, np.uint32).reshape(-1, 2),
                recon_start=np.array(recon_start, np.uint32))


def chain_host(cs, iterations, rounds, minimum=32):
    """the host builds of the pose-graph header and of the filter header run in sequence, as the call chains them"""
    A = dict(cs["A"])
    n_g = len(A["graph_start"]) - 1
    stop, verdict = np.zeros(n_g, np.uint32), np.zeros(n_g, np.uint32)
    pg = dict(poses=A["poses"].copy(), verdict=np.full(n_g, F.FILL32, np.uint32), state=np.full(len(A["poses"]), F.FILL32, np.uint32),
              stats=np.full((n_g, P.STATS), F.FILL32, np.uint32))
    start, obs, n_obs = cs["start"], cs["obs"], len(cs["obs"])
    per_round = []
    for r in range(rounds):
        new = P.relax(dict(A, poses=pg["poses"]), P.settings(iterations))
        for g in range(n_g):                                    # a stopped graph is not run: nothing of it is written
            if stop[g]:
                continue
            a, b = int(A["graph_start"][g]), int(A["graph_start"][g + 1])
            pg["poses"][a:b], pg["state"][a:b] = new["poses"][a:b], new["state"][a:b]
            pg["verdict"][g], pg["stats"][g] = new["verdict"][g], new["stats"][g]
        F.note(pg["verdict"], P.OK, r, F.OR_STAGE_RELAX, stop, verdict)
        o = F.filter_table(cs["kps"], pg["poses"], cs["cam"], start, obs if len(obs) == n_obs else np.concatenate([obs, np.zeros((n_obs - len(obs), 2), np.uint32)]),
                           cs["recon_start"], A["graph_start"], F.settings(minimum_robust_landmarks=minimum), skip=stop.copy(), n_obs=n_obs)
        F.note(o["verdict"], F.OK, r, F.OR_STAGE_FILTER, stop, verdict)
        per_round.append(o)
        start, obs = o["start_out"], o["obs_out"][:o["counts"][0]]
    return dict(pg=pg, verdict=verdict, rounds=per_round, start=start, obs=obs)


def test_the_chain_equals_the_host_builds_run_in_sequence(gpu, cons):
    torch = gpu
    from cv_amd import _lib, triangulation
    from cv_amd.pose_graph import PoseGraph
    from cv_amd.reconstruction import ObservationFilter, ReconstructionOptimizer
    cs = chain_scene()
    A, rounds, iterations = cs["A"], 2, 16
    want = chain_host(cs, iterations, rounds)
    stops = [(int(v) >> 16 & 0xFF, int(v) >> 8 & 0xFF, int(v) & 0xFF) if v else None for v in want["verdict"]]
    assert stops == [None, None, (0, F.OR_STAGE_FILTER, F.FEW_LANDMARKS), (0, F.OR_STAGE_RELAX, P.FEW_VIEWS)]
    assert want["rounds"][1]["verdict"][2] == F.RECON_SKIPPED and want["rounds"][1]["verdict"][3] == F.RECON_SKIPPED
    assert want["rounds"][0]["counts"][1] > 50 and list(want["rounds"][1]["verdict"][:2]) == [F.OK, F.OK]

    dev = torch.device("cuda", 0)
    up = lambda a: _lib.device_bytes(torch, a, dev)
    n_views, n_g, n_c = len(A["poses"]), len(A["graph_start"]) - 1, len(A["views"])
    n_lm, n_obs = len(cs["start"]) - 1, len(cs["obs"])
    d_poses, d_gs, d_rs, d_re, d_views, d_cverdict, d_edges = (up(A[k]) for k in ("poses", "graph_start", "row_start", "row_edges", "views", "cverdict", "edges"))
    d_kps, d_start, d_obs, d_recon = up(cs["kps"].view(np.uint8)), up(cs["start"]), up(cs["obs"]), up(cs["recon_start"])
    fill = lambda n: torch.full((n,), F.FILL8, dtype=torch.uint8, device=dev)
    size = dict(verdict=4 * n_g, gv=4 * n_g, state=4 * n_views, pg_stats=4 * P.STATS * n_g, keep=n_obs, lm_state=n_lm, reason=n_lm, robust=n_lm,
                start_out=4 * (n_lm + 1), obs_out=8 * n_obs, split_out=8 * n_obs * rounds, counts=8 * rounds, rv=4 * n_g * rounds,
                of_stats=4 * F.STATS * n_g * rounds, world=32 * n_lm, world_reason=n_lm)
    d = {k: fill(n) for k, n in size.items()}
    pg = PoseGraph(cons)
    opt = ReconstructionOptimizer(pg)
    prm = ObservationFilter.params(reconstruction_optimization_iterations=rounds)
    cam = rs_camera(cs["cam"])
    pg.resident_views(12)
    try:
        opt.optimize_device(d_poses.data_ptr(), n_views, d_gs.data_ptr(), n_g, d_rs.data_ptr(), d_re.data_ptr(), len(A["row_edges"]), d_views.data_ptr(),
                            d_cverdict.data_ptr(), d_edges.data_ptr(), n_c, PoseGraph.params(optimization_iterations=iterations), d_kps.data_ptr(),
                            cs["kps"].shape[1], cam, d_start.data_ptr(), d_obs.data_ptr(), n_obs, n_lm, d_recon.data_ptr(), prm,
                            *(d[k].data_ptr() for k in ("verdict", "gv", "state", "pg_stats", "keep", "lm_state", "reason", "robust", "start_out",
                                                        "obs_out", "split_out", "counts", "rv", "of_stats", "world", "world_reason")),
                            _lib.wait_handle(torch.cuda.current_stream(dev)))
        cons.sync()
    finally:
        pg.resident_views()
    g32 = lambda k: d[k].cpu().numpy().view(np.uint32)
    assert g32("verdict").tolist() == want["verdict"].tolist()
    assert d_poses.cpu().numpy().tobytes() == want["pg"]["poses"].tobytes()
    assert g32("gv").tolist() == want["pg"]["verdict"].tolist() and np.array_equal(g32("state"), want["pg"]["state"])
    assert np.array_equal(g32("pg_stats").reshape(n_g, P.STATS), want["pg"]["stats"])
    last = want["rounds"][-1]
    for k, hk in (("keep", "keep"), ("lm_state", "state"), ("reason", "reason"), ("robust", "robust")):
        assert np.array_equal(d[k].cpu().numpy(), last[hk]), k
    assert np.array_equal(g32("start_out"), last["start_out"]) and np.array_equal(g32("obs_out").reshape(-1, 2), last["obs_out"])
    for r, o in enumerate(want["rounds"]):
        assert np.array_equal(g32("split_out").reshape(rounds, n_obs, 2)[r], o["split_out"]), r
        assert np.array_equal(g32("counts").reshape(rounds, 2)[r], o["counts"]) and np.array_equal(g32("rv").reshape(rounds, n_g)[r], o["verdict"])
        assert np.array_equal(g32("of_stats").reshape(rounds, n_g, F.STATS)[r], o["stats"]), r
    # d_world is rs_triangulate_landmarks_device on the final table
    table = triangulation.LandmarkTable.from_device(torch, d["start_out"].view(torch.int32), d["obs_out"].view(torch.int32).reshape(-1, 2), n_lm, n_obs)
    d_w, d_r = fill(32 * n_lm), fill(n_lm)
    triangulation.triangulate_landmarks_device(cons._h, table, d_kps, cs["kps"].shape[1], n_views, d_poses, cam, prm.triangulate, d_w, d_r)
    cons.sync()
    assert d_w.cpu().numpy().tobytes() == d["world"].cpu().numpy().tobytes() and d_r.cpu().numpy().tobytes() == d["world_reason"].cpu().numpy().tobytes()
    hw, hr = T.landmarks(cs["kps"], want["pg"]["poses"], cs["cam"], last["start_out"], last["obs_out"], n_obs=n_obs)
    assert d["world"].cpu().numpy().tobytes() == hw.tobytes() and np.array_equal(d["world_reason"].cpu().numpy(), hr)
    assert (hr == 0).sum() > 300


def test_the_python_mirror_runs_the_chain(gpu, cons):
    """ObservationFilter.run and ReconstructionOptimizer.run give what the raw calls give"""
    torch = gpu
    from cv_amd import _lib, triangulation
    from cv_amd.pose_graph import PoseGraph
    from cv_amd.reconstruction import ObservationFilter, ReconstructionOptimizer, stopped_at
    cs = chain_scene()
    A = cs["A"]
    want = chain_host(cs, 16, 2)
    dev = torch.device("cuda", 0)
    d_kps = _lib.device_bytes(torch, cs["kps"].view(np.uint8), dev)
    table = triangulation.LandmarkTable(torch, start=cs["start"], obs=cs["obs"])
    pg = PoseGraph(cons)
    d_poses = torch.from_numpy(A["poses"].copy()).to(dev)
    res = ObservationFilter(cons).run(torch, table, d_kps, cs["kps"].shape[1], len(A["poses"]), d_poses, rs_camera(cs["cam"]), cs["recon_start"],
                                      A["graph_start"])
    ref = F.filter_table(cs["kps"], A["poses"], cs["cam"], cs["start"], cs["obs"], cs["recon_start"], A["graph_start"])
    assert np.array_equal(res.keep, ref["keep"]) and np.array_equal(res.obs_start, ref["start_out"]) and np.array_equal(res.verdicts, ref["verdict"][:4])
    assert np.array_equal(res.obs, ref["obs_out"][:ref["counts"][0]]) and np.array_equal(res.split, ref["split_out"][:ref["counts"][1]])
    edges = pg.edges(torch, A["views"], (A["cposes"], A["cverdict"]))
    pg.resident_views(12)
    try:
        out = ReconstructionOptimizer(pg).run(torch, d_poses, A["graph_start"], A["row_start"], A["row_edges"], edges, table, d_kps, cs["kps"].shape[1],
                                              rs_camera(cs["cam"]), cs["recon_start"], PoseGraph.params(optimization_iterations=16),
                                              ObservationFilter.params(reconstruction_optimization_iterations=2))
    finally:
        pg.resident_views()
    assert out.verdicts.tolist() == want["verdict"].tolist() and [stopped_at(v) for v in out.verdicts][2:] == [(0, "filter", 1), (0, "relax", 1)]
    assert d_poses.cpu().numpy().tobytes() == want["pg"]["poses"].tobytes()
    assert np.array_equal(out.filter.obs_start, want["rounds"][-1]["start_out"]) and np.array_equal(out.filter.obs, want["obs"])
    assert np.array_equal(out.filter.split, want["rounds"][-1]["split_out"][:want["rounds"][-1]["counts"][1]])
    assert out.world.shape == (len(cs["start"]) - 1, 4)


def test_the_native_mirror_gives_the_same_table(gpu, cons, tmp_path):
    """cv_sfm::ObservationFilter of include/akaze.hpp from a process without Python (tests/cpp/observation_filter.cpp)"""
    import subprocess

    import host_build
    sc = F.scene(51, n_landmarks=150, lengths=(0, 8))
    rs, vs = np.array([0, 70, 150], np.uint32), np.array([0, 12, 12], np.uint32)
    want = F.filter_table(sc["kps"], sc["poses"], sc["cam"], sc["start"], sc["obs"], rs, vs)
    path = tmp_path / "table.bin"
    with open(path, "wb") as fp:
        fp.write(np.array([12, sc["kps"].shape[1], 150, len(sc["obs"]), 2], np.uint32).tobytes())
        fp.write(bytes(sc["cam"]))
        for a in (sc["kps"], sc["poses"], sc["start"], sc["obs"], rs, vs):
            fp.write(np.ascontiguousarray(a).tobytes())
    exe = host_build.native(tmp_path, "observation_filter.cpp", hip=True)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("observation_filter ok"), (r.returncode, r.stderr[-400:])
    rows = {line.split(" ", 1)[0]: np.array(line.split()[1:], np.int64) for line in r.stdout.splitlines()[:-1]}
    kept, split = (int(c) for c in want["counts"])
    assert np.array_equal(rows["keep"], want["keep"]) and np.array_equal(rows["states"], want["state"][:150])
    assert np.array_equal(rows["reasons"], want["reason"][:150]) and np.array_equal(rows["robust"], want["robust"][:150])
    assert np.array_equal(rows["start"], want["start_out"]) and np.array_equal(rows["obs"], want["obs_out"][:kept].reshape(-1))
    assert np.array_equal(rows["split"], want["split_out"][:split].reshape(-1)) and rows["counts"].tolist() == [kept, split]
    assert np.array_equal(rows["verdicts"], want["verdict"][:2]) and np.array_equal(rows["stats"], want["stats"][:2].reshape(-1))
