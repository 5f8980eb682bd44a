"""The triangulation kernels (cv_amd/csrc/rs_triangulate.hip) against the host build of the same header
(tests/triangulate_checker.py), bit for bit, and the registration loop closed on the device: poses and observation lists in,
registered poses out, the world table never on the host."""
import ctypes as C

import numpy as np
import pytest

import host_build
import triangulate_checker as tc

pytestmark = pytest.mark.gpu

CAM = (1000.0, 1000.0, 960.0, 540.0, 0.0, None)


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cv_amd import build
    build.build()
    return torch


def _dev(torch, a, view=None):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(view) if view is not None else a).to(torch.device("cuda", 0))


def _kps_dev(torch, kps):
    return _dev(torch, kps.view(np.uint8).reshape(kps.shape + (28,)))


def big_map(rng):
    """50 000 landmarks with every reachable reason among them: 64 ordinary blocks, block 64 with a NaN pose (reason 4),
    block 65 a camera that looks the other way (reason 5: the point lies behind it); points 1e5 units away (reason 2 through
    the full pair search), lists of 0 / 1 (reason 1) and 2 (reason 2) observations, 200 lists of 33..48 observations."""
    nb, cap, nl = 66, 16384, 50000
    kps, poses, start, obs, pts = tc.synthetic_map(rng, 64, cap, nl, max_len=32, long_lists=200)
    kps = np.concatenate([kps, np.zeros((2, cap), tc.KP_DTYPE)])
    poses = np.concatenate([poses, np.zeros((2, 12))])
    poses[64] = poses[0]; poses[64, 7] = np.nan
    back = np.hstack([np.diag([-1.0, 1.0, -1.0]), np.array([[0.0], [0.0], [1.0]])])       # centre (0, 0, 1), looking down -z
    poses[65] = back.reshape(12)
    lens = np.diff(start.astype(np.int64))
    lists = [obs[start[l]:start[l + 1]].tolist() for l in range(nl)]
    cand = np.nonzero(lens >= 3)[0]
    pick = rng.choice(cand, 900, replace=False)
    used = [0, 0]
    for l in pick[:300]:                                   # an observation from the NaN block
        kps[64, used[0]]["x"], kps[64, used[0]]["y"] = 900.0, 500.0
        lists[l].insert(int(rng.integers(0, len(lists[l]) + 1)), [64, used[0]]); used[0] += 1
    for l in pick[300:600]:                                # an observation from the camera behind
        x, y = tc.project(back, pts[l], 1000.0, 960.0, 540.0)
        kps[65, used[1]]["x"], kps[65, used[1]]["y"] = x, y
        lists[l].append([65, used[1]]); used[1] += 1
    for l in pick[600:900]:                                # far away: no pair has the parallax
        far = pts[l] * 1e5 / pts[l][2]
        for b, j in lists[l]:
            kps[b, j]["x"], kps[b, j]["y"] = tc.project(poses[b].reshape(3, 4), far, 1000.0, 960.0, 540.0)
    start = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.uint32)
    obs = np.array([o for l in lists for o in l], np.uint32).reshape(-1, 2)
    return kps, poses, start, obs


def test_landmark_table_equals_the_host_build_bit_for_bit(gpu):
    """rs_triangulate_landmarks_device == the host build of include/akz_triangulate_math.h in bit patterns and reason bytes:
    50 000 landmarks, list lengths 0-32 mixed inside every wave, 200 lists longer than 32, reasons 0, 1, 2, 4, 5 and — with a
    sweep limit of 1 — 3, bad indices (reason 6, neighbouring rows untouched), n_landmarks of 1, 63, 64, 65."""
    torch = gpu
    from cv_amd import _lib, triangulation
    from cv_amd.ransac import EssentialConsensus
    rng = np.random.default_rng(0x7121)
    kps, poses, start, obs = big_map(rng)
    nl, (nb, cap) = len(start) - 1, kps.shape
    # bad indices: a block == n_blocks, a feature == cap
    lens = np.diff(start.astype(np.int64))
    bad = rng.choice(np.nonzero(lens >= 2)[0], 40, replace=False)
    for k, l in enumerate(bad):
        obs[start[l] + (k % lens[l])] = (nb, 0) if k % 2 else (0, cap)
    cam = tc.camera(*CAM[:5])
    want, want_r = tc.landmarks(kps, poses, cam, start, obs)
    hist = np.bincount(want_r, minlength=7)
    print("reasons 0..6:", hist.tolist(), " list lengths: max", lens.max(), "mean %.1f" % lens.mean())
    assert (hist[[0, 1, 2, 4, 5, 6]] > 0).all() and hist[3] == 0 and hist[0] > 0.6 * nl and hist[6] == 40
    cons = EssentialConsensus(8, 1)
    rcam = cons.camera(CAM)
    table = triangulation.LandmarkTable(torch, start=start, obs=obs)
    d_kps, d_poses = _kps_dev(torch, kps), _dev(torch, poses)
    d_world = torch.full((nl + 3, 4), 7.25, dtype=torch.float64, device=d_kps.device)
    d_reason = torch.full((nl + 3,), 99, dtype=torch.uint8, device=d_kps.device)
    torch.cuda.synchronize()
    prm = triangulation.make_params()
    triangulation.triangulate_landmarks_device(cons._h, table, d_kps, cap, nb, d_poses, rcam, prm, d_world, d_reason)
    cons.sync()
    got, got_r = d_world.cpu().numpy(), d_reason.cpu().numpy()
    assert np.array_equal(got_r[:nl], want_r), np.nonzero(got_r[:nl] != want_r)[0][:10]
    diff = np.nonzero((got[:nl].view(np.uint64) != want.view(np.uint64)).any(1))[0]
    assert len(diff) == 0, (len(diff), diff[:10], got[diff[:3]], want[diff[:3]])
    assert (got[nl:] == 7.25).all() and (got_r[nl:] == 99).all()
    none = want_r != 0
    assert (got[:nl][none] == tc.NONE).all() and (got[:nl][~none, 3] >= 0).all()
    # prefixes of the table: 1, 63, 64, 65 landmarks — the rows behind stay as they were; and without a reason array
    L = _lib.lib()
    for n in (1, 63, 64, 65):
        d_w = torch.full((70, 4), 7.25, dtype=torch.float64, device=d_kps.device)
        _lib.check(L.rs_triangulate_landmarks_device(cons._h, d_kps.data_ptr(), cap, nb, d_poses.data_ptr(), C.byref(rcam),
                                                     table.d_start.data_ptr(), table.d_obs.data_ptr(), int(start[n]), n, C.byref(prm),
                                                     d_w.data_ptr(), None, None), "prefix")
        cons.sync()
        g = d_w.cpu().numpy()
        assert g[:n].tobytes() == want[:n].tobytes() and (g[n:] == 7.25).all(), n
    # a sweep limit of 1: reason 3 wherever the full run found a point or failed after the solve
    n3 = 65
    st1, prm1 = tc.settings(max_sweeps=1), triangulation.make_params(max_iterations=1)
    w3, r3 = tc.landmarks(kps, poses, cam, start[:n3 + 1], obs[:start[n3]], st=st1)
    assert (r3 == 3).sum() > 20
    d_w = torch.zeros((n3, 4), dtype=torch.float64, device=d_kps.device)
    d_r = torch.zeros((n3,), dtype=torch.uint8, device=d_kps.device)
    _lib.check(L.rs_triangulate_landmarks_device(cons._h, d_kps.data_ptr(), cap, nb, d_poses.data_ptr(), C.byref(rcam),
                                                 table.d_start.data_ptr(), table.d_obs.data_ptr(), int(start[n3]), n3, C.byref(prm1),
                                                 d_w.data_ptr(), d_r.data_ptr(), None), "sweeps")
    cons.sync()
    assert d_w.cpu().numpy().tobytes() == w3.tobytes() and np.array_equal(d_r.cpu().numpy(), r3)
    # a CSR range that leaves the observation array: reason 6 for the landmarks it touches, nothing read
    n_obs_short = int(start[n3]) - 1
    w6, r6 = tc.landmarks(kps, poses, cam, start[:n3 + 1], obs, n_obs=n_obs_short)
    _lib.check(L.rs_triangulate_landmarks_device(cons._h, d_kps.data_ptr(), cap, nb, d_poses.data_ptr(), C.byref(rcam),
                                                 table.d_start.data_ptr(), table.d_obs.data_ptr(), n_obs_short, n3, C.byref(prm),
                                                 d_w.data_ptr(), d_r.data_ptr(), None), "short")
    cons.sync()
    assert d_w.cpu().numpy().tobytes() == w6.tobytes() and np.array_equal(d_r.cpu().numpy(), r6) and r6[-1] in (6, 1)
    cons.close()


def test_merged_rows_land_where_the_registration_chain_reads_them(gpu):
    """rs_triangulate_merged_device: row n_world + f * cap + j for decision == 2 && merge_ok, the list = best0's observations
    then best1's; every other row of a poisoned table keeps its bytes.  Equal to the host build bit for bit."""
    torch = gpu
    from cv_amd import triangulation
    from cv_amd.ransac import EssentialConsensus
    rng = np.random.default_rng(0x3E6)
    nb, cap, nl, F = 16, 2048, 3000, 3
    kps, poses, start, obs, _ = tc.synthetic_map(rng, nb, cap, nl, max_len=6)
    best = rng.integers(0, nl, (F, cap, 3, 2)).astype(np.uint32)
    best[rng.random((F, cap)) < 0.05, 1, 0] = 0xFFFFFFFF          # no second landmark
    best[rng.random((F, cap)) < 0.02, 0, 0] = nl                  # a key outside the table
    dec = rng.integers(0, 3, (F, cap)).astype(np.uint32)
    ok = (rng.random((F, cap)) < 0.6).astype(np.uint8)
    n_world = nl + 5
    want = np.full((n_world + F * cap, 4), 7.25)
    cam = tc.camera(*CAM[:5])
    want_r = tc.merged(kps, poses, cam, start, obs, best, dec, ok, n_world, want)
    written = (dec == 2) & (ok != 0)
    assert np.array_equal(want_r != 255, written) and (want[:n_world] == 7.25).all()
    hist = np.bincount(want_r[written], minlength=7)
    print("merged rows:", int(written.sum()), "reasons 0..6:", hist.tolist())
    assert hist[0] > 100 and hist[2] > 0 and hist[6] > 0
    cons = EssentialConsensus(8, 1)
    table = triangulation.LandmarkTable(torch, start=start, obs=obs)
    d_kps, d_poses = _kps_dev(torch, kps), _dev(torch, poses)
    d_world = torch.full((n_world + F * cap, 4), 7.25, dtype=torch.float64, device=d_kps.device)
    d_reason = torch.full((F, cap), 255, dtype=torch.uint8, device=d_kps.device)
    d_best, d_dec, d_ok = _dev(torch, best, np.int32), _dev(torch, dec, np.int32), _dev(torch, ok)
    torch.cuda.synchronize()
    triangulation.triangulate_merged_device(cons._h, table, d_kps, cap, nb, d_poses, cons.camera(CAM), triangulation.make_params(),
                                            d_best, d_dec, d_ok, F, n_world, d_world, d_reason)
    cons.sync()
    assert np.array_equal(d_reason.cpu().numpy(), want_r)
    assert d_world.cpu().numpy().tobytes() == want.tobytes()
    cons.close()


def _np_residual_from_point(pose, a, b, p):
    """0.5 * ((1 - a . p^) + (1 - b . (T p)^)) (cv-core/src/pose.rs:291-292) from a returned CameraPoint."""
    q = pose[:, :3] @ p[:3] + pose[:, 3] * p[3]
    return 0.5 * ((1.0 - a @ p[:3]) + (1.0 - b @ (q / np.linalg.norm(q))))


def _check_pairs_batch(torch, cons, kps_a, kps_b, pairs, npairs, ia, ib, cam_a, cam_b, thr, n_hyp, seed, expect_models):
    from cv_amd import triangulation
    S, cap = pairs.shape[0], pairs.shape[1]
    dev = torch.device("cuda", 0)
    d_ka, d_kb = _kps_dev(torch, kps_a), _kps_dev(torch, kps_b)
    d_pairs, d_np = _dev(torch, pairs, np.int32), _dev(torch, npairs, np.int32)
    d_pose = torch.zeros((S, 12), dtype=torch.float64, device=dev)
    d_best = torch.zeros((S,), dtype=torch.int32, device=dev)
    d_inl = torch.zeros((S, cap), dtype=torch.int32, device=dev)
    d_ninl = torch.zeros((S,), dtype=torch.int32, device=dev)
    d_pts = torch.full((S, cap, 4), 7.25, dtype=torch.float64, device=dev)
    d_why = torch.full((S, cap), 255, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    prm = cons.make_params(thr, n_hypotheses=n_hyp, seed=seed, block_size=64, init_blocks=1, max_candidates=64, halve=True)
    ca, cb = cons.camera(cam_a), cons.camera(cam_b)
    # the consensus and, behind it on the same stream, the triangulation of its inliers: no host step in between
    cons.model_inliers_batch_device(d_ka.data_ptr(), d_kb.data_ptr(), cap, ia, ib, d_pairs.data_ptr(), d_np.data_ptr(), ca, cb, prm,
                                    d_pose.data_ptr(), d_best.data_ptr(), d_inl.data_ptr(), d_ninl.data_ptr(), None, shuffle=False)
    cons.triangulate_inliers(d_ka.data_ptr(), d_kb.data_ptr(), cap, ia, ib, d_pairs.data_ptr(), d_np.data_ptr(), ca, cb,
                             d_pose.data_ptr(), d_best.data_ptr(), d_inl.data_ptr(), d_ninl.data_ptr(), d_pts.data_ptr(),
                             d_why.data_ptr(), params=triangulation.make_params())
    cons.sync()
    pose, best = d_pose.cpu().numpy(), d_best.cpu().numpy().view(np.uint32)
    inl, ninl = d_inl.cpu().numpy().view(np.uint32), d_ninl.cpu().numpy().view(np.uint32)
    pts, why = d_pts.cpu().numpy(), d_why.cpu().numpy()
    hca, hcb = tc.camera(*cam_a), tc.camera(*cam_b)
    models = compared = points = 0
    worst = 0.0
    for s in range(S):
        if best[s] == 0xFFFFFFFF:
            assert (pts[s] == 7.25).all() and (why[s] == 255).all(), s           # a scene without a model writes nothing
            continue
        models += 1
        n = int(ninl[s])
        wp, wr = tc.pairs_scene(kps_a[ia[s]], kps_b[ib[s]], pairs[s], npairs[s], hca, hcb, pose[s], inl[s, :n])
        assert np.array_equal(why[s, :n], wr) and pts[s, :n].tobytes() == wp.tobytes(), s
        assert (pts[s, n:] == 7.25).all() and (why[s, n:] == 255).all(), s
        a, b, _ = cons_scene_bearings(cons, s, cap)
        # the bearings the consensus scored are the bearings the triangulation uses: the header's calibrate statement and
        # the consensus' own, bit for bit, on every pair of the scene
        o = np.empty(3)
        for m in range(len(a)):
            ka, kb = kps_a[ia[s]][pairs[s, m, 0]], kps_b[ib[s]][pairs[s, m, 1]]
            tc.lib().tri_calibrate(hca, ka["x"], ka["y"], o.ctypes.data)
            assert o.tobytes() == a[m].tobytes(), (s, m)
            tc.lib().tri_calibrate(hcb, kb["x"], kb["y"], o.ctypes.data)
            assert o.tobytes() == b[m].tobytes(), (s, m)
        P = pose[s].reshape(3, 4)
        ident = np.hstack([np.eye(3), np.zeros((3, 1))])
        dev_res = cons.residuals(P[None], a[inl[s, :n]], b[inl[s, :n]])[0]
        for i in range(n):
            if wr[i] != 0:
                continue
            points += 1
            m = inl[s, i]
            A = np.zeros((4, 4))
            for Q, v in ((ident, a[m]), (P, b[m])):
                t = Q - np.outer(v, v) @ Q
                A += t.T @ t
            if np.linalg.eigvalsh(A)[0] < 0.0:        # (the residual selects by |eigenvalue|, the triangulator by the signed one)
                continue
            compared += 1
            r = _np_residual_from_point(P, a[m], b[m], pts[s, i])
            worst = max(worst, abs(r - dev_res[i]))
            assert abs(r - dev_res[i]) <= 1e-9, (s, i, r, dev_res[i])
    print(f"models {models} / {S}, points {points}, residuals compared {compared}, worst |difference| {worst:.3g}")
    assert models >= expect_models and points > 0 and compared >= 0.5 * points


def cons_scene_bearings(cons, s, cap):
    return cons.scene(s, cap)


def test_two_view_inliers_chained_behind_the_consensus_synthetic_batch(gpu):
    """rs_triangulate_pairs_batch_device behind rs_essential_arrsac_batch_device on 64 synthetic scenes (ragged sizes, three
    without a model): bit-equal to the host build fed the downloaded pose and inliers; the residual recomputed in numpy from
    each returned point agrees with rs_debug_residuals to 1e-9."""
    torch = gpu
    from cv_amd.ransac import EssentialConsensus
    from test_gpu_parity import _pixel_scene
    rng = np.random.default_rng(0x64)
    S, cap, n_hyp = 64, 256, 128
    cam_a = (984.2439, 980.8141, 690.0, 233.1966, 0.0, None)
    cam_b = (950.0, 955.0, 640.0, 250.0, 0.5, -0.05)
    sizes = [int(v) for v in rng.integers(40, cap + 1, S)]
    sizes[3], sizes[17], sizes[40] = 0, 5, 7                         # no model: fewer than eight matches
    pairs = np.zeros((S, cap, 2), np.uint32)
    scenes = [_pixel_scene(rng, cap, cap, n, 0.2, cam_a) for n in sizes]
    for s, sc in enumerate(scenes):
        pairs[s, :len(sc[2])] = sc[2]
    ia = ib = [S - 1 - s for s in range(S)]
    kps_a = np.stack([sc[0] for sc in scenes[::-1]]); kps_b = np.stack([sc[1] for sc in scenes[::-1]])
    npairs = np.array([len(sc[2]) for sc in scenes], np.uint32)
    cons = EssentialConsensus(cap, n_hyp)
    cons.reserve(S)
    _check_pairs_batch(torch, cons, kps_a, kps_b, pairs, npairs, ia, ib, cam_a, cam_b, 2e-7, n_hyp, 5, expect_models=55)
    cons.close()


def test_two_view_inliers_on_the_kitti_pair(gpu, kitti):
    """The reference's own frame pair (akaze/tests/estimate_pose.rs: 399 / 343 descriptors, 11 matches, consensus at 0.1): the
    inliers' CameraPoints on the device, bit-equal to the host build."""
    torch = gpu
    from cv_amd import akaze, knn
    from cv_amd.ransac import EssentialConsensus
    kp1, ds1 = akaze.Akaze.sparse().extract_arrays(kitti[0])
    kp2, ds2 = akaze.Akaze.sparse().extract_arrays(kitti[1])
    m = np.array(knn.match_descriptors(ds1, ds2, 0.5), np.uint32)
    assert len(m) == 11
    cap = 512
    kps_a = np.zeros((1, cap), tc.KP_DTYPE); kps_b = np.zeros((1, cap), tc.KP_DTYPE)
    kps_a[0, :len(kp1)] = kp1; kps_b[0, :len(kp2)] = kp2
    pairs = np.zeros((1, cap, 2), np.uint32)
    pairs[0, :11] = m
    cam = (984.2439, 980.8141, 690.0, 233.1966, 0.0, None)
    cons = EssentialConsensus(cap, 256)
    cons.reserve(1)
    _check_pairs_batch(torch, cons, kps_a, kps_b, pairs, np.array([11], np.uint32), [0], [0], cam, cam, 0.1, 256, 0, expect_models=1)
    cons.close()


def test_registration_loop_closed_on_the_device(gpu, oracle):
    """A synthetic map — known poses, projected points with pixel noise, observation lists — goes in; the world table is made
    on the device (Registration.triangulate / triangulate_merged), match_views -> triangulate_merged -> consensus chain by
    their streams, and registered poses come out: d_world never visits the host on the way.  Afterwards the table is
    downloaded for the check: equal to the host build bit for bit, and the consensus equals oracle.p3p_arrsac_pairs on that
    table."""
    torch = gpu
    from cv_amd import _lib
    from cv_amd.registration import Registration
    from cv_amd.triangulation import LandmarkTable
    rng = np.random.default_rng(0x10C)
    V, F, cap, n_pts = 6, 4, 1024, 700
    NB = V + F
    f_cam = 1000.0
    poses = tc.random_poses(rng, NB)
    pts = np.stack([rng.uniform(-1.5, 1.5, n_pts), rng.uniform(-1.0, 1.0, n_pts), rng.uniform(4, 9, n_pts)], 1)
    desc_of = rng.integers(0, 256, (n_pts, 64), dtype=np.uint8)               # one descriptor per world point
    kps = np.zeros((NB, cap), tc.KP_DTYPE)
    descs = np.zeros((NB, cap, 64), np.uint8)
    counts = np.zeros(NB, np.int32)
    landmarks = np.zeros((NB, cap), np.uint32)
    lists = [[] for _ in range(n_pts)]
    for b in range(NB):
        seen = rng.permutation(n_pts)[:int(rng.integers(450, 600))]
        for j, l in enumerate(seen):
            x, y = tc.project(poses[b], pts[l], f_cam, CAM[2], CAM[3])
            kps[b, j]["x"], kps[b, j]["y"] = x + rng.uniform(-0.5, 0.5), y + rng.uniform(-0.5, 0.5)
            d = desc_of[l].copy()
            d[rng.integers(0, 64, 2)] ^= np.uint8(1) << rng.integers(0, 8, 2).astype(np.uint8)   # a couple of flipped bits
            descs[b, j] = d
            landmarks[b, j] = l
            if b < V:                                                        # the map knows the views' observations only
                lists[l].append((b, j))
        counts[b] = len(seen)
    dev = torch.device("cuda", 0)
    d_kps, d_descs = _kps_dev(torch, kps), _dev(torch, descs)
    d_counts, d_lm = _dev(torch, counts), _dev(torch, landmarks, np.int32)
    d_poses = _dev(torch, poses.reshape(NB, 12))
    table = LandmarkTable(torch, lists=lists)
    n_world = table.n_landmarks
    codewords = rng.integers(0, 256, (256, 64), dtype=np.uint8)
    kw = dict(block_size=32, max_candidates=64, estimations_per_block=16)
    thr, n_hyp = 2e-6, 256
    reg = Registration(torch, cap, F, V, codewords, CAM, threshold=thr, n_hypotheses=n_hyp, seed=11, **kw)
    d_merge_ok = torch.ones((F, cap), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    frame_blocks = [V + f for f in range(F)]
    view_blocks = [[v for v in range(V)] for f in range(F)]
    d_reason = torch.full((n_world,), 99, dtype=torch.uint8, device=dev)
    d_world = reg.triangulate(table, d_kps, d_poses, d_reason=d_reason)
    reg.match_views(d_descs, d_counts, frame_blocks, view_blocks, d_lm)
    reg.triangulate_merged(table, d_kps, d_poses, d_merge_ok, d_world, n_world)
    reg.consensus(d_kps, d_counts, d_world, n_world, d_merge_ok=d_merge_ok, d_obs_counts=table.d_obs_counts,
                  stream_to_wait=reg.rs_stream())
    reg.sync()
    # ---- only now anything comes back ----
    g_world = d_world.cpu().numpy()
    g_best = reg.best.cpu().numpy().view(np.uint32); g_dec = reg.decision.cpu().numpy().view(np.uint32)
    g_pairs = reg.pairs.cpu().numpy().view(np.uint32); g_np = reg.npairs.cpu().numpy().view(np.uint32)
    g_pose = reg.pose.cpu().numpy(); g_id = reg.best_id.cpu().numpy().view(np.uint32)
    g_inl = reg.inliers.cpu().numpy().view(np.uint32); g_ninl = reg.n_inliers.cpu().numpy().view(np.uint32)
    cam = tc.camera(*CAM[:5])
    start = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.uint32)
    obs = np.array([o for l in lists for o in l], np.uint32).reshape(-1, 2)
    want, want_r = tc.landmarks(kps, poses.reshape(NB, 12), cam, start, obs)
    want = np.concatenate([want, np.zeros((F * cap, 4))]); want[n_world:, 3] = -1.0
    tc.merged(kps, poses.reshape(NB, 12), cam, start, obs, g_best[:F], g_dec[:F], np.ones((F, cap), np.uint8), n_world, want)
    assert g_world.tobytes() == want.tobytes()
    assert np.array_equal(d_reason.cpu().numpy(), want_r) and (want_r == 0).sum() > 0.8 * n_pts
    ok = want_r == 0
    err = np.linalg.norm(want[:n_world][ok, :3] / want[:n_world][ok, 3:4] - pts[ok], axis=1)
    print("triangulated", int(ok.sum()), "of", n_pts, "median error", float(np.median(err)))
    assert np.median(err) < 0.05
    models = 0
    for f in range(F):
        n = int(g_np[f])
        assert n > 100, (f, n)
        want_c = oracle.p3p_arrsac_pairs(kps[frame_blocks[f]], g_pairs[f, :n], g_world, CAM, thr, n_hyp, scene=f, shuffle=False,
                                         seed=11, init_blocks=1, halve=True, sprt=True, **kw)
        assert g_id[f] == want_c["best_id"] and g_ninl[f] == len(want_c["inliers"]), (f, g_id[f], want_c["best_id"])
        if want_c["best_id"] == 0xFFFFFFFF:
            continue
        models += 1
        assert g_pose[f].tobytes() == want_c["pose"].tobytes(), f
        assert np.array_equal(g_inl[f, :g_ninl[f]], want_c["inliers"]), f
        P = g_pose[f].reshape(3, 4)
        T = poses[frame_blocks[f]]
        assert np.abs(P[:, :3] - T[:, :3]).max() < 0.01 and np.abs(P[:, 3] - T[:, 3]).max() < 0.05, (f, P, T)
    assert models == F
    reg.close()


def test_observations_entry_point_python_mirror_and_refusals(gpu):
    """rs_triangulate_observations and the Python LinearEigenTriangulator on the reference's doc-test pin
    (cv-geom/src/triangulation.rs:26-38: within 1e-6 of (0.3, 0.1, 2.0)); the reference's None cases; bad arguments are
    refused with AKZ_E_INVALID before any launch."""
    torch = gpu
    from cv_amd import _lib, triangulation
    from cv_amd.ransac import EssentialConsensus
    X = np.array([0.3, 0.1, 2.0])
    pose = np.hstack([tc.rodrigues([0.1, 0.1, 0.1]), np.full((3, 1), 0.1)])
    a = X / np.linalg.norm(X)
    q = pose[:, :3] @ X + pose[:, 3]
    b = q / np.linalg.norm(q)
    tri = triangulation.LinearEigenTriangulator.new()
    p = tri.triangulate_relative(pose, a, b)
    assert p is not None and np.linalg.norm(p[:3] / p[3] - X) < 1e-6
    ident = np.hstack([np.eye(3), np.zeros((3, 1))])
    want, why = tc.observations([ident, pose], [a, b])
    assert why == 0 and p.tobytes() == want.tobytes()
    assert tri.triangulate_observations([(ident, a), (pose, b)]).tobytes() == want.tobytes()
    assert tri.triangulate_observations_to_camera(a, [(pose, b)]).tobytes() == want.tobytes()
    assert tri.triangulate_observations([(ident, a)]) is None and tri.triangulate_observations([]) is None
    assert tri.triangulate_observations_with_reason([(ident, a), (pose, -b)])[1] == 5
    assert tri.max_iterations(1).triangulate_observations_with_reason([(ident, a), (pose, b)])[1] == 3
    assert tri.epsilon(1e-6).triangulate_relative(pose, a, b) is not None
    # max_iterations(0) is nalgebra's "no limit"; the device runs RS_TRI_MAX_SWEEPS at the most, which this list never needs
    assert tri.max_iterations(0).triangulate_relative(pose, a, b).tobytes() == want.tobytes()
    assert tri.max_iterations(0).epsilon(0.0).triangulate_relative(pose, a, b) is not None
    # refusals
    L = _lib.lib()
    cons = EssentialConsensus(8, 1)
    prm = triangulation.make_params()
    P = np.ascontiguousarray(np.stack([ident, pose]).reshape(2, 12)); B = np.ascontiguousarray(np.stack([a, b]))
    out = np.zeros(4)
    args = lambda prm_: (cons._h, P.ctypes.data, B.ctypes.data, 2, C.byref(prm_), out.ctypes.data, None)
    assert L.rs_triangulate_observations(*args(prm)) == 0
    assert L.rs_triangulate_observations(None, P.ctypes.data, B.ctypes.data, 2, C.byref(prm), out.ctypes.data, None) == -1
    assert L.rs_triangulate_observations(cons._h, None, B.ctypes.data, 2, C.byref(prm), out.ctypes.data, None) == -1
    assert L.rs_triangulate_observations(cons._h, P.ctypes.data, B.ctypes.data, 2, None, out.ctypes.data, None) == -1
    for field, val in (("struct_size", 8), ("max_sweeps", 0), ("eps", -1.0), ("eps", float("nan")),
                       ("incidence_minimum_cosine_distance", float("inf"))):
        bad = triangulation.make_params()
        setattr(bad, field, val)
        assert L.rs_triangulate_observations(*args(bad)) == -1, field
    d = torch.zeros((64,), dtype=torch.float64, device=torch.device("cuda", 0))
    cam = cons.camera(CAM)
    ptr = d.data_ptr()
    ok_args = [cons._h, ptr, 4, 1, ptr, C.byref(cam), ptr, ptr, 0, 0, C.byref(prm), ptr, None, None]
    assert L.rs_triangulate_landmarks_device(*ok_args) == 0                       # no landmarks: nothing to do
    for i, v in ((0, None), (1, None), (2, 0), (3, 0), (4, None), (6, None), (11, None)):
        bad_args = list(ok_args); bad_args[i] = v
        assert L.rs_triangulate_landmarks_device(*bad_args) == -1, i
    cam.reserved = 1
    assert L.rs_triangulate_landmarks_device(*ok_args) == -1
    cam.reserved = 0
    m_args = [cons._h, ptr, 4, 1, ptr, C.byref(cam), ptr, ptr, 0, 0, C.byref(prm), ptr, ptr, ptr, 0, 0, ptr, None, None]
    assert L.rs_triangulate_merged_device(*m_args) == 0
    for i, v in ((11, None), (12, None), (13, None), (14, 65536), (16, None)):
        bad_args = list(m_args); bad_args[i] = v
        assert L.rs_triangulate_merged_device(*bad_args) == -1, i
    one = (C.c_uint32 * 1)(0)
    p_args = [cons._h, ptr, ptr, 4, one, one, ptr, ptr, 0, C.byref(cam), C.byref(cam), ptr, ptr, ptr, ptr, C.byref(prm), ptr, None, None]
    assert L.rs_triangulate_pairs_batch_device(*p_args) == 0
    for i, v in ((1, None), (4, None), (11, None), (15, None), (16, None), (3, 0), (8, 65536)):
        bad_args = list(p_args); bad_args[i] = v
        assert L.rs_triangulate_pairs_batch_device(*bad_args) == -1, i
    p_args[8] = 2                                                                # more scenes than rs_batch_reserve left room for
    assert L.rs_triangulate_pairs_batch_device(*p_args) == -6
    cons.close()


def test_cpp_host_mirror_triangulate(gpu, tmp_path):
    """cv_geom::LinearEigenTriangulator of include/akaze.hpp from a native process (tests/cpp/triangulate.cpp): the
    reference's doc-test and its None cases."""
    import subprocess
    exe = host_build.native(tmp_path, "triangulate.cpp", hip=False)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "doc-test distance" in r.stdout and "none cases ok" in r.stdout and "triangulate ok" in r.stdout
