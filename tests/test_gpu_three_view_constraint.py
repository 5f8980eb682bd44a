"""The three-view constraint kernel (cv_amd/csrc/rs_three_view_constraint.hip) against the host build of the same header
(tests/three_view_constraint_checker.py): poses, every stats word and every verdict in bit patterns (the bytes are
compared).  Poses a constraint does not write keep the pattern they were filled with, on both sides.  Run with -m gpu.

Residency: the kernel takes 230 VGPRs, two waves per SIMD, 2 048 constraints at once on the 256 CUs; the batch of 1 025 is
beyond one wave per SIMD (1 024), the batch of 2 305 beyond what is resident at all."""
import subprocess

import numpy as np
import pytest

import host_build
import three_view_constraint_checker as T

pytestmark = pytest.mark.gpu

FILL = 0xA5
CAP = 320


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


@pytest.fixture(scope="module")
def scenes():
    """0: 300 landmarks; 1 - 7: 140 each; 8: 40 in a field too small for a robust bearing pair"""
    return [T.scene(500, 300)] + [T.scene(501 + k, 140) for k in range(7)] + [T.scene(77, 40, spread=0.05)]


def camera():
    from cv_amd import _lib
    return _lib.Camera(T.K.CAM["fx"], T.K.CAM["fy"], T.K.CAM["cx"], T.K.CAM["cy"], 0.0, 0.0, 0, 0)


def run(torch, cons, arrays, st, n_lm=None):
    """The device call on `arrays` (T.device_arrays) and the host build on each constraint; everything the call may write is
    compared in bytes.  -> the host results."""
    from cv_amd import _lib
    from cv_amd.three_view import ThreeViewConstraints
    kps, poses, views, lm_start, lm = arrays
    n = len(views)
    n_lm = len(lm) if n_lm is None else n_lm
    dev = torch.device("cuda", 0)
    up = lambda a: _lib.device_bytes(torch, a, dev)
    d_kps, d_poses, d_views, d_start, d_lm = up(kps), up(poses), up(views), up(lm_start), up(lm)
    d_pose = torch.full((n * 24 * 8,), FILL, dtype=torch.uint8, device=dev)
    d_verdict = torch.full((n * 4,), FILL, dtype=torch.uint8, device=dev)
    d_stats = torch.full((n * T.STATS * 4,), FILL, dtype=torch.uint8, device=dev)
    ThreeViewConstraints(cons).batch_device(d_kps.data_ptr(), kps.shape[1], kps.shape[0], d_poses.data_ptr(), camera(), d_views.data_ptr(),
                                            d_start.data_ptr(), d_lm.data_ptr(), n_lm, n, ThreeViewConstraints.params(**T.settings_dict(st)),
                                            d_pose.data_ptr(), d_verdict.data_ptr(), d_stats.data_ptr(),
                                            _lib.wait_handle(torch.cuda.current_stream(dev)))
    cons.sync()
    pose = d_pose.cpu().numpy().view(np.float64).reshape(n, 24)
    verdict = d_verdict.cpu().numpy().view(np.uint32)
    stats = d_stats.cpu().numpy().view(np.uint32).reshape(n, T.STATS)
    prior = np.full(24 * 8, FILL, np.uint8).view(np.float64)
    hosts = []
    lm_host = lm[:n_lm] if n_lm <= len(lm) else np.concatenate([lm, np.zeros((n_lm - len(lm), 3), np.uint32)])
    for s in range(n):
        h = T.constraint_scene(kps, poses, T.K.rig_camera(), views, lm_start, lm_host, s, st, prior=prior)
        hosts.append(h)
        assert verdict[s] == h["verdict"], (s, verdict[s], h["verdict"], stats[s], h["stats"])
        assert np.array_equal(stats[s], h["stats"]), (s, stats[s], h["stats"])
        assert pose[s].tobytes() == h["pose_out"].tobytes(), (s, pose[s], h["pose_out"])
    return hosts


LENGTHS = [0, 1, 23, 24, 63, 64, 65, 127, 128, 255, 256, 300]


@pytest.mark.parametrize("cap_landmarks", [64, 65, 256])
def test_list_lengths(gpu, cons, scenes, cap_landmarks):
    """the lane and stride boundaries: one landmark per lane up to 64, then two, ..., four at 256"""
    arrays = T.device_arrays(scenes[:1], CAP, [(0, np.arange(n)) for n in LENGTHS])
    hosts = run(gpu, cons, arrays, T.settings(constraint_patience=16, optimization_maximum_landmarks=cap_landmarks))
    assert [h["verdict"] for h in hosts] == [T.FEW_LANDMARKS if n < 24 else T.OK for n in LENGTHS]
    assert [int(h["stats"][T.S_USED]) for h in hosts] == [0 if n < 24 else min(n, cap_landmarks) for n in LENGTHS]
    assert [int(h["stats"][T.S_LANDMARKS]) for h in hosts] == LENGTHS


@pytest.mark.parametrize("patience", [0, 1, 2, 50, 4096])
def test_patience(gpu, cons, scenes, patience):
    arrays = T.device_arrays(scenes[:2], CAP, [(0, np.arange(24)), (1, np.arange(64)), (0, np.arange(100))])
    hosts = run(gpu, cons, arrays, T.settings(constraint_patience=patience, optimization_maximum_landmarks=128))
    assert all(h["verdict"] == T.OK for h in hosts)
    if patience == 0:       # nothing moves: the result is the relative poses through two inversions and the scale
        for h in hosts:
            assert abs(T.stat_f64(h["stats"], T.S_FINAL_SCALE) - T.stat_f64(h["stats"], T.S_ORIGINAL_SCALE)) < 1e-14


def mixed_batch(scenes, n, seed):
    """n constraints over the scenes, every verdict among them (from three constraints on): shuffled lists of several
    lengths, the scene without bearing pairs, lists below the minimum, and indices out of range."""
    rng = np.random.default_rng(seed)
    lengths = [64, 24, 10, 40, 70, 130, 33, 63]
    cons_ = []
    for i in range(n):
        k = 8 if i % 11 == 1 else 1 + i % 7
        length = min(lengths[i % len(lengths)], scenes[k].n)
        cons_.append((k, rng.permutation(scenes[k].n)[:length]))
    arrays = T.device_arrays(scenes, CAP, cons_)
    kps, poses, views, lm_start, lm = arrays
    for i in range(5, n, 50):          # a feature out of range
        lm[lm_start[i] + (i % 3), i % 3] = CAP + i
    for i in range(17, n, 100):        # a block out of range
        views[i, i % 3] = len(kps)
    return arrays


@pytest.mark.parametrize("n,patience", [(1, 16), (3, 16), (67, 16), (1025, 64), (2305, 4)])
def test_batches(gpu, cons, scenes, n, patience):
    hosts = run(gpu, cons, mixed_batch(scenes, n, n), T.settings(constraint_patience=patience))
    seen = {h["verdict"] for h in hosts}
    assert seen == ({T.OK} if n == 1 else {T.OK, T.FEW_LANDMARKS, T.FEW_BEARING_PAIRS} if n == 3 else {0, 1, 2, 3})


def test_bad_indices_refuse_their_own_constraint_only(gpu, cons, scenes):
    cons_ = [(1 + i % 3, np.arange(30 + i)) for i in range(8)]
    kps, poses, views, lm_start, lm = T.device_arrays(scenes, CAP, cons_)
    good = run(gpu, cons, (kps, poses, views, lm_start, lm), T.settings(constraint_patience=8, optimization_maximum_landmarks=20))
    assert all(h["verdict"] == T.OK for h in good)
    views, lm, lm_start = views.copy(), lm.copy(), lm_start.copy()
    views[0, 1] = len(kps)                      # a block
    views[1, 0] = 0xFFFFFFFF
    lm[lm_start[2] + 3, 2] = CAP                # a feature among the landmarks used
    lm[lm_start[3] + 29, 0] = 0xFFFFFFFF        # a feature behind the landmarks used: the whole list is looked at
    lm_start[5] = lm_start[4] - 1               # constraint 4's range runs backwards; constraint 5 begins one landmark early
    hosts = run(gpu, cons, (kps, poses, views, lm_start, lm), T.settings(constraint_patience=8, optimization_maximum_landmarks=20),
                n_lm=len(lm) - 1)               # constraint 7's range leaves [0, n_lm]
    assert [h["verdict"] for h in hosts] == [3, 3, 3, 3, 3, 0, 0, 3]
    assert all(np.all(h["stats"] == 0) for h in hosts if h["verdict"] == 3)
    assert hosts[6]["pose_out"].tobytes() == good[6]["pose_out"].tobytes()


def test_degenerate_landmarks_inside_a_good_constraint(gpu, cons, scenes):
    """the same landmark many times over, and keypoints whose bearings are NaN: their gradients are NaN, which
    Se3TangentSpace::new turns into zero vectors, and no comparison with a NaN counts a bearing pair"""
    order = np.arange(64)
    order[10:20] = 3                                              # ten copies of landmark 3
    kps, poses, views, lm_start, lm = T.device_arrays(scenes[1:3], CAP, [(0, order), (1, np.arange(64)), (0, np.full(64, 7))])
    kps["x"][3 + 1, 5] = np.nan                                   # scene 1 (blocks 3 - 5): landmark 5 in the second view
    kps["y"][3 + 2, 40] = np.nan
    kps["x"][3, 41] = np.inf
    hosts = run(gpu, cons, (kps, poses, views, lm_start, lm), T.settings(constraint_patience=32))
    assert [h["verdict"] for h in hosts] == [T.OK, T.OK, T.FEW_BEARING_PAIRS]
    assert np.all(np.isfinite(hosts[0]["pose_out"])) and np.all(np.isfinite(hosts[1]["pose_out"]))
    # 64 copies of one landmark, no pair asked for: the optimiser runs on it
    hosts = run(gpu, cons, (kps, poses, views, lm_start, lm), T.settings(constraint_patience=32, robust_view_num_robust_bearing_pair=0))
    assert [h["verdict"] for h in hosts] == [T.OK] * 3 and hosts[2]["stats"][T.S_PAIRS] == 0


def test_a_pose_that_is_not_finite(gpu, cons, scenes):
    kps, poses, views, lm_start, lm = T.device_arrays(scenes[1:4], CAP, [(0, np.arange(64)), (1, np.arange(64)), (2, np.arange(64))])
    poses[1, 7] = np.nan          # the second view of constraint 0
    poses[6, 0] = np.nan          # the first view of constraint 2
    hosts = run(gpu, cons, (kps, poses, views, lm_start, lm), T.settings(constraint_patience=8))
    assert [h["verdict"] for h in hosts] == [T.OK] * 3             # the bearing pairs do not look at the poses
    assert np.any(np.isnan(hosts[0]["pose_out"])) and np.any(np.isnan(hosts[2]["pose_out"]))
    assert np.all(np.isfinite(hosts[1]["pose_out"]))


def test_default_settings_constraint(gpu, cons, scenes):
    """64 landmarks, 4 096 iterations, the reference's defaults, against the host build directly (0.1 s on the host)."""
    hosts = run(gpu, cons, T.device_arrays(scenes[:1], CAP, [(0, np.arange(64)), (0, np.arange(300))]), T.settings())
    assert [h["verdict"] for h in hosts] == [T.OK, T.OK] and [int(h["stats"][T.S_USED]) for h in hosts] == [64, 64]
    assert hosts[0]["pose_out"].tobytes() == hosts[1]["pose_out"].tobytes()        # take(64) of the longer list


def test_run_takes_torch_tensors(gpu, cons, scenes):
    """ThreeViewConstraints.run, the convenience over tensors, gives what the pointer call gives"""
    from cv_amd.three_view import ThreeViewConstraints
    torch = gpu
    arrays = T.device_arrays(scenes[:2], CAP, [(0, np.arange(64)), (1, np.arange(20)), (1, np.arange(100))])
    st = T.settings(constraint_patience=8)
    hosts = run(torch, cons, arrays, st)
    kps, poses, views, lm_start, lm = arrays
    dev = torch.device("cuda", 0)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(dev)
    res = ThreeViewConstraints(cons).run(torch, t(kps, np.uint8).reshape(len(kps), CAP, 28), t(poses, np.float64), camera(),
                                         t(views, np.int32), t(lm_start, np.int32), t(lm, np.int32),
                                         ThreeViewConstraints.params(constraint_patience=8))
    assert res.verdicts.tolist() == [h["verdict"] for h in hosts] == [0, 1, 0]
    for s in (0, 2):
        assert res.poses[s].tobytes() == hosts[s]["pose_out"].tobytes() and np.array_equal(res.stats[s], hosts[s]["stats"])
    assert res.scale(0) == T.stat_f64(hosts[0]["stats"], T.S_FINAL_SCALE)


def test_cpp_host_mirror_three_view_constraint(gpu, cons, scenes, tmp_path):
    """cv_sfm::ThreeViewConstraints of include/akaze.hpp from a native process (tests/cpp/three_view_constraint.cpp): its
    printed verdicts, poses and stats equal the ctypes path's."""
    exe = host_build.native(tmp_path, "three_view_constraint.cpp", hip=True)
    arrays = T.device_arrays(scenes[1:3] + scenes[8:], CAP, [(0, np.arange(64)), (1, np.arange(12)), (1, np.arange(130)), (2, None)])
    kps, poses, views, lm_start, lm = arrays
    patience, maximum = 24, 100
    with open(tmp_path / "batch.bin", "wb") as f:
        f.write(np.array([CAP, len(kps), len(views), len(lm), patience, maximum], np.uint32).tobytes())
        f.write(np.array([T.K.CAM["fx"], T.K.CAM["fy"], T.K.CAM["cx"], T.K.CAM["cy"]], np.float64).tobytes())
        for a in (poses, kps, views, lm_start, lm):
            f.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([str(exe), str(tmp_path / "batch.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "three_view_constraint ok" in r.stdout
    hosts = run(gpu, cons, arrays, T.settings(constraint_patience=patience, optimization_maximum_landmarks=maximum))
    lines = dict(l.split(" ", 1) for l in r.stdout.strip().splitlines() if " " in l)
    assert [int(x) for x in lines["verdicts"].split()] == [h["verdict"] for h in hosts] == [0, 1, 0, 2]
    got = lines["poses"].split()
    for s, h in enumerate(hosts):
        if h["verdict"] == 0:
            assert got[24 * s:24 * s + 24] == [f"{int(u):016x}" for u in h["pose_out"].view(np.uint64)]
        else:
            assert got[24 * s:24 * s + 24] == ["0" * 16] * 24
    assert [int(x) for x in lines["stats"].split()] == [int(x) for h in hosts for x in h["stats"]]
