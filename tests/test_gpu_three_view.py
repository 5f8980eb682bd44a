"""The three-view bootstrap kernel (cv_amd/csrc/rs_three_view.hip) against the host build of the same header
(tests/three_view_checker.py): poses, every mask byte, every stats word and every verdict in bit patterns (NaN == NaN, the
bytes are compared).  Outputs a scene does not write keep the pattern they were filled with, on both sides.  Run with -m gpu."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import host_build
import three_view_checker as K

pytestmark = pytest.mark.gpu

QUICK = dict(three_view_patience=64, three_view_filter_loop_iterations=2)
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
    c = EssentialConsensus(2048, 1024)
    c.reserve(80)
    yield c
    c.close()


def scene_of(rig, cap, shuffle_seed=None):
    kps, triples, fo, so = rig.scene_arrays(cap, shuffle_seed)
    return dict(kps=kps, triples=triples, n=rig.n, fo=fo, nf=rig.n_first, so=so, ns=rig.n_second, pose_in=rig.pose_in.copy(), blocks=None)


def device_params(st):
    from cv_amd.three_view import ThreeViewInit
    return ThreeViewInit.params(**K.settings_dict(st))


def run(torch, cons, scenes, st, blocks_override=None):
    """The device call on `scenes` (scene s owns keypoint blocks 3s .. 3s + 2) and the host build on each; everything the call
    may write is compared in bytes.  -> the host results."""
    from cv_amd import _lib
    from cv_amd.three_view import ThreeViewInit
    S, cap = len(scenes), scenes[0]["kps"].shape[1]
    dev = torch.device("cuda", 0)
    up = lambda a: _lib.device_bytes(torch, a, dev)
    kps = np.concatenate([s["kps"] for s in scenes])
    blocks = [list(range(3 * s, 3 * s + 3)) for s in range(S)]
    for s, b in (blocks_override or {}).items():
        blocks[s] = b
    d_kps = up(kps)
    d_pf, d_ps = up(np.stack([s["pose_in"][0] for s in scenes])), up(np.stack([s["pose_in"][1] for s in scenes]))
    d_t, d_f, d_s = up(np.stack([s["triples"] for s in scenes])), up(np.stack([s["fo"] for s in scenes])), up(np.stack([s["so"] for s in scenes]))
    d_n = up(np.array([[s["n"] for s in scenes], [s["nf"] for s in scenes], [s["ns"] for s in scenes]], np.uint32))
    d_pose = torch.full((S * 24 * 8,), FILL, dtype=torch.uint8, device=dev)
    d_masks = torch.full((3, S * cap), FILL, dtype=torch.uint8, device=dev)
    d_verdict = torch.full((S * 4,), FILL, dtype=torch.uint8, device=dev)
    d_stats = torch.full((S * K.STATS * 4,), FILL, dtype=torch.uint8, device=dev)
    tv = ThreeViewInit(cons)
    tv.init_batch_device(d_kps.data_ptr(), cap, len(kps), [b[0] for b in blocks], [b[1] for b in blocks], [b[2] for b in blocks], K.rig_camera_dev(),
                         d_pf.data_ptr(), d_ps.data_ptr(), d_t.data_ptr(), d_n.data_ptr(), d_f.data_ptr(), d_n.data_ptr() + 4 * S, d_s.data_ptr(),
                         d_n.data_ptr() + 8 * S, device_params(st), d_pose.data_ptr(), d_verdict.data_ptr(), d_masks[0].data_ptr(),
                         d_masks[1].data_ptr(), d_masks[2].data_ptr(), d_stats.data_ptr(), _stream(torch))
    cons.sync()
    pose = d_pose.cpu().numpy().view(np.float64).reshape(S, 24)
    masks = d_masks.cpu().numpy().reshape(3, S, cap)
    verdict = d_verdict.cpu().numpy().view(np.uint32)
    stats = d_stats.cpu().numpy().view(np.uint32).reshape(S, K.STATS)
    prior = (np.full(24 * 8, FILL, np.uint8).view(np.float64), *(np.full(cap, FILL, np.uint8) for _ in range(3)))
    hosts = []
    for s, sc in enumerate(scenes):
        h = K.init_scene(kps, len(kps), blocks[s], K.rig_camera(), sc["pose_in"], sc["triples"], sc["n"], sc["fo"], sc["nf"], sc["so"], sc["ns"], st,
                         prior=prior)
        hosts.append(h)
        assert verdict[s] == h["verdict"], (s, verdict[s], h["verdict"], stats[s], h["stats"])
        assert np.array_equal(stats[s], h["stats"]), (s, stats[s], h["stats"])
        assert pose[s].tobytes() == h["pose_out"].tobytes(), (s, pose[s], h["pose_out"])
        for m, k in enumerate(("combined", "first_ok", "second_ok")):
            assert np.array_equal(masks[m, s], h[k]), (s, k)
    return hosts


def _stream(torch):
    from cv_amd import _lib
    return _lib.wait_handle(torch.cuda.current_stream(torch.device("cuda", 0)))


COUNTS = [0, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1500]


@pytest.fixture(scope="module")
def count_scenes():
    return [scene_of(K.Rig(100 + n, n, noise=0.5, perturb=2e-3, n_first=min(n, 9), n_second=min(n, 5), outliers=n // 16 if n >= 63 else 0), 1536, shuffle_seed=n)
            for n in COUNTS]


def test_common_match_counts(gpu, cons, count_scenes):
    hosts = run(gpu, cons, count_scenes, K.settings(**QUICK))
    by = dict(zip(COUNTS, hosts))
    assert [by[n]["verdict"] for n in (0, 15)] == [1, 1] and [by[n]["verdict"] for n in (16, 17, 31)] == [3, 3, 3]
    assert all(by[n]["verdict"] == 0 for n in COUNTS if n >= 32)
    # take(1024): the first run of the two largest scenes takes 1024 landmarks, every run of the largest (1500 - 93 outliers
    # pass the later filters); the masks still cover the matches behind the last landmark taken
    assert by[1025]["stats"][K.S_RUN_MATCHES] == 1024
    assert list(by[1500]["stats"][K.S_RUN_MATCHES:K.S_RUN_MATCHES + 3]) == [1024, 1024, 1024]
    for n in (1025, 1500):
        assert by[n]["combined"][1024:n].sum() > 0


@pytest.mark.parametrize("cap_landmarks", [32, 33, 100, 1024])
def test_optimisation_landmark_caps(gpu, cons, count_scenes, cap_landmarks):
    pick = [count_scenes[COUNTS.index(n)] for n in (33, 65, 257, 1025, 1500)]
    hosts = run(gpu, cons, pick, K.settings(three_view_optimization_landmarks=cap_landmarks, **QUICK))
    assert all(h["verdict"] == 0 for h in hosts)
    assert [int(h["stats"][K.S_RUN_MATCHES]) for h in hosts] == [min(cap_landmarks, n) for n in (33, 65, 257, 1025, 1500)]


@pytest.mark.parametrize("patience", [1, 50, 51, 300])
@pytest.mark.parametrize("filters", [0, 1, 3])
def test_patience_and_filter_iterations(gpu, cons, count_scenes, patience, filters):
    pick = [count_scenes[COUNTS.index(n)] for n in (64, 257)]
    hosts = run(gpu, cons, pick, K.settings(three_view_patience=patience, three_view_filter_loop_iterations=filters))
    for h in hosts:
        assert h["verdict"] == 0
        assert list(h["stats"][K.S_RUN_STOP:K.S_RUN_STOP + filters + 1]) == [patience - 1] * (filters + 1)
        assert np.all(h["stats"][K.S_RUN_STOP + filters + 1:K.S_ROBUST] == 0xFFFFFFFF)


def verdict_scenes(cap):
    """one scene per verdict under minimum_robust_matches = 50 and two filter iterations"""
    tight = K.Rig(31, 60, noise=0.5, perturb=2e-3)
    z = tight.points[:, 2]
    tight.points[:, 0], tight.points[:, 1] = 0.04 * (tight.points[:, 0] / (0.35 * z)) * z, 0.04 * (tight.points[:, 1] / (0.2 * z)) * z
    ident = np.hstack([np.eye(3), np.zeros((3, 1))])
    tight.px = [np.asarray(K.project(p, tight.points), np.float32) for p in (ident, tight.first, tight.second)]
    return {0: scene_of(K.Rig(32, 200, noise=0.5, perturb=2e-3, n_first=20, n_second=30, outliers=12), cap, 5),
            1: scene_of(K.Rig(33, 15, noise=0.5, perturb=2e-3), cap),
            2: scene_of(tight, cap),
            3: scene_of(K.Rig(34, 31, noise=0.5, perturb=2e-3), cap),
            4: scene_of(K.Rig(35, 100, noise=0.5, perturb=2e-3, outliers=60), cap),
            5: scene_of(K.Rig(36, 45, noise=0.5, perturb=2e-3, n_first=3), cap)}


@pytest.mark.parametrize("n_scenes", [1, 3, 67])
def test_batches_mix_every_verdict(gpu, cons, n_scenes):
    """67 scenes: every verdict among accepted ones (bad indices included), rejected between accepted.  An accepted scene's
    results equal those of a call with that scene alone."""
    cap = 256
    st = K.settings(three_view_minimum_robust_matches=50, **QUICK)
    kinds = verdict_scenes(cap)
    order = [0, 4, 0, 1, 2, 0, 3, 5, 6, 0]
    scenes, want = [], []
    for s in range(n_scenes):
        k = order[s % len(order)]
        sc = {key: (v.copy() if isinstance(v, np.ndarray) else v) for key, v in kinds[0 if k == 6 else k].items()}
        if k == 6:
            sc["triples"][7, s % 3] = cap                      # a feature index == cap_per_img
        scenes.append(sc)
        want.append(k)
    hosts = run(gpu, cons, scenes, st)
    assert [h["verdict"] for h in hosts] == want
    alone = run(gpu, cons, [scenes[0]], st)[0]
    for s, k in enumerate(want):
        if k == 0:
            assert all(np.array_equal(hosts[s][key], alone[key]) for key in ("pose_out", "combined", "first_ok", "second_ok", "stats"))


def test_degenerate_landmarks_inside_a_good_scene(gpu, cons):
    """A centre keypoint at the first camera's epipole (its bearing runs along the translation) and a match whose three
    keypoints are the same pixel (identical bearings), in the middle of 120 good matches."""
    rig = K.Rig(41, 120, noise=0.5, perturb=2e-3)
    sc = scene_of(rig, 128)
    centre = -rig.first[:, :3].T @ rig.first[:, 3]
    epi = K.project(np.hstack([np.eye(3), np.zeros((3, 1))]), centre[None] * 10.0)[0]
    sc["kps"]["x"][0, 120], sc["kps"]["y"][0, 120] = epi
    sc["kps"]["x"][1:, 120], sc["kps"]["y"][1:, 120] = sc["kps"]["x"][1:, 3], sc["kps"]["y"][1:, 3]
    for b in range(3):
        sc["kps"]["x"][b, 121], sc["kps"]["y"][b, 121] = 700.0, 400.0
    sc["triples"][60:122] = np.concatenate([[[120] * 3, [121] * 3], sc["triples"][60:120]])
    sc["n"] = 122
    h = run(gpu, cons, [sc], K.settings(**QUICK))[0]
    assert h["verdict"] == 0 and np.all(np.isfinite(h["pose_out"]))


def test_bad_index_refuses_the_scene_only(gpu, cons):
    cap = 128
    good = scene_of(K.Rig(51, 100, noise=0.5, perturb=2e-3, n_first=4, n_second=4), cap)
    scenes = [{k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in good.items()} for _ in range(6)]
    scenes[1]["triples"][99, 2] = cap
    scenes[2]["fo"][3, 1] = cap
    scenes[3]["so"][0, 0] = 0xFFFFFFFF
    # scene 4: a block == n_blocks
    hosts = run(gpu, cons, scenes, K.settings(**QUICK), blocks_override={4: [12, 13, 18]})
    assert [h["verdict"] for h in hosts] == [0, 6, 6, 6, 6, 0]
    assert all(h["stats"][K.S_STAGE] == 0 for h in hosts[1:5])


def test_chain_from_two_consensuses(gpu, cons):
    """rs_essential_arrsac_batch_device for (centre, first) and (centre, second) -> join_pairs on their inliers ->
    rs_three_view_init_batch_device behind the uploads of the joined lists (stream_to_wait, no host wait in between): verdict
    OK, and the device's result equals the host build fed the same device-produced poses and lists."""
    torch = gpu
    from cv_amd.three_view import join_pairs
    cap = 512
    rig = K.Rig(61, 300, noise=0.5, n_first=40, n_second=50)
    kps, _, _, _ = rig.scene_arrays(cap)
    dev = torch.device("cuda", 0)
    d_kps = torch.from_numpy(kps.view(np.uint8).reshape(3, cap, 28)).to(dev)
    idx = np.arange(cap, dtype=np.uint32)
    pairs = np.zeros((2, cap, 2), np.uint32)
    first = np.concatenate([idx[:300], idx[300:340]])
    second = np.concatenate([idx[:300], idx[340:390]])
    pairs[0, :len(first)] = first[:, None]
    pairs[1, :len(second)] = second[:, None]
    d_pairs = torch.from_numpy(pairs.view(np.int32)).to(dev)
    d_np = torch.from_numpy(np.array([len(first), len(second)], np.int32)).to(dev)
    d_pose = torch.zeros((2, 12), dtype=torch.float64, device=dev)
    d_best = torch.zeros((2,), dtype=torch.int32, device=dev)
    d_inl = torch.zeros((2, cap), dtype=torch.int32, device=dev)
    d_ninl = torch.zeros((2,), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    cam = K.rig_camera_dev()
    prm = cons.make_params(1e-5, n_hypotheses=256, seed=7, block_size=64, init_blocks=1, max_candidates=64, halve=True)
    cons.model_inliers_batch_device(d_kps.data_ptr(), d_kps.data_ptr(), cap, [0, 0], [1, 2], d_pairs.data_ptr(), d_np.data_ptr(), cam, cam, prm,
                                    d_pose.data_ptr(), d_best.data_ptr(), d_inl.data_ptr(), d_ninl.data_ptr(), None, shuffle=False)
    cons.sync()
    assert np.all(d_best.cpu().numpy().view(np.uint32) != 0xFFFFFFFF)
    inl, ninl = d_inl.cpu().numpy().view(np.uint32), d_ninl.cpu().numpy().view(np.uint32)
    lists = [pairs[k][inl[k, :ninl[k]]] for k in range(2)]
    assert min(ninl) >= 200
    triples, fo, so = join_pairs(lists[0], lists[1], permutation=np.random.default_rng(3).permutation(len(set(lists[0][:, 0]) & set(lists[1][:, 0]))))
    pad = lambda a, w: np.concatenate([a, np.zeros((cap - len(a), w), np.uint32)])
    pose_in = d_pose.cpu().numpy().reshape(2, 3, 4)
    sc = dict(kps=kps, triples=pad(triples, 3), n=len(triples), fo=pad(fo, 2), nf=len(fo), so=pad(so, 2), ns=len(so), pose_in=pose_in)
    h = run(torch, cons, [sc], K.settings(**QUICK))[0]
    assert h["verdict"] == 0
    assert h["combined"][:len(triples)].sum() >= 0.9 * len(triples)


def test_default_settings_scene(gpu, cons):
    """1 024 landmarks, patience 65 536, 8 filter iterations, one triple: verdict, stats, masks and poses against the host
    build's recorded result (tests/golden/three_view_default.npz, made by tests/golden/make_three_view_golden.py: the host
    build needs 191 s for it).  Measured on the MI355X: 18.9 us per iteration, 11.0 s for the 589 824 iterations, and the
    poses equal the host build's bit for bit — asserted; the tolerance of tests/test_three_view_math.py (6.6e-14) is what would
    hold if they did not.  The time limit is three times what a patience-512 call projects, and that must be below 60 s."""
    import time
    torch = gpu
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "three_view_default.npz"))
    cap = g["kps"].shape[1]
    kps = np.ascontiguousarray(g["kps"]).view(K.KP_DTYPE).reshape(3, cap)
    n, nf, ns = (int(x) for x in g["counts"])
    sc = dict(kps=kps, triples=g["triples"], n=n, fo=g["first_only"], nf=nf, so=g["second_only"], ns=ns, pose_in=g["pose_in"])
    from cv_amd import _lib
    from cv_amd.three_view import ThreeViewInit
    dev = torch.device("cuda", 0)
    up = lambda a: _lib.device_bytes(torch, a, dev)
    d_kps, d_p, d_t, d_f, d_s = up(kps), up(sc["pose_in"]), up(sc["triples"]), up(sc["fo"]), up(sc["so"])
    d_n = up(g["counts"])
    d_pose = torch.zeros(24, dtype=torch.float64, device=dev)
    d_masks = torch.zeros((3, cap), dtype=torch.uint8, device=dev)
    d_out = torch.zeros(1 + K.STATS, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

    def call(st):
        t0 = time.perf_counter()
        ThreeViewInit(cons).init_batch_device(d_kps.data_ptr(), cap, 3, [0], [1], [2], K.rig_camera_dev(), d_p.data_ptr(), d_p.data_ptr() + 96,
                                              d_t.data_ptr(), d_n.data_ptr(), d_f.data_ptr(), d_n.data_ptr() + 4, d_s.data_ptr(),
                                              d_n.data_ptr() + 8, device_params(st), d_pose.data_ptr(), d_out.data_ptr(), d_masks[0].data_ptr(),
                                              d_masks[1].data_ptr(), d_masks[2].data_ptr(), d_out.data_ptr() + 4)
        cons.sync()
        return time.perf_counter() - t0

    call(K.settings(three_view_patience=8))                                   # (the first call loads the code object)
    t512 = call(K.settings(three_view_patience=512))
    its = int(np.sum(d_out.cpu().numpy().view(np.uint32)[1 + K.S_RUN_STOP:1 + K.S_ROBUST].astype(np.int64) + 1))
    limit = 3 * t512 / its * 9 * 65536
    print(f"patience 512: {its} iterations in {t512 * 1e3:.1f} ms, limit of the default-settings call {limit:.1f} s")
    assert its == 9 * 512 and limit < 60
    took = call(K.settings())
    out = d_out.cpu().numpy().view(np.uint32)
    masks = d_masks.cpu().numpy()
    pose = d_pose.cpu().numpy()
    print(f"default settings: {took:.2f} s, largest pose difference {np.max(np.abs(pose - g['pose_out'])):.3g}")
    assert took <= limit
    assert out[0] == g["verdict"] == 0
    assert np.array_equal(out[1:], g["stats"])
    assert np.max(np.abs(pose - g["pose_out"])) <= 6.6e-14
    assert pose.tobytes() == g["pose_out"].tobytes()
    for m, k in enumerate(("combined", "first_ok", "second_ok")):
        assert np.array_equal(masks[m], g[k]), k


def test_cpp_host_mirror_three_view(gpu, cons, tmp_path):
    """cv_sfm::ThreeViewInit of include/akaze.hpp from a native process (tests/cpp/three_view.cpp): its printed verdict, poses
    and stats equal the ctypes path's."""
    exe = host_build.native(tmp_path, "three_view.cpp", hip=True)
    cap = 256
    rig = K.Rig(71, 150, noise=0.5, perturb=2e-3, n_first=11, n_second=13, outliers=9)
    sc = scene_of(rig, cap, shuffle_seed=2)
    with open(tmp_path / "scene.bin", "wb") as f:
        f.write(np.array([cap, sc["n"], sc["nf"], sc["ns"], QUICK["three_view_patience"], QUICK["three_view_filter_loop_iterations"]], np.uint32).tobytes())
        f.write(np.array([K.CAM["fx"], K.CAM["fy"], K.CAM["cx"], K.CAM["cy"]], np.float64).tobytes())
        f.write(np.ascontiguousarray(sc["pose_in"], np.float64).tobytes())
        for a in (sc["kps"], sc["triples"], sc["fo"], sc["so"]):
            f.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([str(exe), str(tmp_path / "scene.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "three_view ok" in r.stdout
    h = run(gpu, cons, [sc], K.settings(**QUICK))[0]
    lines = dict(l.split(" ", 1) for l in r.stdout.strip().splitlines() if " " in l)
    assert int(lines["verdict"]) == h["verdict"] == 0
    assert lines["poses"].split() == [f"{int(u):016x}" for u in h["pose_out"].view(np.uint64)]
    assert [int(x) for x in lines["stats"].split()] == [int(x) for x in h["stats"]]
    assert [int(x) for x in lines["masks"].split()] == [int(h[k][:m].sum()) for k, m in (("combined", sc["n"]), ("first_ok", sc["nf"]),
                                                                                         ("second_ok", sc["ns"]))]
