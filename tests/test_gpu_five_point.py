"""The five-point estimator of the two-view consensus on the device (rs_five_point_batch, RS_ESTIMATOR_FIVE_POINT):
device == host build of include/akz_five_point_math.h bit for bit, the E -> poses -> residual path == the oracle's on the
device's own matrices, and the consensus entry points agree with one another.  Run with -m gpu."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import host_build
import five_point_checker as ck
import five_point_statement as st

pytestmark = pytest.mark.gpu

TOL_E = 5.2e-8       # tests/test_five_point_math.py: 10 x the measured host-build-vs-statement deviation


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cv_amd import build
    build.build()
    from cv_amd import ransac
    return ransac


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def pool():
    """The matches of the 512 seeded exact scenes side by side: sample s = matches 5 s .. 5 s + 4, except every seventh,
    which repeats a match (nullity 5: rejected) — rejected samples sit between valid ones."""
    sc = st.scenes()
    a = np.concatenate([s[0] for s in sc]); b = np.concatenate([s[1] for s in sc])
    samples = np.arange(5 * len(sc), dtype=np.uint32).reshape(-1, 5)
    samples[3::7, 4] = samples[3::7, 3]
    return a, b, samples


@pytest.fixture(scope="module")
def noisy():
    """300 matches of one rigid motion, half of them replaced by outliers, 0.5 px noise at f = 1000; 128 samples."""
    rng = np.random.default_rng(0xF15E)
    n = 300
    r = st.rotation(rng.normal(size=3), 0.15)
    t = np.array([0.5, -0.1, 0.2])
    p = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(3, 9, n)], axis=1)
    q = p @ r.T + t

    def bearings(x):
        xy = x[:, :2] / x[:, 2:] + rng.normal(size=(len(x), 2)) * (0.5 / 1000.0)
        v = np.concatenate([xy, np.ones((len(x), 1))], axis=1)
        return v / np.linalg.norm(v, axis=1, keepdims=True)
    a, b = bearings(p), bearings(q)
    out = rng.permutation(n)[:n // 2]
    b[out] = bearings(np.stack([rng.uniform(-2, 2, len(out)), rng.uniform(-1.5, 1.5, len(out)), rng.uniform(3, 9, len(out))], axis=1))
    samples = np.stack([rng.choice(n, 5, replace=False) for _ in range(128)]).astype(np.uint32)
    return np.ascontiguousarray(a), np.ascontiguousarray(b), samples, 5e-7


@pytest.fixture(scope="module")
def exhaustive(gpu, noisy):
    """rs_five_point_batch on the noisy scene, once: (pose, inliers, best_id, counts [1280, 4], poses, ok)"""
    a, b, samples, thr = noisy
    cons = gpu.EssentialConsensus(len(a), 10 * len(samples))
    pose, inl, best = cons.five_point_model_inliers(a, b, samples, thr)
    counts = cons.counts(10 * len(samples))
    poses, ok = cons.poses(10 * len(samples))
    cons.close()
    return pose.copy(), inl, best, counts, poses, ok


@pytest.mark.parametrize("n_samples", [1, 63, 64, 65, 200])
def test_essentials_and_poses_equal_the_host_build_and_the_oracle(gpu, oracle, pool, n_samples):
    """rs_debug_essentials == host build in bit patterns and counts; rs_debug_poses == oracle.essential_poses of the device's
    own E bit for bit; unused slots hold no pose.  Solution counts 0 (rejected), 2, 4 and 6 share a wave."""
    a, b, samples = pool
    samples = samples[:n_samples]
    cons = gpu.EssentialConsensus(len(a), 10 * n_samples)
    cons.five_point_model_inliers(a, b, samples, 1e-6)
    E, n = cons.essentials(n_samples)
    poses, ok = cons.poses(10 * n_samples)
    cons.close()
    want_E, want_n = ck.essentials(a, b, samples, fill=0.0)
    assert np.array_equal(n, want_n), np.flatnonzero(n != want_n)
    assert np.array_equal(_bits(E), _bits(want_E))          # (unused slots: zero on both sides)
    if n_samples >= 63:
        first_wave = set(n[:63].tolist())
        assert {0, 2, 4, 6} <= first_wave, first_wave
    ok = ok.reshape(n_samples, 10, 4); poses = poses.reshape(n_samples, 10, 4, 3, 4)
    checked = 0
    for s in range(n_samples):
        assert np.all(ok[s, n[s]:] == 0), s
        for j in range(n[s]):
            want = oracle.essential_poses(E[s, j])
            if want is None:
                assert np.all(ok[s, j] == 0), (s, j)
                continue
            assert np.all(ok[s, j] != 0), (s, j)
            assert np.array_equal(_bits(poses[s, j]), _bits(want)), (s, j)
            checked += 1
    assert checked >= n_samples // 2


def test_five_point_batch_counts_winner_and_inliers(gpu, oracle, noisy, exhaustive):
    """Counts of every slot == oracle.pose_residual < thresh on the device's poses (exact: the scoring kernels are the
    existing ones); winner = most inliers, ties to the lowest id; inlier list ascending."""
    a, b, samples, thr = noisy
    pose, inl, best, counts, poses, ok = exhaustive
    L = oracle.lib()
    pa = [a[i].ctypes.data for i in range(len(a))]; pb = [b[i].ctypes.data for i in range(len(b))]
    flat = np.ascontiguousarray(poses.reshape(-1, 12)); okf = ok.reshape(-1); cf = counts.reshape(-1)
    want = np.zeros(len(flat), np.uint32)
    residual = L.orc_residual
    for pid in np.flatnonzero(okf):
        pp = flat[pid].ctypes.data
        want[pid] = sum(residual(pp, x, y, 1e-12, 1024) < thr for x, y in zip(pa, pb))
    assert np.array_equal(cf[okf != 0], want[okf != 0])
    assert np.all(cf[okf == 0] == 0)
    score = np.where(okf != 0, want.astype(np.int64), -1)
    want_best = int(np.argmax(score))            # argmax: the first of equal counts = lowest (sample, solution, pose)
    assert best == want_best
    assert np.array_equal(_bits(pose), _bits(flat[best].reshape(3, 4)))
    pp = flat[best].ctypes.data
    want_inl = [i for i in range(len(a)) if residual(pp, pa[i], pb[i], 1e-12, 1024) < thr]
    assert inl.tolist() == want_inl
    assert len(want_inl) >= 100                   # half of 300 are inliers of the true motion


def test_arrsac_with_the_bound_alone_equals_exhaustive_scoring(gpu, noisy, exhaustive):
    """rs_essential_arrsac + RS_ESTIMATOR_FIVE_POINT + RS_PRUNE_BOUND: winner, count and inlier set == the exhaustive call on
    the same samples — given, and drawn on the device and reproduced by rs_arrsac_samples(.., 5)."""
    a, b, samples, thr = noisy
    pose, inl, best, *_ = exhaustive
    cons = gpu.EssentialConsensus(len(a), 10 * len(samples))
    kw = dict(block_size=64, init_blocks=1, max_candidates=0, bound=True, sprt=False, estimator="five_point")
    got = cons.arrsac_model_inliers(a, b, thr, sample_idx=samples, **kw)
    assert got[2] == best and np.array_equal(_bits(got[0]), _bits(pose)) and got[1].tolist() == inl.tolist()
    assert got[3]["poses"] == 40 * len(samples)
    assert got[3]["residuals_evaluated"] < got[3]["residuals_exhaustive"]
    E, n = cons.essentials(len(samples))          # the tap follows the ARRSAC-shaped call too
    assert n.max() >= 2
    drawn = cons.arrsac_model_inliers(a, b, thr, n_hypotheses=len(samples), seed=9, **kw)
    same = gpu.EssentialConsensus.arrsac_samples(9, len(a), len(samples), sample_size=5)
    assert same.shape == (len(samples), 5) and all(len(set(r)) == 5 for r in same.tolist())
    want = cons.five_point_model_inliers(a, b, same, thr)
    assert drawn[2] == want[2] and np.array_equal(_bits(drawn[0]), _bits(want[0])) and drawn[1].tolist() == want[1].tolist()
    cons.close()


@pytest.mark.parametrize("shuffle", [False, True], ids=["in order", "shuffled"])
def test_batched_device_entry_equals_the_single_scene_call(gpu, oracle, shuffle):
    """rs_essential_arrsac_batch_device with the flag: 3 scenes, one with 4 matches (no model), estimations_per_block = 2;
    each scene == rs_essential_arrsac on rs_debug_scene's bearings in its scoring order with the scene's seed.  The same call
    without the flag is the eight-point one: == oracle.arrsac_pairs."""
    import torch
    from test_gpu_parity import _pixel_scene
    rng = np.random.default_rng(0x5B7C)
    cap, n_smp, seed, thr = 256, 24, 31, 2e-7
    cam = (984.2439, 980.8141, 690.0, 233.1966, 0.0, None)
    kw = dict(block_size=64, init_blocks=1, max_candidates=64, sprt=True, estimations_per_block=2)
    sizes = [200, 4, 120]
    S = len(sizes)
    scenes = [_pixel_scene(rng, cap, cap, n, 0.3, cam) for n in sizes]
    pairs = np.zeros((S, cap, 2), np.uint32)
    for s, n in enumerate(sizes):
        pairs[s, :n] = scenes[s][2]
    dev = torch.device("cuda", 0)
    d_ka = torch.from_numpy(np.stack([sc[0] for sc in scenes]).view(np.uint8).reshape(S, cap, 28)).to(dev)
    d_kb = torch.from_numpy(np.stack([sc[1] for sc in scenes]).view(np.uint8).reshape(S, cap, 28)).to(dev)
    d_pairs = torch.from_numpy(pairs.view(np.int32)).to(dev)
    d_np = torch.from_numpy(np.array(sizes, np.uint32).view(np.int32)).to(dev)
    d_pose = torch.zeros((S, 12), dtype=torch.float64, device=dev)
    d_best = torch.zeros((S,), dtype=torch.int32, device=dev)
    d_inl = torch.zeros((S, cap), dtype=torch.int32, device=dev)
    d_ninl = torch.zeros((S,), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    blocks_max = (cap + kw["block_size"] - 1) // kw["block_size"]
    slots = 10 * (n_smp + kw["estimations_per_block"] * blocks_max)
    cons = gpu.EssentialConsensus(cap, slots)
    cons.reserve(S)
    c = cons.camera(cam)
    single = gpu.EssentialConsensus(cap, slots)

    def run(estimator):
        prm = cons.make_params(thr, n_hypotheses=n_smp, seed=seed, estimator=estimator, **kw)
        cons.model_inliers_batch_device(d_ka.data_ptr(), d_kb.data_ptr(), cap, list(range(S)), list(range(S)), d_pairs.data_ptr(),
                                        d_np.data_ptr(), c, c, prm, d_pose.data_ptr(), d_best.data_ptr(), d_inl.data_ptr(),
                                        d_ninl.data_ptr(), None, shuffle=shuffle)
        cons.sync()
        return (d_pose.cpu().numpy().copy(), d_best.cpu().numpy().view(np.uint32).copy(), d_inl.cpu().numpy().view(np.uint32).copy(),
                d_ninl.cpu().numpy().view(np.uint32).copy())

    pose, best, inl, ninl = run("five_point")
    models = 0
    for s, n in enumerate(sizes):
        if n < 5:
            assert best[s] == 0xFFFFFFFF and ninl[s] == 0
            continue
        ga, gb, order = cons.scene(s, cap)
        order = order.astype(np.int64) if shuffle else np.arange(n)
        inv = np.empty(n, np.int64); inv[order] = np.arange(n)
        sseed = oracle.scene_seed(seed, s)
        samples = inv[gpu.EssentialConsensus.arrsac_samples(sseed, n, n_smp, sample_size=5).astype(np.int64)]
        want = single.arrsac_model_inliers(ga[order], gb[order], thr, sample_idx=samples.astype(np.uint32), seed=sseed,
                                           estimator="five_point", **kw)
        assert want is not None, s
        assert best[s] == want[2], (s, best[s], want[2])
        assert np.array_equal(_bits(pose[s].reshape(3, 4)), _bits(want[0])), s
        assert inl[s, :ninl[s]].tolist() == sorted(order[want[1].astype(np.int64)].tolist()), s
        models += 1
    assert models == 2
    # the same call without the flag: the eight-point result, as the specification gives it
    pose, best, inl, ninl = run("eight_point")
    for s, n in enumerate(sizes):
        want = oracle.arrsac_pairs(scenes[s][0], scenes[s][1], pairs[s, :n], cam, cam, thr, n_smp, scene=s, shuffle=shuffle, seed=seed, **kw)
        assert best[s] == want["best_id"], s
        assert ninl[s] == len(want["inliers"]), s
        if want["best_id"] != 0xFFFFFFFF:
            assert np.array_equal(_bits(pose[s].reshape(3, 4)), _bits(want["pose"])), s
            assert inl[s, :ninl[s]].tolist() == want["inliers"].tolist(), s
    cons.close(); single.close()


def test_refusals(gpu, noisy):
    from cv_amd import _lib
    a, b, samples, thr = noisy
    L = _lib.lib()
    cons = gpu.EssentialConsensus(len(a), 10 * len(samples) - 1)
    pose = np.zeros(12); best = C.c_uint32(); ninl = C.c_uint32(); inl = np.zeros(len(a), np.uint32)
    # fewer than ten slots per sample
    assert L.rs_five_point_batch(cons._h, a.ctypes.data, b.ctypes.data, len(a), samples.ctypes.data, len(samples), thr,
                                 pose.ctypes.data, C.byref(best), inl.ctypes.data, len(a), C.byref(ninl)) == -1
    prm = cons.make_params(thr, n_hypotheses=len(samples), block_size=64, init_blocks=1, max_candidates=0, sprt=False,
                           estimator="five_point")
    args = [cons._h, a.ctypes.data, b.ctypes.data, len(a), None, C.byref(prm), pose.ctypes.data, C.byref(best), inl.ctypes.data,
            len(a), C.byref(ninl), None]
    assert L.rs_essential_arrsac(*args) != 0
    prm.n_hypotheses = len(samples) - 1
    assert L.rs_essential_arrsac(*args) == 0
    # fewer than five matches: no model from the exhaustive entry, AKZ_E_INVALID from the ARRSAC-shaped one (as for 8)
    four = np.array([[0, 1, 2, 3, 3]], np.uint32)
    assert L.rs_five_point_batch(cons._h, a.ctypes.data, b.ctypes.data, 4, four.ctypes.data, 1, thr, pose.ctypes.data,
                                 C.byref(best), inl.ctypes.data, len(a), C.byref(ninl)) == 0
    assert best.value == 0xFFFFFFFF and ninl.value == 0
    # the P3P entry points refuse the flag; unknown bits and `reserved` stay refused
    world = np.concatenate([a, np.ones((len(a), 1))], axis=1)
    p3p = [cons._h, a.ctypes.data, world.ctypes.data, len(a), None, C.byref(prm), pose.ctypes.data, C.byref(best), inl.ctypes.data,
           len(a), C.byref(ninl), None]
    assert L.rs_p3p_arrsac(*p3p) == -1
    prm.flags &= ~_lib.RS_ESTIMATOR_FIVE_POINT
    assert L.rs_p3p_arrsac(*p3p) == 0
    prm.flags |= 1 << 7
    assert L.rs_essential_arrsac(*args) == -1
    prm.flags = _lib.RS_PRUNE_BOUND | _lib.RS_ESTIMATOR_FIVE_POINT
    prm.reserved = 1
    assert L.rs_essential_arrsac(*args) == -1
    # sample sizes
    out = np.zeros((4, 8), np.uint32)
    assert L.rs_arrsac_samples(1, 100, 4, 4, out.ctypes.data) == -1
    assert L.rs_arrsac_samples(1, 100, 4, 5, out.ctypes.data) == 0
    assert L.rs_arrsac_samples(1, 4, 4, 5, out.ctypes.data) == -1
    with pytest.raises(ValueError):
        cons.make_params(thr, estimator="seven_point")
    cons.close()


def test_batched_p3p_entry_refuses_the_flag(gpu):
    import torch
    from cv_amd import _lib
    dev = torch.device("cuda", 0)
    cons = gpu.EssentialConsensus(64, 640)
    prm = cons.make_params(1e-6, n_hypotheses=16, block_size=64, init_blocks=1, max_candidates=0, sprt=False, estimator="five_point")
    buf = torch.zeros(64 * 64, dtype=torch.float64, device=dev)
    cam = cons.camera((1000.0, 1000.0, 0.0, 0.0, 0.0, None))
    with pytest.raises(_lib.AkzError):
        cons.p3p_model_inliers_batch_device(buf.data_ptr(), 64, [0], buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), 8, cam, prm,
                                            buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), shuffle=False)
    cons.close()


def test_cpp_host_mirror_five_point(gpu, noisy, tmp_path):
    """arrsac::Arrsac::model_inliers(NisterStewenius) of include/akaze.hpp from a native process (tests/cpp/five_point.cpp):
    its output file == the ctypes path's bytes."""
    a, b, samples, thr = noisy
    exe = host_build.native(tmp_path, "five_point.cpp", hip=False)
    np.concatenate([a, b], axis=1).tofile(tmp_path / "matches.bin")
    n_hyp, seed, block = 64, 4242, 100
    r = subprocess.run([str(exe), str(tmp_path / "matches.bin"), str(tmp_path / "out.bin"), repr(thr), str(seed), str(n_hyp), str(block)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "five_point ok" in r.stdout
    cons = gpu.EssentialConsensus(len(a), 10 * n_hyp)
    got = cons.arrsac_model_inliers(a, b, thr, n_hypotheses=n_hyp, seed=seed, block_size=block, init_blocks=1, max_candidates=0,
                                    bound=True, sprt=True, sprt_delta=0.05, sprt_ratio=1e300, halve=True, estimations_per_block=0,
                                    estimator="five_point")
    cons.close()
    assert got is not None
    want = (np.array([1, len(got[1])], np.uint32).tobytes() + np.ascontiguousarray(got[0], np.float64).tobytes()
            + got[1].astype(np.uint32).tobytes())
    assert (tmp_path / "out.bin").read_bytes() == want


def test_an_exact_scene_recovers_the_motion(gpu):
    """No noise, no outliers: the winner's R and the direction of its t equal the truth to ten times the tolerance of the CPU
    test (the chain E -> SVD -> R, t adds its own conditioning)."""
    rng = np.random.default_rng(0xE8AC7)
    a, b, r, t, _ = st.scene(rng, n=60)
    samples = np.stack([rng.choice(60, 5, replace=False) for _ in range(16)]).astype(np.uint32)
    cons = gpu.EssentialConsensus(64, 160)
    pose, inl, best = cons.five_point_model_inliers(a, b, samples, 1e-12)
    cons.close()
    assert len(inl) == 60
    assert np.linalg.norm(pose[:, :3] - r) < 10 * TOL_E
    d = pose[:, 3] / np.linalg.norm(pose[:, 3])
    assert np.linalg.norm(d - t / np.linalg.norm(t)) < 10 * TOL_E


@pytest.mark.parametrize("then", ["batched p3p", "eight point"])
def test_essentials_tap_answers_only_for_the_last_five_point_call(gpu, then):
    """rs_debug_essentials reads the matrices of the last single-scene five-point call: after any other consensus call on the
    context — a valid one-scene rs_p3p_arrsac_batch_device, or rs_essential_batch — it refuses (AKZ_E_INVALID = -1) instead of
    returning the earlier call's matrices."""
    import torch
    from cv_amd import _lib
    from test_oracle_arrsac import _registration_scene
    rng = np.random.default_rng(0xE8AC7)
    a, b, r, t, _ = st.scene(rng, n=60)
    samples = np.stack([rng.choice(60, 5, replace=False) for _ in range(16)]).astype(np.uint32)
    cons = gpu.EssentialConsensus(64, 160)
    cons.reserve(1)
    assert cons.five_point_model_inliers(a, b, samples, 1e-12) is not None
    E, n = cons.essentials(16)
    assert n.max() >= 1
    if then == "batched p3p":
        cap, n_world = 64, 80
        cam = (950.0, 955.0, 640.0, 250.0, 0.0, None)
        kps, world, pr, *_ = _registration_scene(rng, cap, n_world, 48, 0.3, cam)
        pairs = np.zeros((1, cap, 2), np.uint32)
        pairs[0, :len(pr)] = pr
        dev = torch.device("cuda", 0)
        d_k = torch.from_numpy(kps.view(np.uint8).reshape(1, cap, 28)).to(dev)
        d_pairs = torch.from_numpy(pairs.view(np.int32)).to(dev)
        d_np = torch.from_numpy(np.array([len(pr)], np.uint32).view(np.int32)).to(dev)
        d_world = torch.from_numpy(world).to(dev)
        d_pose = torch.zeros((1, 12), dtype=torch.float64, device=dev)
        d_best = torch.zeros((1,), dtype=torch.int32, device=dev)
        d_inl = torch.zeros((1, cap), dtype=torch.int32, device=dev)
        d_ninl = torch.zeros((1,), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        prm = cons.make_params(1e-6, n_hypotheses=16, seed=5)
        cons.p3p_model_inliers_batch_device(d_k.data_ptr(), cap, [0], d_pairs.data_ptr(), d_np.data_ptr(), d_world.data_ptr(), n_world,
                                            cons.camera(cam), prm, d_pose.data_ptr(), d_best.data_ptr(), d_inl.data_ptr(),
                                            d_ninl.data_ptr(), shuffle=False)
        cons.sync()
        assert int(d_ninl.cpu().numpy().view(np.uint32)[0]) <= len(pr)
    else:
        eight = np.stack([rng.choice(60, 8, replace=False) for _ in range(16)]).astype(np.uint32)
        assert cons.model_inliers(a, b, eight, 1e-12) is not None
    out_E = np.zeros((1, 10, 9), np.float64); out_n = np.zeros(1, np.uint32)
    assert _lib.lib().rs_debug_essentials(cons._h, out_E.ctypes.data, out_n.ctypes.data, 1) == -1
    cons.close()
