"""The single-view refinement kernel (cv_amd/csrc/rs_single_view.hip) against the host build of the same header
(tests/single_view_checker.py): every output buffer is compared in bytes, WHOLE — what a call does not write keeps the pattern
it was filled with on both sides, so the rows behind the valid ones and the outputs of refused scenes are held untouched by the
same comparison.  Run with -m gpu.

Shapes: cap_per_img 512, a dozen views, patience <= 400.  The partial sums and the ordered compaction work 256 matches at a
time in waves of 64: the original-match counts cross both edges; the selection cut falls inside a block (100) and on its edge
(256); one scene fills the whole LDS layout (2 100 robust matches under the default 2 048)."""
import numpy as np
import pytest

import single_view_checker as V

pytestmark = pytest.mark.gpu

FILL8 = 0xA5
RATE = 0.02          # the reference's 1e-3 needs thousands of iterations; the stop rules are the same at any rate
OUT = ("pose_out", "verdict", "final", "n_final", "stats")


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
    c.reserve(16)
    yield c
    c.close()


def device_params(st):
    from cv_amd.single_view import SingleViewRefiner
    return SingleViewRefiner.params(**V.settings_dict(st))


def device_refine(torch, cons, b, st):
    """rs_refine_poses_batch_device on a Batch -> dict of the five output buffers, and the pattern they were filled with"""
    from cv_amd import _lib
    from cv_amd.single_view import SingleViewRefiner
    dev = torch.device("cuda", 0)
    up = lambda a: _lib.device_bytes(torch, a, dev)
    S = len(b.rigs)
    d_in = [up(x) for x in (b.kps.view(np.uint8), b.poses, b.obs_start, b.obs, b.world, b.matches, b.nmatches, b.pose, b.best_id, b.inliers,
                            b.n_inliers)]
    d_best = None if b.best is None else up(b.best)
    size = dict(pose_out=96 * S, verdict=4 * S, final=b.cap * S, n_final=4 * S, stats=4 * V.STATS * S)
    d = {k: torch.full((n,), FILL8, dtype=torch.uint8, device=dev) for k, n in size.items()}
    p = [t.data_ptr() for t in d_in]
    SingleViewRefiner(cons).refine_batch_device(
        p[0], b.cap, b.n_blocks, p[1], V.rig_camera_dev(), p[2], p[3] if b.n_obs else None, b.n_obs, b.n_landmarks, p[4], b.n_world,
        [int(x) for x in b.ik], p[5], p[6], None if d_best is None else d_best.data_ptr(), p[7], p[8], p[9], p[10], device_params(st),
        d["pose_out"].data_ptr(), d["verdict"].data_ptr(), d["final"].data_ptr(), d["n_final"].data_ptr(), d["stats"].data_ptr(),
        _lib.wait_handle(torch.cuda.current_stream(dev)))
    cons.sync()
    h = {k: v.cpu().numpy() for k, v in d.items()}
    return dict(pose_out=h["pose_out"].view(np.float64).reshape(S, 12), verdict=h["verdict"].view(np.uint32), final=h["final"].reshape(S, b.cap),
                n_final=h["n_final"].view(np.uint32), stats=h["stats"].view(np.uint32).reshape(S, V.STATS))


def check(torch, cons, b, st):
    """device == host build in every byte of every output buffer -> the host result"""
    S = len(b.rigs)
    got = device_refine(torch, cons, b, st)
    prior_pose = np.full(96 * S, FILL8, np.uint8).view(np.float64).reshape(S, 12)
    want = b.host(st, prior_pose, np.full((S, b.cap), FILL8, np.uint8))
    for k in OUT:
        g, w = np.ascontiguousarray(got[k]).view(np.uint8).reshape(S, -1), np.ascontiguousarray(want[k]).view(np.uint8).reshape(S, -1)
        if not np.array_equal(g, w):
            bad = np.flatnonzero((g != w).any(1))
            raise AssertionError((k, bad[:10], got[k][bad[:2]], want[k][bad[:2]], want["verdict"], want["stats"][bad[:2]]))
    return want


def small(**kw):
    return V.settings(single_view_optimization_rate=RATE, single_view_patience=120, single_view_filter_loop_iterations=2,
                      single_view_minimum_landmarks=0, single_view_minimum_robust_landmarks=1, **kw)


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 255, 256, 257, 300])
def test_original_match_counts_around_a_wave_and_a_block(gpu, cons, n):
    r = V.Rig(100 + n, n, none=[k for k in (1, 70, 200) if k < n])
    h = check(gpu, cons, V.Batch([r], 512), small())
    if n >= 1:
        assert h["verdict"][0] == V.OK and h["n_final"][0] == n and h["stats"][0, V.S_ROBUST] == n - int(r.none.sum())
    else:
        assert h["verdict"][0] == V.LOST_HALF            # 0 <= 0 / 2


@pytest.mark.parametrize("num", [100, 256])
def test_the_selection_cuts_inside_a_block_and_at_its_edge(gpu, cons, num):
    r = V.Rig(7, 300, none=(3, 120), outliers=(5, 50, 99, 130, 255))
    h = check(gpu, cons, V.Batch([r], 512), small(single_view_optimization_num_matches=num))
    assert h["verdict"][0] == V.OK and list(h["stats"][0, V.S_RUN_MATCHES:V.S_RUN_MATCHES + 3]) == [num] * 3
    assert h["stats"][0, V.S_INLIERS] == num and h["n_final"][0] == 295


def test_the_full_lds_layout(gpu, cons):
    """2 100 robust matches (and 20 without a world point) at cap 4 096 under the default 2 048, patience 60"""
    r = V.Rig(11, 2120, none=range(50, 2050, 100))
    st = V.settings(single_view_optimization_rate=RATE, single_view_patience=60)
    h = check(gpu, cons, V.Batch([r], 4096), st)
    assert h["verdict"][0] == V.OK and h["stats"][0, V.S_INLIERS] == 2048 and list(h["stats"][0, V.S_RUN_MATCHES:V.S_RUN_MATCHES + 6]) == [2048] * 6
    assert h["n_final"][0] == 2120 and h["stats"][0, V.S_ROBUST] == 2100


def test_observation_counts_and_match_kinds(gpu, cons):
    """landmarks with 0, 1, 2, 3 and 40 other observations; merged matches (1 + 1, 2 + 2, 3 + 40 observations); "None" rows"""
    n = 200
    counts = np.r_[0, 1, 2, 3, 40, 1, 2, 3, 1 + np.arange(n - 8) % 5]
    r = V.Rig(21, n, obs_counts=counts, merged=(5, 6, 7, 90), merged_second=2, none=(2, 6, 150), outliers=(1, 4, 60))
    r2 = V.Rig(22, n, obs_counts=counts, merged=(5, 7), merged_second=1, none=(9,))
    h = check(gpu, cons, V.Batch([r, r2], 512), small())
    assert list(h["verdict"]) == [V.OK, V.OK] and list(h["stats"][:, V.S_NO_OTHER]) == [1, 1]
    # no other observation: never consistent.  Matches 1 and 4 are 20 - 40 px off: the pair test of a single other observation
    # (a sine distance of 1e-1) lets that pass, the 40 other observations of match 4 do not
    assert not h["final"][0, 0] and h["final"][0, 1] and not h["final"][0, 4] and not h["final"][0, 60]
    assert h["final"][0, 2] and h["final"][0, 5] and h["final"][0, 6] and h["final"][0, 7] and h["final"][0, 90]


def mixture():
    many = list(range(0, 200, 3)) + list(range(1, 200, 3))            # two thirds of the matches are 20 - 40 px off
    rigs = [V.Rig(31, 200),                                           # 0 ok
            V.Rig(32, 200, has_model=False),                          # 1 no model
            V.Rig(33, 200),                                           # 2 bad index: a feature == cap
            V.Rig(34, 20),                                            # 3 few landmarks
            V.Rig(35, 200, outliers=many),                            # 4 lost half, entering a run
            V.Rig(36, 40),                                            # 5 few robust
            V.Rig(37, 200),                                           # 6 bad index: an inlier beyond the robust list
            V.Rig(38, 200, none=(0, 1)),                              # 7 bad index: an observation in block n_blocks
            V.Rig(39, 200, merged=(4,)),                              # 8 bad index: a world row == n_rows
            V.Rig(40, 200)]                                           # 9 ok
    b = V.Batch(rigs, 512)
    b.matches[2, 17, 0] = 512
    b.inliers[6, 5] = 200
    o = int(b.obs_start[sum(r.n_landmarks for r in rigs[:7]) + 30])
    b.obs[o, 0] = b.n_blocks
    b.matches[8, 100, 1] = b.n_rows
    return b


def test_a_batch_of_every_verdict(gpu, cons):
    """an OK scene, a no-model scene, bad indices of four kinds and each rejecting verdict side by side: a refused scene changes
    nothing in its neighbours"""
    st = V.settings(single_view_optimization_rate=RATE, single_view_patience=100, single_view_filter_loop_iterations=2)
    h = check(gpu, cons, mixture(), st)
    assert list(h["verdict"]) == [V.OK, V.NO_MODEL, V.BAD_INDEX, V.FEW_LANDMARKS, V.LOST_HALF, V.FEW_ROBUST, V.BAD_INDEX, V.BAD_INDEX, V.BAD_INDEX,
                                  V.OK]
    assert h["stats"][4, V.S_STAGE] == V.STAGE_RUN0 + 1 and h["stats"][5, V.S_STAGE] == V.STAGE_MINIMUM


@pytest.mark.parametrize("loops, stage", [(1, V.STAGE_RUN0 + 1), (0, V.STAGE_FINAL)])
def test_lost_half_at_the_last_run_and_at_the_final_count(gpu, cons, loops, stage):
    many = list(range(0, 200, 3)) + list(range(1, 200, 3))
    b = V.Batch([V.Rig(35, 200, outliers=many), V.Rig(41, 200)], 512)
    h = check(gpu, cons, b, V.settings(single_view_optimization_rate=RATE, single_view_patience=100, single_view_filter_loop_iterations=loops))
    assert list(h["verdict"]) == [V.LOST_HALF, V.OK] and h["stats"][0, V.S_STAGE] == stage


def test_both_breaks_of_the_optimiser(gpu, cons):
    """patience 400: the first run ends at its last iteration, a later one after 50 iterations without improvement; and the
    patiences 0 and 1"""
    r = V.Rig(1, 300)
    b = V.Batch([r], 512)
    h = check(gpu, cons, b, V.settings(single_view_optimization_rate=RATE, single_view_patience=400))
    stops = h["stats"][0, V.S_RUN_STOP:V.S_RUN_STOP + 6]
    assert stops[0] == 399 and (stops < 399).any() and h["verdict"][0] == V.OK
    for patience in (0, 1):
        h = check(gpu, cons, b, V.settings(single_view_patience=patience))
        assert list(h["stats"][0, V.S_RUN_STOP:V.S_RUN_STOP + 6]) == [0] * 6 and h["verdict"][0] == V.OK
    assert np.array_equal(check(gpu, cons, b, V.settings(single_view_patience=0))["pose_out"][0], r.pose_in.reshape(12))


def test_the_native_mirror(gpu, cons, tmp_path):
    """cv_sfm::SingleViewRefiner of include/akaze.hpp from a native process gives the host build's outputs"""
    import subprocess

    import host_build
    b = V.Batch([V.Rig(51, 150, merged=(3,), none=(7,), outliers=(9, 10)), V.Rig(52, 40), V.Rig(53, 150, has_model=False)], 512)
    st = V.settings(single_view_optimization_rate=RATE, single_view_patience=100, single_view_filter_loop_iterations=2)
    S = len(b.rigs)
    want = b.host(st, np.full(96 * S, FILL8, np.uint8).view(np.float64).reshape(S, 12), np.full((S, b.cap), FILL8, np.uint8))
    path = tmp_path / "batch.bin"
    with open(path, "wb") as fp:
        fp.write(np.array([b.n_blocks, b.cap, b.n_landmarks, b.n_obs, b.n_world, b.n_rows, S, 1, 100, 2], np.uint32).tobytes())
        fp.write(np.array([RATE]).tobytes())
        fp.write(bytes(V.rig_camera_dev()))
        for a in (b.kps, b.poses, b.obs_start, b.obs[:b.n_obs], b.world[:b.n_rows], b.ik, b.matches, b.nmatches, b.best, b.pose, b.best_id,
                  b.inliers, b.n_inliers):
            fp.write(np.ascontiguousarray(a).tobytes())
    exe = host_build.native(tmp_path, "single_view.cpp", hip=True)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("single_view ok"), (r.returncode, r.stderr[-400:])
    lines = r.stdout.splitlines()
    for s in range(S):
        head = np.array(lines[3 * s].split()[1:], np.int64)
        assert head[0] == s and head[1] == want["verdict"][s] and head[2] == want["n_final"][s] and np.array_equal(head[3:], want["stats"][s])
        pose = np.array([int(x, 16) for x in lines[3 * s + 1].split()[1:]], np.uint64)
        assert np.array_equal(pose, want["pose_out"][s].view(np.uint64))
        final = np.array(lines[3 * s + 2].split()[1:], np.int64)
        assert np.array_equal(final, want["final"][s, :b.rigs[s].n])
    assert list(want["verdict"]) == [V.OK, V.FEW_ROBUST, V.NO_MODEL]


def test_registration_consensus_then_refine(gpu):
    """Registration.consensus -> refine on one small batch, no host step between them: the original matches are the lists of
    the consensus before its drop, and the refinement equals the host build fed with what the device consensus left (its
    pose, id and inliers: the consensus itself is held to its oracle elsewhere)."""
    torch = gpu
    from cv_amd.registration import Registration
    rigs = [V.Rig(61, 200, none=(4, 90)), V.Rig(62, 180, merged=(5, 6), none=(8,), outliers=(11, 12, 13)), V.Rig(63, 120)]
    b = V.Batch(rigs, 512)
    S, cap = len(rigs), b.cap
    best = np.full((S, cap, 3, 2), V.NO_ID, np.uint32)
    decision, merge_ok = np.zeros((S, cap), np.uint32), np.zeros((S, cap), np.uint8)
    counts = np.zeros(b.n_blocks, np.uint32)
    for s, r in enumerate(rigs):
        rows = b.matches[s, :r.n, 1]
        best[s, :r.n, 0, 0] = np.where(r.merged, b.best[s, :r.n, 0, 0], rows)
        best[s, :r.n, 1, 0] = np.where(r.merged, b.best[s, :r.n, 1, 0], V.NO_ID)
        best[s, :r.n, :, 1] = (10, 50, 90)
        decision[s, :r.n] = np.where(r.merged, 2, 1)
        merge_ok[s, :r.n] = r.merged
        counts[b.ik[s]] = r.n
    b.best = best
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    cw = np.random.default_rng(1).integers(0, 256, (32, 64), dtype=np.uint8)
    reg = Registration(torch, cap, S, 2, cw, (V.CAM["fx"], V.CAM["fy"], V.CAM["cx"], V.CAM["cy"], 0.0, None), n_hypotheses=512, max_candidates=64,
                       estimations_per_block=0, block_size=64)
    try:
        # what match_views() leaves, set by hand: the matcher's search is not what this test is about
        reg._cur, reg._fb, reg._calls = reg._sets[0], np.asarray(b.ik, np.uint32), 1
        reg.best.copy_(t(best.view(np.int32)))
        reg.decision.copy_(t(decision.view(np.int32)))
        d_kps, d_counts, d_world = t(b.kps.view(np.uint8).reshape(b.n_blocks, cap, 28)), t(counts.view(np.int32)), t(b.world)
        d_poses, d_start, d_obs = t(b.poses), t(b.obs_start.view(np.int32)), t(b.obs.view(np.int32))
        torch.cuda.synchronize()
        reg.consensus(d_kps, d_counts, d_world, b.n_world, d_merge_ok=t(merge_ok))
        st = V.settings(single_view_optimization_rate=RATE, single_view_patience=100, single_view_filter_loop_iterations=2)
        out = reg.refine(d_poses, d_start, d_obs, b.n_landmarks, params=device_params(st), stream=torch.cuda.current_stream(dev))
        reg.sync()
        originals, n_orig = reg.originals.cpu().numpy().view(np.uint32), reg.noriginals.cpu().numpy().view(np.uint32)
        pairs, n_pairs = reg.pairs.cpu().numpy().view(np.uint32), reg.npairs.cpu().numpy().view(np.uint32)
        for s, r in enumerate(rigs):
            assert n_orig[s] == r.n and np.array_equal(originals[s, :r.n], b.matches[s, :r.n])
            assert n_pairs[s] == int((~r.none).sum()) and np.array_equal(pairs[s, :n_pairs[s]], b.matches[s, :r.n][~r.none])
        b.pose = reg.pose.cpu().numpy()[:S].copy()
        b.best_id = reg.best_id.cpu().numpy().view(np.uint32)[:S].copy()
        b.inliers = reg.inliers.cpu().numpy().view(np.uint32)[:S].copy()
        b.n_inliers = reg.n_inliers.cpu().numpy().view(np.uint32)[:S].copy()
        assert (b.best_id != V.NO_ID).all() and (b.n_inliers > 100).all()
        want = b.host(st, np.zeros((S, 12)), np.zeros((S, cap), np.uint8))
        pose, verdict, final, n_final, stats = out.host()
        assert np.array_equal(verdict[:S], want["verdict"]) and list(verdict[:S]) == [V.OK] * 3
        assert pose[:S].tobytes() == want["pose_out"].tobytes() and np.array_equal(final[:S], want["final"].astype(bool))
        assert np.array_equal(n_final[:S], want["n_final"]) and np.array_equal(stats[:S], want["stats"])
    finally:
        reg.close()
