"""The kernels that start a reconstruction (cv_amd/csrc/rs_bootstrap_table.hip) against the host build of the same header
(tests/bootstrap_table_checker.py): every output buffer is compared in bytes, WHOLE — both sides start from the same fill
pattern, so a word a call should have written and did not shows, and so does one it should have left alone.  Then the chain
reconstruction.start_reconstructions against the existing host path on the same device results, and cv_sfm::ReconstructionStart
from a native process.  Run with -m gpu.

Shapes: the join walks a list 1024 entries at a time (one workgroup of 1024 per scene; lists of 1023 / 1024 / 1025 inliers at cap
2048), cap 64 and 256 with lists of 0, 1, 63, 64, 65 and cap entries; add_reconstruction walks matches and features 256 at a
time and scans a scene's centre rows in tiles of T = RS_LT_TILE rows (centre counts and scene totals of T - 1, T, T + 1)."""
import numpy as np
import pytest

import bootstrap_table_checker as K
import bootstrap_table_statement as S

pytestmark = pytest.mark.gpu
T = K.TILE


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


def _run(torch, inp, in_names, want, out_names, launch):
    from cv_amd import _lib
    dev = torch.device("cuda", 0)
    up = lambda a: None if a is None else _lib.device_bytes(torch, a, dev)
    d_in = {k: up(inp[k]) for k in in_names}
    d = {k: up(want[k]) for k in out_names}                              # the host's fill, byte for byte
    launch(d_in, d, _lib.wait_handle(torch.cuda.current_stream(dev)))
    return {k: d[k].cpu().numpy().view(want[k].dtype).reshape(want[k].shape) for k in out_names}


def device_join(torch, cons, inp):
    """rs_join_pairs_batch_device on the arrays of a call -> dict of the output buffers as the host checker shapes them"""
    from cv_amd.bootstrap import PairJoin

    def launch(i, o, wait):
        PairJoin(cons).join_device(i["pairs"], i["npairs"], i["inliers"], i["n_inliers"], i["best_id"], i["pose"], inp["n_slots"], inp["cap"],
                                   inp["slot_first"], inp["slot_second"], *(o[k] for k in K.JOIN_OUTPUT_NAMES), minimum=inp["minimum"],
                                   shuffle=bool(inp["flags"]), seed=inp["seed"], stream_to_wait=wait)
        cons.sync()
    return _run(torch, inp, ("pairs", "npairs", "inliers", "n_inliers", "best_id", "pose"), K.join_outputs(inp), K.JOIN_OUTPUT_NAMES, launch)


ADD_INPUTS = ("triples", "ntriples", "first_only", "nfirst", "second_only", "nsecond", "combined", "first_ok", "second_ok", "pose_out", "tv_verdict",
              "kps", "counts", "skip", "obs_start", "obs", "recon_start", "view_start")


def device_add(torch, cons, inp, same_pool=False):
    """rs_add_reconstruction_batch_device on the arrays of a call -> dict of the output buffers as the host checker shapes them.
    same_pool: the destination pool IS the source pool (n_blocks == n_src_blocks)."""
    from cv_amd.bootstrap import ReconstructionStart

    def launch(i, o, wait):
        if same_pool:
            o["kps_dst"] = i["kps"]
        ReconstructionStart(cons).add_device(
            *(i[k] for k in ADD_INPUTS[:11]), inp["ic"], inp["i_first"], inp["i_second"], i["kps"], i["counts"], inp["n_src_blocks"], inp["cap"],
            i["skip"], i["obs_start"], i["obs"] if inp["n_obs"] else None, inp["n_obs"], inp["n_landmarks"], i["recon_start"], i["view_start"],
            inp["n_recons"], o["kps_dst"], o["counts_dst"], o["poses"], inp["n_blocks"], inp["view_base"], inp["obs_room"], inp["lm_room"],
            *(o[k] for k in K.ADD_OUTPUT_NAMES[3:]), stream_to_wait=wait)
        cons.sync()
    return _run(torch, inp, ADD_INPUTS, K.add_outputs(inp), K.ADD_OUTPUT_NAMES, launch)


def assert_same(got, want, names):
    for k in names:
        g, w = got[k].view(np.uint8).reshape(len(want[k]), -1), want[k].view(np.uint8).reshape(len(want[k]), -1)
        if not np.array_equal(g, w):
            bad = np.flatnonzero((g != w).any(1))
            raise AssertionError((k, len(bad), bad[:10], got[k][bad[:4]], want[k][bad[:4]]))


def check_join(torch, cons, inp):
    want = K.join(inp)
    assert_same(device_join(torch, cons, inp), want, K.JOIN_OUTPUT_NAMES)
    return want


def check_add(torch, cons, inp):
    want = K.add(inp)
    assert_same(device_add(torch, cons, inp), want, K.ADD_OUTPUT_NAMES)
    return want


# ---- the join ----
@pytest.mark.parametrize("shuffle", [False, True])
@pytest.mark.parametrize("cap", [64, 256])
def test_join_list_lengths(gpu, cons, cap, shuffle):
    """lists of 0, 1, 63, 64, 65 and cap inliers, every length against every other; half as many centre features as pairs, so
    that a centre feature occurs twice in a list"""
    rng = np.random.default_rng(cap)
    lengths = (0, 1, 63, 64, min(65, cap), cap)
    slots = [K.drawn_slot(rng, cap, cap, n, centres=cap // 2) for n in lengths]
    want = check_join(gpu, cons, K.join_inputs(slots, [(a, b) for a in range(6) for b in range(6)], cap, shuffle=shuffle, seed=0x1234567890ABCDEF))
    assert (want["verdict"] == K.JP_OK).all() and want["ntriples"].max() > cap // 2
    if cap == 64:                                                         # small enough to walk: the statement too
        inp = K.join_inputs(slots, [(a, b) for a in range(6) for b in range(6)], cap, shuffle=shuffle, seed=0x1234567890ABCDEF)
        assert K.same(want, S.join(inp, K.join_outputs(inp)), K.JOIN_OUTPUT_NAMES) == []


@pytest.mark.parametrize("shuffle", [False, True])
def test_join_across_the_workgroup_size(gpu, cons, shuffle):
    rng = np.random.default_rng(2048)
    slots = [K.drawn_slot(rng, 2048, 2048, n, centres=1500) for n in (1023, 1024, 1025)]
    want = check_join(gpu, cons, K.join_inputs(slots, [(a, b) for a in range(3) for b in range(3)], 2048, minimum=1000, shuffle=shuffle, seed=99))
    assert (want["verdict"] == K.JP_OK).all() and want["ntriples"].min() > 300 and want["nfirst"][1] > 100


@pytest.mark.parametrize("n_scenes, at", [(1, 0), (2, 0), (2, 1), (9, 0), (9, 4), (9, 8)])
def test_join_refusals(gpu, cons, n_scenes, at):
    """every refusal class first, in the middle and last among good scenes: outputs equal the host build's, the bytes of a refused
    scene's lists and those behind every count untouched"""
    cap = 64
    rng = np.random.default_rng(n_scenes * 10 + at)
    good = [K.drawn_slot(rng, cap, 60, 40 + k, centres=50) for k in range(3)]
    bad = [K.drawn_slot(rng, cap, 60, 40, best_id=K.NONE), K.drawn_slot(rng, cap, 60, 7), K.drawn_slot(rng, cap, 60, 40, npairs=cap + 1),
           dict(K.drawn_slot(rng, cap, 60, 40), n_inliers=cap + 1), K.drawn_slot(rng, cap, 60, 40, npairs=30),
           K.slot([(k, cap if k == 17 else k) for k in range(40)]), K.slot([(cap + 5 if k == 39 else k, k) for k in range(40)])]
    verdicts = (K.JP_NO_MODEL, K.JP_FEW_INLIERS, K.JP_BAD_INDEX, K.JP_BAD_INDEX, K.JP_BAD_INDEX, K.JP_BAD_INDEX, K.JP_BAD_INDEX)
    for k, v in enumerate(verdicts):
        for side in (0, 1):
            scenes = [(s % 3, (s + 1) % 3) for s in range(n_scenes)]
            scenes[at] = (3 + k, 0) if side == 0 else (1, 3 + k)
            want = check_join(gpu, cons, K.join_inputs(good + bad, scenes, cap, minimum=8, shuffle=bool(side), seed=5))
            assert want["verdict"].tolist() == [v if s == at else K.JP_OK for s in range(n_scenes)], (k, side)


# ---- add_reconstruction ----
def drawn_call(seed, cap, n_scenes, refused=None, how=None, table=None, **kw):
    """n_scenes valid scenes over distinct source blocks; scene `refused` broken in the way `how`"""
    rng = np.random.default_rng(seed)
    scenes = []
    for s in range(n_scenes):
        counts = tuple(int(c) for c in rng.integers(cap // 2, cap + 1, 3))
        lists = tuple(int(v) for v in rng.integers(1, cap // 6, 3))
        extra = {}
        if s == refused:
            extra = dict(skip=dict(skip=1), verdict=dict(verdict=K.TV_FEW_ROBUST)).get(how, {})
        sc = K.drawn_scene(rng, (3 * s + 1, 3 * s, 3 * s + 2), counts, cap, lists, keep=0.7, **extra)
        if s == refused and how == "duplicate":
            sc["lists"][1].append((sc["lists"][0][0][0], int(counts[1]) - 1))     # a centre feature of a triple in a first-only pair
            sc["masks"][1].append(1)
            sc["masks"][0][0] = 1
            sc["n"][1] += 1
        if s == refused and how == "range":
            sc["lists"][2].append((0, counts[2]))
            sc["masks"][2].append(1)
            sc["n"][2] += 1
        if s == refused and how == "taken":
            sc["blocks"] = (sc["blocks"][0], 0, sc["blocks"][2])                 # scene 0's first frame
            sc["counts"] = (counts[0], scenes[0]["counts"][1], counts[2])
            sc = K.drawn_scene(rng, sc["blocks"], sc["counts"], cap, (1, 1, 1))
        scenes.append(sc)
    n_blocks = 3 * n_scenes + 5
    return K.add_inputs(scenes, cap, 3 * n_scenes, n_blocks, 4, table=table, extra_room=7, seed=seed, **kw)


@pytest.mark.parametrize("cap", [64, 256])
@pytest.mark.parametrize("n_scenes, refused", [(1, None), (1, 0), (2, 0), (2, 1), (9, 0), (9, 4), (9, 8)])
def test_add_reconstruction_scenes(gpu, cons, cap, n_scenes, refused):
    for how in ((None,) if refused is None else ("skip", "verdict", "duplicate", "range") + (("taken",) if refused else ())):
        inp = drawn_call(cap * 100 + n_scenes * 10 + (refused or 0), cap, n_scenes, refused, how)
        want = check_add(gpu, cons, inp)
        expect = dict(skip=K.AR_NOT_ACCEPTED, verdict=K.AR_NOT_ACCEPTED, duplicate=K.AR_BAD_INDEX, range=K.AR_BAD_INDEX, taken=K.AR_TAKEN).get(how)
        assert want["frame_verdict"].tolist() == [expect if s == refused else K.AR_OK for s in range(n_scenes)], how
        assert want["call_verdict"][0] == K.AR_OK and want["counts_out"][3] == n_scenes - (refused is not None)
        if cap == 64 and n_scenes <= 2:                                   # small enough to walk: the statement too
            assert K.same(want, S.add_reconstruction(inp, K.add_outputs(inp)), K.ADD_OUTPUT_NAMES) == []


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_add_reconstruction_tile_boundaries(gpu, cons, delta):
    """a tile boundary inside one scene's centre rows (T + delta centre features) and between two scenes (a scene of T + delta
    rows in front of another)"""
    cap = 2048
    rng = np.random.default_rng(delta + 5)
    inside = K.drawn_scene(rng, (0, 1, 2), (T + delta, 700, 300), cap, (200, 100, 50), keep=0.8)
    # rows = 900 + (100 - 20) + (60 + delta - 16) = T + delta
    between = K.drawn_scene(rng, (3, 4, 5), (900, 100, 60 + delta), cap, (10, 10, 6), keep=1.0)
    last = K.drawn_scene(rng, (6, 7, 8), (2048, 2048, 2048), cap, (1000, 500, 500), keep=0.9)
    want = check_add(gpu, cons, K.add_inputs([between, inside, last], cap, 9, 10, 1, extra_room=3))
    assert want["stats"][0, 3] == T + delta and want["recon_start_out"][1] == T + delta and (want["frame_verdict"] == K.AR_OK).all()


def numpy_table(seed, n_landmarks, n_views, cap):
    """n_landmarks lists of 0 .. 3 observations over n_views blocks, every {block, feature} once"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 4, n_landmarks)
    start = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    n = int(start[-1])
    row_of = np.repeat(np.arange(n_landmarks), lens)
    blocks = (row_of * 7 + (np.arange(n) - start[row_of])) % n_views
    order = np.argsort(blocks, kind="stable")
    feats = np.empty(n, np.int64)
    feats[order] = np.arange(n) - np.searchsorted(blocks[order], blocks[order], "left")
    assert feats.max() < cap
    obs = np.full((n + 3, 2), K.FILL32, np.uint32)
    obs[:n] = np.stack([blocks, feats], 1)
    return start, obs, n + 3


@pytest.mark.parametrize("what", ["good", "starts", "recon_end", "view_end"])
def test_add_reconstruction_behind_a_table_of_1025_rows(gpu, cons, what):
    cap = 512
    start, obs, n_obs = numpy_table(3, T + 1, 4, cap)
    recon, views = [0, 400, T + 1], [0, 2, 4]
    if what == "starts":
        start = start.copy()
        start[T - 1] = start[T] + 1
    elif what == "recon_end":
        recon[2] = T
    elif what == "view_end":
        views[2] = 3
    inp = drawn_call(17, cap, 3, table=(start, obs, n_obs), recon_start=recon, view_start=views)
    want = check_add(gpu, cons, inp)
    assert want["call_verdict"][0] == (K.AR_OK if what == "good" else K.AR_BAD_TABLE)
    assert want["counts_out"][3] == (3 if what == "good" else 0) and want["recon_start_out"][:3].tolist() == recon


def test_add_reconstruction_inside_one_pool(gpu, cons):
    """the destination pool is the source pool: the views lie behind the source blocks"""
    cap = 64
    rng = np.random.default_rng(8)
    scenes = [K.drawn_scene(rng, (2, 0, 1), (60, 64, 33), cap, (9, 5, 5)), K.drawn_scene(rng, (3, 5, 4), (64, 1, 50), cap, (1, 0, 7))]
    inp = K.add_inputs(scenes, cap, 12, 12, 6)
    want = K.add(inp)
    got = device_add(gpu, cons, inp, same_pool=True)
    pool = inp["kps"].copy()
    pool[6:12] = want["kps_dst"][6:12]
    want["kps_dst"] = pool
    assert_same(got, want, K.ADD_OUTPUT_NAMES)
    assert (want["frame_verdict"] == K.AR_OK).all()


# ---- the chain ----
def synthetic_views(seed, n_points=200, cap=256):
    """three views of n_points points (three_view_checker.Rig: 3 - 9 units deep, half a pixel of noise), the points in a different
    order in each view: keypoints (centre, first, second) [cap] KP_DTYPE and the feature of every point in every view"""
    import three_view_checker as R
    rng = np.random.default_rng(seed)
    rig = R.Rig(seed, n_points, noise=0.5)
    kps = np.zeros((3, cap), R.KP_DTYPE)
    feature = np.zeros((3, n_points), np.int64)
    for v in range(3):
        order = rng.permutation(n_points)
        kps["x"][v, :n_points], kps["y"][v, :n_points] = rig.px[v][order, 0], rig.px[v][order, 1]
        kps["size"][v] = 4.0
        feature[v, order] = np.arange(n_points)
    return kps, feature, R.rig_camera_dev()


def test_start_reconstructions_is_the_host_path_on_the_same_device_results(gpu, cons):
    """consensus -> join -> bootstrap -> add_reconstruction -> world table -> optimize_reconstruction with one wait; the table,
    maps and constraint arrays equal, byte for byte, what read back, join_pairs with the key rule's permutation,
    ThreeViewInit.init and the statement give on the same device results"""
    torch = gpu
    from cv_amd import _lib
    from cv_amd.ransac import EssentialConsensus
    from cv_amd.reconstruction import start_reconstructions
    from cv_amd.three_view import ThreeViewInit, join_pairs
    cap, n = 256, 200
    kps, feature, cam = synthetic_views(61, n, cap)
    dev = torch.device("cuda", 0)
    c = EssentialConsensus(2048, 1024)
    try:
        c.reserve(2)
        d_kps = _lib.device_bytes(torch, kps, dev)
        counts = np.array([n, n, n], np.uint32)
        pairs = np.zeros((2, cap, 2), np.uint32)
        rng = np.random.default_rng(4)
        for k in (0, 1):                                                  # the matcher's lists, a tenth of them wrong
            other = feature[k + 1].copy()
            wrong = rng.permutation(n)[:n // 10]
            other[wrong] = other[np.roll(wrong, 1)]
            order = rng.permutation(n)
            pairs[k, :n] = np.stack([feature[0][order], other[order]], 1)
        d_pairs, d_npairs = torch.from_numpy(pairs.view(np.int32)).to(dev), torch.from_numpy(np.array([n, n], np.int32)).to(dev)
        arrsac = c.make_params(1e-5, n_hypotheses=256, seed=7, block_size=64, init_blocks=1, max_candidates=64, halve=True)
        tv = ThreeViewInit.params(three_view_patience=64, three_view_filter_loop_iterations=2)
        seed = 0xABCDEF12345
        r = start_reconstructions(torch, c, d_kps, counts, cap, cam, d_pairs, d_npairs, [0, 0], [1, 2], arrsac, [(0, 1)], [0], [1], [2],
                                  3, 0, minimum=64, seed=seed, tv_params=tv)
        u32 = lambda t: t.cpu().numpy().view(np.uint32)
        # the host path on the same consensus results
        inliers, n_inl, best = u32(r.consensus[2]), u32(r.consensus[3]), u32(r.consensus[1])
        poses = r.consensus[0].cpu().numpy().reshape(2, 3, 4)
        assert (best != K.NONE).all() and n_inl.min() >= 150
        lists = [pairs[k][inliers[k, :n_inl[k]]] for k in (0, 1)]
        n_common = len(join_pairs(lists[0], lists[1])[0])
        perm = S.shuffle_permutation(seed, 0, n_common)
        triples, first_only, second_only = join_pairs(lists[0], lists[1], permutation=perm)
        join = r.join
        assert u32(join.verdict).tolist() == [K.JP_OK] and u32(join.counts).reshape(-1).tolist() == [len(triples), len(first_only), len(second_only)]
        assert np.array_equal(u32(join.triples)[0, :len(triples)], triples) and np.array_equal(u32(join.first_only)[0, :len(first_only)], first_only)
        assert np.array_equal(u32(join.second_only)[0, :len(second_only)], second_only)
        host = ThreeViewInit(c).init(torch, [kps[v][:n] for v in range(3)], cam, poses[0], poses[1], lists[0], lists[1], tv, permutation=perm)
        tv_verdict, pose_out, combined, first_ok, second_ok = r.bootstrap
        assert int(u32(tv_verdict)[0]) == host.verdict == _lib.RS_TV_OK
        assert np.array_equal(pose_out.cpu().numpy().reshape(2, 3, 4), host.poses)
        masks = [combined.cpu().numpy()[0], first_ok.cpu().numpy()[0], second_ok.cpu().numpy()[0]]
        assert np.array_equal(masks[0][:len(triples)].astype(bool), host.combined) and np.array_equal(masks[1][:len(first_only)].astype(bool), host.first_ok)
        assert np.array_equal(masks[2][:len(second_only)].astype(bool), host.second_ok)
        # ... then the statement
        scene = K.scene((0, 1, 2), (n, n, n), triples.tolist(), host.combined.astype(int).tolist(), first_only.tolist(),
                        host.first_ok.astype(int).tolist(), second_only.tolist(), host.second_ok.astype(int).tolist(), pose=host.poses.reshape(24))
        inp = K.add_inputs([scene], cap, 3, 3, 0)
        inp["kps"] = kps.view(np.uint8).reshape(3, cap, 28)
        stated = S.add_reconstruction(inp, K.add_outputs(inp))
        st = r.start
        got = dict(obs_start_out=st.obs_start_out, obs_out=st.obs_out, obs_counts_out=st.obs_counts_out, counts_out=st.counts_out,
                   landmarks_out=st.landmarks_out, recon_start_out=st.recon_start_out, view_start_out=st.view_start_out, views_out=st.views_out,
                   constraint_verdict_out=st.constraint_verdict_out, frame_verdict=st.frame_verdict, stats=st.stats, call_verdict=st.call_verdict,
                   counts_dst=st.counts_dst)
        rows, n_obs = (int(v) for v in stated["counts_out"][:2])
        for k, t in got.items():
            g, w = u32(t).reshape(-1), stated[k].reshape(-1)
            if k == "obs_out":
                g, w = g[:2 * n_obs], w[:2 * n_obs]                       # (behind the total: the fill there, zeros here)
            assert np.array_equal(g, w), k
        assert np.array_equal(st.constraint_poses_out.cpu().numpy(), stated["constraint_poses_out"])
        assert np.array_equal(st.kps_dst.cpu().numpy().view(np.uint8).reshape(3, cap, 28), stated["kps_dst"])
        assert stated["frame_verdict"].tolist() == [K.AR_OK] and rows >= n and n_obs == 3 * n
        # the stages behind accept the table
        reason = r.first_reason.cpu().numpy()[:rows]
        assert (reason == _lib.TRI_OK).sum() >= 50 and (reason != _lib.TRI_BAD_INDEX).all()
        assert int(u32(r.rows[2])[0]) == 0
        from cv_amd.reconstruction import stopped_at
        assert stopped_at(u32(r.verdict)[0]) not in [(k, "relax", _lib.RS_PG_BAD_INDEX) for k in range(64)] + [(k, "filter", _lib.RS_OF_BAD_RANGE) for k in range(64)]
        assert int(u32(r.pose_graph[0])[0]) != _lib.RS_PG_BAD_INDEX and int(u32(r.filter.recon_verdict)[0]) != _lib.RS_OF_BAD_RANGE
    finally:
        c.close()


def test_reconstruction_start_from_a_native_process(gpu, tmp_path):
    """cv_sfm::ReconstructionStart of include/akaze.hpp from a process without Python (tests/cpp/bootstrap.cpp)"""
    import subprocess

    import host_build
    cap, n_slots = 72, 4
    rng = np.random.default_rng(31)

    def one_to_one(n_pairs, n_inliers):
        pairs = list(zip(rng.permutation(60)[:n_pairs].tolist(), rng.permutation(60)[:n_pairs].tolist()))
        return K.slot(pairs, sorted(rng.permutation(n_pairs)[:n_inliers].tolist()))
    slots = [one_to_one(55, 50), one_to_one(50, 41), one_to_one(58, 30), one_to_one(40, 40)]
    scenes = [(0, 1), (2, 3)]
    jin = K.join_inputs(slots, scenes, cap, minimum=20, shuffle=True, seed=0x0123456789ABCDEF)
    joined = K.join(jin)
    assert joined["verdict"].tolist() == [K.JP_OK, K.JP_OK]
    ain = K.add_inputs([K.scene((0, 1, 2), (60, 60, 60)), K.scene((5, 3, 4), (66, 60, 72))], cap, 6, 7, 1)
    for k in K.JOIN_OUTPUT_NAMES[:6]:
        ain[k] = joined[k]
    for k in ("combined", "first_ok", "second_ok"):
        ain[k] = (rng.random((2, cap)) < 0.8).astype(np.uint8)
    want = K.add(ain)
    assert want["frame_verdict"].tolist() == [K.AR_OK, K.AR_OK]
    path = tmp_path / "call.bin"
    with open(path, "wb") as fp:
        fp.write(np.array([n_slots, cap, 2, 6, 7, 1, 20, 1, 0x89ABCDEF, 0x01234567], np.uint32).tobytes())
        for a in (jin["pairs"], jin["npairs"], jin["inliers"], jin["n_inliers"], jin["best_id"], jin["slot_first"], jin["slot_second"], ain["ic"],
                  ain["i_first"], ain["i_second"], ain["tv_verdict"], ain["counts"], jin["pose"], ain["pose_out"], ain["combined"], ain["first_ok"],
                  ain["second_ok"], ain["kps"]):
            fp.write(np.ascontiguousarray(a).tobytes())
    exe = host_build.native(tmp_path, "bootstrap.cpp", hip=True)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("bootstrap ok"), (r.returncode, r.stderr[-400:])
    out = {line.split(" ", 1)[0]: line.split()[1:] for line in r.stdout.splitlines()[:-1]}
    num = lambda k: np.array(out[k], np.int64)
    rows, n = (int(v) for v in want["counts_out"][:2])
    assert np.array_equal(num("join_counts"), np.concatenate([joined["ntriples"], joined["nfirst"], joined["nsecond"]]))
    assert np.array_equal(num("join_verdict"), joined["verdict"]) and np.array_equal(num("triples"), joined["triples"].reshape(-1))
    assert np.array_equal(num("counts"), want["counts_out"]) and np.array_equal(num("start"), want["obs_start_out"][:rows + 1])
    assert np.array_equal(num("obs"), want["obs_out"][:n].reshape(-1)) and np.array_equal(num("landmarks"), want["landmarks_out"].reshape(-1))
    assert np.array_equal(num("obs_counts"), want["obs_counts_out"][:rows]) and np.array_equal(num("verdicts"), want["frame_verdict"])
    assert np.array_equal(num("recon_start"), want["recon_start_out"]) and np.array_equal(num("view_start"), want["view_start_out"])
    assert np.array_equal(num("views"), want["views_out"].reshape(-1)) and np.array_equal(num("constraint_verdict"), want["constraint_verdict_out"])
    assert np.array_equal(num("stats"), want["stats"].reshape(-1)) and num("call").tolist() == [K.AR_OK]
    assert np.array_equal(num("counts_dst"), want["counts_dst"]) and np.array_equal(num("kps_dst"), want["kps_dst"].reshape(-1).view(np.uint32))
    assert np.array_equal(np.array(out["poses"], np.float64)[12:], want["poses"].reshape(-1)[12:])      # (block 0 is no view: its fill)
