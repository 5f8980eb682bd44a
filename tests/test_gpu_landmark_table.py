"""The landmark-table kernels (cv_amd/csrc/rs_landmark_table.hip) against the host build of the same header
(tests/landmark_table_checker.py): every output buffer is compared in bytes, WHOLE — both sides start from the same fill
pattern, so a word a call should have written and did not shows, and so does one it should have left alone.  Where the
tables are small enough to walk in Python the device's buffers are held to the independent statement
(tests/landmark_table_statement.py) as well.  Run with -m gpu.

Shapes: T = RS_LT_TILE rows of the input table are one workgroup's tile of the scan (256 threads x 4 rows), the workgroup
that scans the tile sums takes 256 of them per pass; a slot's features and matches are walked 256 at a time (cap = 200 is no
multiple of 64); the mask hands a candidate to its wave when its two lists hold more than 32 entries together."""
import ctypes as C

import numpy as np
import pytest

import landmark_table_checker as K
import landmark_table_statement as S
import observation_filter_checker as F

pytestmark = pytest.mark.gpu


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


def tile():
    from cv_amd import _lib
    return _lib.RS_LT_TILE


def device_add_views(torch, cons, inp):
    """rs_add_views_device on the arrays of a call -> dict of the output buffers as the host checker shapes them"""
    from cv_amd import _lib
    from cv_amd.landmark_table import LandmarkUpdate
    dev = torch.device("cuda", 0)
    up = lambda a: None if a is None else _lib.device_bytes(torch, a, dev)
    p = lambda t: None if t is None else t.data_ptr()
    names = ("start", "obs", "split", "split_count", "counts", "matches", "nmatches", "final", "verdict", "pose_out", "best", "skip")
    d_in = {k: up(inp[k]) for k in names}
    want = K.outputs(inp)
    d = {k: up(want[k]) for k in K.OUTPUT_NAMES}                       # the host's fill, byte for byte
    LandmarkUpdate(cons).add_views_device(
        p(d_in["start"]), p(d_in["obs"]), inp["n_obs"], inp["n_landmarks"], inp["n_world"], p(d_in["split"]), p(d_in["split_count"]),
        inp["split_room"], inp["cap"], inp["n_blocks"], inp["ik"], p(d_in["counts"]), p(d_in["matches"]), p(d_in["nmatches"]), p(d_in["final"]),
        p(d_in["verdict"]), p(d_in["pose_out"]), p(d_in["best"]), p(d_in["skip"]), inp["obs_room"], inp["lm_room"],
        *(p(d[k]) for k in K.OUTPUT_NAMES), stream_to_wait=_lib.wait_handle(torch.cuda.current_stream(dev)))
    cons.sync()
    return {k: d[k].cpu().numpy().view(want[k].dtype).reshape(want[k].shape) for k in K.OUTPUT_NAMES}


def assert_same(got, want):
    for k in K.OUTPUT_NAMES:
        g, w = got[k].view(np.uint8).reshape(len(want[k]), -1), want[k].view(np.uint8).reshape(len(want[k]), -1)
        if not np.array_equal(g, w):
            bad = np.flatnonzero((g != w).any(1))
            raise AssertionError((k, len(bad), bad[:10], got[k][bad[:4]], want[k][bad[:4]]))


def check(torch, cons, inp, statement=False):
    """device == host build in every byte of every output buffer -> the host result"""
    want = K.add_views(inp)
    got = device_add_views(torch, cons, inp)
    assert_same(got, want)
    if statement:
        K.check_against_statement(inp, got)
    return want


def numpy_table(seed, n_landmarks, n_views, cap, max_len=4, long_rows=()):
    """n_landmarks lists of 0 .. max_len observations (empty rows among them; `long_rows`: {row: length}), the blocks of a list
    distinct, every {block, feature} once -> start, obs, counts [n_views]"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, max_len + 1, n_landmarks)
    for r, n in dict(long_rows).items():
        lens[r] = n
    assert lens.max(initial=0) <= n_views
    start = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    n = int(start[-1])
    row_of = np.repeat(np.arange(n_landmarks), lens)
    blocks = (row_of * 7 + (np.arange(n) - start[row_of])) % n_views
    order = np.argsort(blocks, kind="stable")
    first = np.searchsorted(blocks[order], blocks[order], "left")
    feats = np.empty(n, np.int64)
    feats[order] = np.arange(n) - first
    counts = np.bincount(blocks, minlength=n_views).astype(np.uint32)
    assert counts.max(initial=0) <= cap
    obs = np.stack([blocks, feats], 1).astype(np.uint32).reshape(-1, 2)
    return start, obs, counts


def call_on(start, obs, counts, cap, slots, pad=3, **kw):
    """a call over a numpy_table: the frames' blocks lie behind the table's, in descending order"""
    n_views, n_obs = len(counts), len(obs) + pad
    full = np.full((max(n_obs, 1), 2), K.FILL32, np.uint32)
    full[:len(obs)] = obs
    n_blocks = n_views + len(slots)
    cnt = np.zeros(n_blocks, np.uint32)
    cnt[:n_views] = counts
    made = []
    for f, s in enumerate(slots):
        s = dict(s, block=n_blocks - 1 - f)
        cnt[s["block"]] = s["count"]
        made.append(s)
    return K.inputs(start, full, n_obs, cap, n_blocks, made, counts=cnt, **kw)


@pytest.mark.parametrize("n", ["0", "1", "T-1", "T", "T+1", "256T+3"])
def test_row_counts_around_a_tile_and_beyond_one_pass_of_the_tile_sums(gpu, cons, n):
    T = tile()
    n = {"0": 0, "1": 1, "T-1": T - 1, "T": T, "T+1": T + 1, "256T+3": 256 * T + 3}[n]
    cap, n_views = 200, 64 if n <= 2 * T else 8192
    start, obs, counts = numpy_table(n, n, n_views, cap)
    names = sorted({l for l in (0, n // 2, T - 1, T, n - 1, 255 * T, 256 * T, 256 * T + 1) if 0 <= l < n})
    slots = [K.slot(0, cap, [(j, l) for j, l in enumerate(names)]),                       # count == cap: 200 - len(names) new rows
             K.slot(0, 5, [(3, n - 1)] if n else []),                                     # the last row a second time
             K.slot(0, 0)]
    inp = call_on(start, obs, counts, cap, slots, split=[(0, cap - 1), (1, cap - 1)])
    want = check(gpu, cons, inp, statement=n <= 2 * T)
    assert want["counts_out"][0] == n + 2 + (cap - len(names)) + (4 if n else 5)
    assert np.all(want["frame_verdict"] == K.OK)


def test_lists_and_merges_across_tiles(gpu, cons):
    """long lists in the last row of a tile and the first of the next; a merge whose lists lie in different tiles, once with
    b > a and once with b < a; empty rows all over the input"""
    T = tile()
    n, cap = 2 * T + 10, 200
    long_rows = {T - 1: 60, T: 60, 5: 3, T + 7: 2, 2 * T + 3: 3, 9: 2, T - 2: 0, T + 1: 0}
    start, obs, counts = numpy_table(5, n, 64, cap, long_rows=long_rows)
    slots = [K.slot(0, 4, [(0, n + 0), (1, T - 1), (3, T)]), K.slot(0, 7, [(2, n + cap + 2), (0, T), (6, T - 2)])]
    inp = call_on(start, obs, counts, cap, slots, best={(0, 0): (5, T + 7), (1, 2): (2 * T + 3, 9)})
    want = check(gpu, cons, inp, statement=True)
    assert want["counts_out"].tolist()[2:] == [2, 0]
    rows = K.rows(want, n)
    assert len(rows[5]) == 3 + 2 + 1 and rows[T + 7] == [] and len(rows[2 * T + 3]) == 3 + 2 + 1 and rows[9] == []
    assert len(rows[T]) == 62 and rows[T][-2:] == [(65, 3), (64, 0)] and rows[T - 2] == [(64, 6)]     # slot order: block 65 is slot 0


def test_frames_of_every_kind_in_one_call(gpu, cons):
    """cap = 200; a frame without features, one with count == cap, a refused slot between two accepted ones, a skipped slot, a
    split list whose count lies above its room"""
    cap, n = 200, 300
    start, obs, counts = numpy_table(11, n, 16, cap)
    rng = np.random.default_rng(11)
    feats, lms = rng.permutation(cap)[:150], rng.permutation(n)[:150]
    slots = [K.slot(0, 0),
             K.slot(0, cap, [(int(j), int(l)) for j, l in zip(feats, lms)], final=[int(k % 7 != 0) for k in range(150)]),
             K.slot(0, 9, [(1, 2), (3, n)]),                                               # names row n: refused
             K.slot(0, 130, [(5, int(lms[0])), (129, 7), (128, 299)]),
             K.slot(0, 12, [(0, 1)], skip=1),
             K.slot(0, 65, [(64, 7), (0, 8)], verdict=K.SV_FEW_ROBUST),
             K.slot(0, 65, [(64, 7), (63, 0)])]
    inp = call_on(start, obs, counts, cap, slots, split=[(b, cap - 1) for b in range(5)], split_count=9, split_room=5)
    want = check(gpu, cons, inp, statement=True)
    assert want["frame_verdict"].tolist() == [K.OK, K.OK, K.BAD_INDEX, K.OK, K.NOT_ACCEPTED, K.NOT_ACCEPTED, K.OK]
    assert np.all(want["stats"][[2, 4, 5]] == 0) and want["stats"][0].tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("name", sorted(K.designed_cases()))
def test_designed_calls(gpu, cons, name):
    """every rule between frames and every refusal, one at a time: tests/landmark_table_checker.py designed_cases"""
    check(gpu, cons, K.designed_cases()[name], statement=True)


def test_a_bad_slot_leaves_its_neighbours_output_unchanged(gpu, cons):
    cases = K.designed_cases()
    good = lambda block, lm: K.slot(block, 3, [(1, lm)])
    base = device_add_views(gpu, cons, K.designed([good(4, 0), K.slot(5, 2, [(0, 99)], verdict=K.SV_FEW_ROBUST), good(6, 2)]))
    for name in sorted(cases):
        if not name.startswith("bad:"):
            continue
        got = device_add_views(gpu, cons, cases[name])
        assert got["frame_verdict"].tolist() == [K.OK, K.BAD_INDEX, K.OK], name
        for k in ("start_out", "obs_out", "landmarks_out", "obs_counts_out", "counts_out", "poses", "call_verdict"):
            assert np.array_equal(got[k], base[k]), (name, k)
        assert np.array_equal(got["stats"][[0, 2]], base["stats"][[0, 2]]) and np.all(got["stats"][1] == 0)


@pytest.mark.parametrize("seed", range(6))
def test_random_batches(gpu, cons, seed):
    inp = K.random_call(200 + seed, n_landmarks=60 + 140 * seed, n_views=16, n_frames=1 + seed, cap=200, merges=4, collide=seed % 2 == 0,
                        bad_slots=seed == 3, split=seed, extra_room=seed % 3)
    check(gpu, cons, inp, statement=True)


def test_the_output_does_not_depend_on_arrival_order(gpu, cons):
    """64 frames on the same few landmarks: the cursor hands out places in any order, the fix-up brings slot order back — the
    same bytes on every run, and the host's"""
    n, cap = 40, 64
    start, obs, counts = numpy_table(3, n, 8, cap)
    slots = [K.slot(0, 6, [(j, (j * 5 + f) % 4) for j in range(4)]) for f in range(64)]
    inp = call_on(start, obs, counts, cap, slots)
    want = check(gpu, cons, inp, statement=True)
    assert max(len(r) for r in K.rows(want, n)) >= 64
    for _ in range(2):
        assert_same(device_add_views(gpu, cons, inp), want)


def device_mask(torch, cons, start, obs, n_obs, best, decision):
    from cv_amd import _lib
    from cv_amd.landmark_table import LandmarkUpdate
    dev = torch.device("cuda", 0)
    up = lambda a: _lib.device_bytes(torch, a, dev)
    d_start, d_obs, d_best, d_decision = up(start), up(obs), up(best), up(decision)
    Fr, cap = decision.shape
    d_mask = torch.full((Fr * cap,), K.FILL8, dtype=torch.uint8, device=dev)
    LandmarkUpdate(cons).sharing_view_device(d_start.data_ptr(), d_obs.data_ptr(), n_obs, len(start) - 1, d_best.data_ptr(), d_decision.data_ptr(),
                                             cap, Fr, d_mask.data_ptr(), _lib.wait_handle(torch.cuda.current_stream(dev)))
    cons.sync()
    return d_mask.cpu().numpy().reshape(Fr, cap)


def test_the_mask_on_designed_candidates(gpu, cons):
    """decisions 0, 1, 2 (and 3), absent landmarks, keys beyond the table, lists that share their last element only, lists of 1
    and of 65+ entries on both sides, an empty list; then the fill below n_obs"""
    lists = K.mask_lists()
    start, obs, n_obs, best, decision = K.mask_case(lists, K.MASK_PAIRS, K.MASK_DECISIONS)
    got = device_mask(gpu, cons, start, obs, n_obs, best, decision)
    assert np.array_equal(got, K.sharing_view(start, obs, n_obs, best, decision)) and got[0].tolist() == K.MASK_WANT
    # the same candidates spread over three slots of cap 200: every byte is written, 0 where nothing was designed
    pairs = [(K.NONE, K.NONE)] * 600
    decisions = [0] * 600
    for k, (pr, d) in enumerate(zip(K.MASK_PAIRS, K.MASK_DECISIONS)):
        pairs[37 * k], decisions[37 * k] = pr, d
    start, obs, n_obs, best, decision = K.mask_case(lists, pairs, decisions, cap=200, frames=3)
    got = device_mask(gpu, cons, start, obs, n_obs, best, decision)
    assert np.array_equal(got, K.sharing_view(start, obs, n_obs, best, decision))
    assert got.reshape(-1)[::37][:16].tolist() == K.MASK_WANT and got.sum() == sum(K.MASK_WANT)
    # the fill below n_obs
    start, obs, _, best, decision = K.mask_case(lists, K.MASK_PAIRS, K.MASK_DECISIONS, pad=0)
    cut = int(start[7]) + 3
    got = device_mask(gpu, cons, start, obs, cut, best, decision)
    assert np.array_equal(got, K.sharing_view(start, obs, cut, best, decision))
    assert got[0, 9] == 1 and got[0, 10] == 0 and got[0, 12] == 0


def test_the_mask_on_random_candidates_with_many_long_lists_in_one_wave(gpu, cons):
    n, cap, Fr = 500, 200, 3
    long_rows = {int(r): int(l) for r, l in zip(range(0, 500, 9), np.random.default_rng(1).integers(20, 250, 56))}
    start, obs, _ = numpy_table(21, n, 256, 4096, long_rows=long_rows)
    rng = np.random.default_rng(22)
    best = np.full((Fr, cap, 3, 2), K.NONE, np.uint32)
    best[:, :, :2, 0] = rng.integers(0, n + 3, (Fr, cap, 2))
    best[:, :, 0, 0][rng.random((Fr, cap)) < 0.4] = rng.choice(list(long_rows), 1)[0]           # many wide candidates per wave
    best[:, :, 1, 0][rng.random((Fr, cap)) < 0.3] = rng.choice(list(long_rows), 1)[0]
    best[:, :, 1, 0][rng.random((Fr, cap)) < 0.05] = K.NONE
    decision = rng.choice([0, 1, 2, 2, 2], (Fr, cap)).astype(np.uint32)
    want = K.sharing_view(start, obs, len(obs), best, decision)
    assert 50 < want.sum() < Fr * cap - 50
    assert np.array_equal(device_mask(gpu, cons, start, obs, len(obs), best, decision), want)
    want = K.sharing_view(start, obs, len(obs) // 2, best, decision)                            # half the table is not the table's
    assert np.array_equal(device_mask(gpu, cons, start, obs, len(obs) // 2, best, decision), want)


def test_the_mask_on_both_sides_of_the_lanes_and_the_waves_walk(gpu, cons):
    """k_lt_sharing hands a candidate to its wave above 32 entries in both lists together (kLtShortPair): 32 and 33, disjoint and
    sharing the last element of either list only, in the first and the last lane of a wave and in the wave behind it"""
    a16 = [(v, 0) for v in range(16)]
    b16, b17 = [(100 + v, 0) for v in range(16)], [(100 + v, 0) for v in range(17)]
    c16, c17 = [(200 + v, 0) for v in range(15)] + [(15, 1)], [(200 + v, 0) for v in range(16)] + [(15, 1)]     # view 15 is a16's last
    lists = [a16, b16, b17, c16, c17]
    cases = [((0, 1), 1), ((0, 2), 1), ((0, 3), 0), ((0, 4), 0), ((4, 0), 0), ((2, 0), 1)]                    # 32, 33, 32, 33, 33, 33
    assert [len(lists[a]) + len(lists[b]) for (a, b), _ in cases] == [32, 33, 32, 33, 33, 33]
    cap = 192
    pairs, decisions, want = [(K.NONE, K.NONE)] * cap, [0] * cap, [0] * cap
    for j0, turn in ((0, 0), (58, 2), (64, 4)):                            # lanes 0 .. 5, lanes 58 .. 63, and wave 1
        for i, (pr, ok) in enumerate(cases[turn:] + cases[:turn]):
            pairs[j0 + i], decisions[j0 + i], want[j0 + i] = pr, 2, ok
    assert pairs[63] == (0, 2) and pairs[62] == (0, 1)                     # 33 entries in lane 63, 32 beside it
    start, obs, n_obs, best, decision = K.mask_case(lists, pairs, decisions, cap=cap)
    got = device_mask(gpu, cons, start, obs, n_obs, best, decision)
    assert np.array_equal(got, K.sharing_view(start, obs, n_obs, best, decision)) and got[0].tolist() == want


def test_refusals_with_a_context_launch_nothing(gpu, cons):
    """rooms too small, a repeated block, outputs over the input: AKZ_E_INVALID, and the outputs keep their fill"""
    from cv_amd import _lib
    from cv_amd.landmark_table import LandmarkUpdate
    torch = gpu
    dev = torch.device("cuda", 0)
    inp = K.designed_cases()["frames and a split list"]
    up = lambda a: None if a is None else _lib.device_bytes(torch, a, dev)
    p = lambda t: None if t is None else t.data_ptr()
    d_in = {k: up(inp[k]) for k in ("start", "obs", "split", "split_count", "counts", "matches", "nmatches", "final", "verdict", "pose_out")}
    d = {k: up(v) for k, v in K.outputs(inp).items()}

    def call(ik=None, **over):
        a = dict(obs_room=inp["obs_room"], lm_room=inp["lm_room"], **{k: p(d[k]) for k in K.OUTPUT_NAMES})
        a.update(over)
        try:
            LandmarkUpdate(cons).add_views_device(
                p(d_in["start"]), p(d_in["obs"]), inp["n_obs"], inp["n_landmarks"], inp["n_world"], p(d_in["split"]), p(d_in["split_count"]),
                inp["split_room"], inp["cap"], inp["n_blocks"], inp["ik"] if ik is None else ik, p(d_in["counts"]), p(d_in["matches"]),
                p(d_in["nmatches"]), p(d_in["final"]), p(d_in["verdict"]), p(d_in["pose_out"]), None, None, a["obs_room"], a["lm_room"],
                *(a[k] for k in K.OUTPUT_NAMES))
        except _lib.AkzError as e:
            return e.status
        return 0

    assert call(obs_room=inp["obs_room"] - 1) == -1 and call(lm_room=inp["lm_room"] - 1) == -1
    assert call(ik=[9]) == -1
    assert call(start_out=p(d_in["start"])) == -1 and call(obs_out=p(d_in["obs"])) == -1 and call(obs_counts_out=p(d_in["obs"])) == -1
    cons.sync()
    fill = K.outputs(inp)
    for k in K.OUTPUT_NAMES:
        assert np.array_equal(d[k].cpu().numpy().view(fill[k].dtype).reshape(fill[k].shape), fill[k]), k
    assert call() == 0
    cons.sync()
    assert d["call_verdict"].cpu().numpy().view(np.uint32)[0] == K.OK


# ---- behind the call: the stages that read the new table ----------------------------------------------------------------
def rs_camera(cam):
    from cv_amd import _lib
    return _lib.Camera(cam.fx, cam.fy, cam.cx, cam.cy, cam.skew, cam.k1, cam.use_k1, 0)


def registered_scene(seed=7, n_views=14, n_new=2, n_landmarks=2500, halves=0, outliers=0.25):
    """An observation_filter_checker scene of n_views views whose last n_new are the frames of a micro-batch: the table holds the
    observations of the others, the frames' own observations are their final matches (one in five is not final, so that its
    feature becomes a landmark).  `halves`: that many landmarks seen by the first frame and by four or more old views are cut in
    two — the second half of the list becomes a row behind the table — and the frame's feature is a merge candidate of the two
    (no other frame sees them, so every such merge is applied).
    -> dict(sc, inp, best, decision, lists)"""
    sc = F.scene(seed, n_views=n_views, n_landmarks=n_landmarks, lengths=(2, 8), outlier_fraction=outliers)
    rng = np.random.default_rng(seed)
    old, cap = n_views - n_new, sc["kps"].shape[1]
    start, obs = sc["start"].astype(np.int64), sc["obs"].astype(np.int64)
    lists = [[(int(b), int(f)) for b, f in obs[start[l]:start[l + 1]] if b < old] for l in range(n_landmarks)]
    seen = [{int(b): int(f) for b, f in obs[start[l]:start[l + 1]] if b >= old} for l in range(n_landmarks)]
    ik = [n_views - 1 - f for f in range(n_new)]                                  # slot 0 is the last block: not ascending
    counts = np.array([int(obs[obs[:, 0] == b, 1].max(initial=-1)) + 1 for b in range(n_views)], np.uint32)
    best, decision = {}, np.zeros((n_new, cap), np.uint32)
    cut = [l for l in range(n_landmarks) if ik[0] in seen[l] and len(seen[l]) == 1 and len(lists[l]) >= 4][:halves]   # named by that frame alone
    for k, l in enumerate(cut):
        lists.append(lists[l][len(lists[l]) // 2:])
        lists[l] = lists[l][:len(lists[l]) // 2]
        best[(0, seen[l][ik[0]])] = (l, n_landmarks + k)
    n_lm = len(lists)
    slots = []
    for f, b in enumerate(ik):
        matches, final = [], []
        for l in range(n_landmarks):
            if b not in seen[l]:
                continue
            j = seen[l][b]
            merged = (f, j) in best
            matches.append((j, n_lm + f * cap + j if merged else l))
            final.append(1 if merged else int(rng.random() < 0.8))
            decision[f, j] = 2 if merged else 1
        order = rng.permutation(len(matches))
        slots.append(K.slot(b, int(counts[b]), [matches[k] for k in order], [final[k] for k in order], pose=sc["poses"][b]))
    t_start, t_obs, n_obs = K.table(lists, pad=4)
    inp = K.inputs(t_start, t_obs, n_obs, cap, n_views, slots, best=best or None, counts=counts)
    inp["poses"] = sc["poses"].copy()
    inp["poses"][old:] = 0.0
    return dict(sc=sc, inp=inp, best=inp["best"], decision=decision, lists=lists, old=old)


def add_views_tensors(torch, cons, rs, table, d_poses):
    from cv_amd.landmark_table import LandmarkUpdate
    inp = rs["inp"]
    return LandmarkUpdate(cons).add_views_tensors(torch, table, d_poses, inp["cap"], [int(b) for b in inp["ik"]], inp["counts"], inp["matches"],
                                                  inp["nmatches"], inp["final"], inp["verdict"], inp["pose_out"], best=inp["best"])


def tensors_as_outputs(o, inp):
    u32 = lambda t: t.cpu().numpy().view(np.uint32)
    return dict(poses=o.poses.cpu().numpy(), start_out=u32(o.obs_start_out), obs_out=u32(o.obs_out).reshape(-1, 2), counts_out=u32(o.counts_out),
                landmarks_out=u32(o.landmarks_out), obs_counts_out=u32(o.obs_counts_out), frame_verdict=u32(o.frame_verdict), stats=u32(o.stats),
                call_verdict=u32(o.call_verdict))


def test_the_stages_behind_tolerate_the_empty_tail(gpu, cons):
    """rs_triangulate_landmarks_device, rs_filter_observations_device and rs_covisibility_candidates_device on the new table, once
    with (lm_room, obs_room) — what a chain that does not wait passes — and once with the counts: the same bytes on the filled
    rows; the tail reads RS_TRI_TOO_FEW and RS_OF_SINGLE"""
    from cv_amd import _lib, triangulation
    from cv_amd.covisibility import Covisibility
    from cv_amd.reconstruction import ObservationFilter
    torch = gpu
    dev = torch.device("cuda", 0)
    rs = registered_scene()
    sc, inp = rs["sc"], rs["inp"]
    cap, n_blocks = inp["cap"], inp["n_blocks"]
    table = triangulation.LandmarkTable(torch, start=inp["start"], obs=inp["obs"][:int(inp["start"][-1])])
    d_poses = torch.from_numpy(inp["poses"]).to(dev)
    d_kps = _lib.device_bytes(torch, sc["kps"].view(np.uint8), dev)
    added = add_views_tensors(torch, cons, rs, table, d_poses)
    cons.sync()
    got = tensors_as_outputs(added, inp)
    K.check_against_statement(dict(inp, n_obs=table.n_obs, obs_room=added.obs_room, lm_room=added.lm_room), got, fill=0)   # torch.zeros
    rows, n_filled = int(got["counts_out"][0]), int(got["counts_out"][1])
    assert inp["n_landmarks"] + 200 < rows < added.lm_room - 1000 and np.all(got["frame_verdict"] == K.OK)
    cam, prm = rs_camera(sc["cam"]), ObservationFilter.params(minimum_robust_landmarks=8)
    res = []
    for t in (added.table(torch), added.table(torch, (rows, n_filled))):
        world, reason = t.new_world(), torch.full((t.n_landmarks,), 0xA5, dtype=torch.uint8, device=dev)
        wait = _lib.wait_handle(torch.cuda.current_stream(dev))
        triangulation.triangulate_landmarks_device(cons._h, t, d_kps, cap, n_blocks, d_poses, cam, prm.triangulate, world, reason, wait)
        flt = ObservationFilter(cons).run_tensors(torch, t, d_kps, cap, n_blocks, d_poses, cam, np.array([0, t.n_landmarks], np.uint32),
                                                  np.array([0, n_blocks], np.uint32), params=prm)
        cov = Covisibility(cons).run_tensors(torch, t, cap, n_blocks, reason, np.arange(n_blocks, dtype=np.uint32),
                                             Covisibility.params(optimization_robust_covisibility_minimum_landmarks=4, optimization_minimum_landmarks=4))
        cons.sync()
        res.append((t, world.cpu().numpy(), reason.cpu().numpy(), flt, cov))
    (ta, wa, ra, fa, ca), (tb, wb, rb, fb, cb) = res
    assert ta.n_landmarks == added.lm_room and tb.n_landmarks == rows
    assert np.array_equal(wa[:rows].view(np.uint64), wb.view(np.uint64)) and np.array_equal(ra[:rows], rb)
    assert np.all(ra[rows:] == _lib.TRI_TOO_FEW) and (rb == _lib.TRI_OK).sum() > 1000
    h = lambda t: t.cpu().numpy()
    kept, split = (int(v) for v in h(fb.counts).view(np.uint32))
    assert h(fa.counts).view(np.uint32).tolist() == [kept, split] and kept + split == n_filled and split > 0
    assert np.array_equal(h(fa.keep)[:n_filled], h(fb.keep)[:n_filled])
    for name in ("lm_state", "tri_reason", "robust"):
        assert np.array_equal(h(getattr(fa, name))[:rows], h(getattr(fb, name))[:rows]), name
    assert np.all(h(fa.lm_state)[rows:] == _lib.RS_OF_SINGLE)
    assert np.array_equal(h(fa.obs_start_out)[:rows + 1], h(fb.obs_start_out)[:rows + 1]) and np.all(h(fa.obs_start_out)[rows:] == kept)
    assert np.array_equal(h(fa.obs_out)[:kept], h(fb.obs_out)[:kept]) and np.array_equal(h(fa.split_out)[:split], h(fb.split_out)[:split])
    assert np.array_equal(h(fa.recon_verdict), h(fb.recon_verdict)) and h(fb.recon_verdict)[0] == _lib.RS_OF_OK
    sa, sb = h(fa.stats).view(np.uint32), h(fb.stats).view(np.uint32)
    assert np.array_equal(sa[:, 1:], sb[:, 1:]) and sa[0, 0] == added.lm_room and sb[0, 0] == rows       # word 0: the rows it was handed
    for name in ("views", "lm_start", "lm", "slot_count", "target_verdict", "stats"):
        assert np.array_equal(h(getattr(ca, name)), h(getattr(cb, name))), name
    assert (h(cb.stats).view(np.uint32)[:, _lib.RS_CV_S_EMITTED] > 0).sum() >= n_blocks - 2


def test_the_chain_from_the_mask_to_the_next_world_table_waits_once(gpu, cons, monkeypatch):
    """Registration-shaped tensors made by hand: sharing_view -> triangulate -> triangulate_merged -> (the refinement's outputs:
    designed arrays) -> add_views -> LandmarkTable.from_device -> triangulate, enqueued without a wait in between and waited
    for once.  The mask and the new table are the statement's."""
    from cv_amd import _lib, triangulation
    from cv_amd.landmark_table import LandmarkUpdate
    torch = gpu
    dev = torch.device("cuda", 0)
    rs = registered_scene(seed=9, halves=40, outliers=0.0)
    sc, inp = rs["sc"], rs["inp"]
    cap, n_blocks, n_lm, Fr = inp["cap"], inp["n_blocks"], inp["n_landmarks"], inp["n_frames"]
    # two candidates whose lists share a view, and one with an absent second landmark: no merge, the feature matches nothing
    best, decision = inp["best"].copy(), rs["decision"]
    free = [j for j in range(int(inp["counts"][inp["ik"][0]]), cap)][:3]
    sharing = [(a, b) for a in range(200) for b in range(200, 400) if {v for v, _ in rs["lists"][a]} & {v for v, _ in rs["lists"][b]}][:2]
    for j, (a, b) in zip(free, sharing + [(5, K.NONE)]):
        best[0, j, 0, 0], best[0, j, 1, 0], decision[0, j] = a, b, 2
    table = triangulation.LandmarkTable(torch, start=inp["start"], obs=inp["obs"][:int(inp["start"][-1])])
    up = lambda a: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(dev)       # shaped, as Registration holds them
    d_poses, d_kps = torch.from_numpy(inp["poses"]).to(dev), _lib.device_bytes(torch, sc["kps"].view(np.uint8), dev)
    d_best, d_decision = up(best), up(decision)
    d_in = [up(inp[k]) for k in ("counts", "matches", "nmatches", "final", "verdict", "pose_out")]
    cam, tri = rs_camera(sc["cam"]), triangulation.make_params()
    upd = LandmarkUpdate(cons)
    torch.cuda.synchronize()
    waits = []
    monkeypatch.setattr(type(cons), "sync", lambda self, _f=type(cons).sync: (waits.append("rs_sync"), _f(self))[1])
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: waits.append("synchronize"))
    wait = lambda: _lib.wait_handle(torch.cuda.current_stream(dev))
    d_mask = upd.sharing_view_tensors(torch, table, d_best, d_decision)
    d_world = table.new_world(Fr * cap)
    triangulation.triangulate_landmarks_device(cons._h, table, d_kps, cap, n_blocks, d_poses, cam, tri, d_world, None, wait())
    triangulation.triangulate_merged_device(cons._h, table, d_kps, cap, n_blocks, d_poses, cam, tri, d_best, d_decision, d_mask, Fr, n_lm, d_world)
    added = upd.add_views_tensors(torch, table, d_poses, cap, [int(b) for b in inp["ik"]], *d_in, best=d_best)
    t2 = added.table(torch)
    world2, reason2 = t2.new_world(), torch.zeros((t2.n_landmarks,), dtype=torch.uint8, device=dev)
    triangulation.triangulate_landmarks_device(cons._h, t2, d_kps, cap, n_blocks, d_poses, cam, tri, world2, reason2, wait())
    cons.sync()
    assert waits == ["rs_sync"]
    monkeypatch.undo()
    mask = d_mask.cpu().numpy()
    lists = rs["lists"]
    assert mask.tolist() == S.sharing_mask(lists, best, decision, n_lm)
    merged = sorted((f, j) for (f, j) in ((0, j) for j in range(cap)) if decision[f, j] == 2 and mask[f, j])
    assert len(merged) == 40 and mask[0, free].tolist() == [0, 0, 0]
    st = K.check_against_statement(dict(inp, best=best, n_obs=table.n_obs, obs_room=added.obs_room, lm_room=added.lm_room),
                                   tensors_as_outputs(added, inp), fill=0)
    assert st["counts"][2:] == [40, 0]
    rows = st["counts"][0]
    w, w2, r2 = d_world.cpu().numpy(), world2.cpu().numpy(), reason2.cpu().numpy()
    a_rows = [int(best[f, j, 0, 0]) for f, j in merged]
    b_rows = [int(best[f, j, 1, 0]) for f, j in merged]
    assert (w[[n_lm + f * cap + j for f, j in merged], 3] >= 0).sum() >= 35          # the consensus' rows of the merged matches
    assert np.all(r2[b_rows] == _lib.TRI_TOO_FEW) and np.all(r2[rows:] == _lib.TRI_TOO_FEW)   # tombstones and the tail
    assert (r2[a_rows] == _lib.TRI_OK).sum() >= 35 and np.all(w2[np.array(a_rows)[r2[a_rows] == _lib.TRI_OK], 3] >= 0)
    # the new views' poses are where the next triangulation read them
    assert np.array_equal(added.poses.cpu().numpy()[rs["old"]:], sc["poses"][rs["old"]:])


def test_the_native_mirror_gives_the_same_table(gpu, cons, tmp_path):
    """cv_sfm::LandmarkBook of include/akaze.hpp from a process without Python (tests/cpp/landmark_table.cpp)"""
    import subprocess

    import host_build
    inp = K.random_call(77, n_landmarks=120, n_views=8, n_frames=3, cap=72, merges=3, split=4)
    inp["verdict"][:] = 0
    inp["skip"] = None
    inp["obs_room"], inp["lm_room"] = inp["n_obs"] + 4 + 3 * 72, 120 + 4 + 3 * 72
    decision = np.where(inp["best"][:, :, 0, 0] != K.NONE, 2, 1).astype(np.uint32)
    want = K.add_views(inp)
    mask = K.sharing_view(inp["start"], inp["obs"], inp["n_obs"], inp["best"], decision)
    path = tmp_path / "call.bin"
    with open(path, "wb") as fp:
        fp.write(np.array([inp["n_blocks"], 72, 120, inp["n_obs"], inp["n_world"], 3, 4, 1], np.uint32).tobytes())
        for a in (inp["start"], inp["obs"][:inp["n_obs"]], inp["split"], inp["split_count"], inp["ik"], inp["counts"], inp["matches"],
                  inp["nmatches"], inp["verdict"], inp["best"], decision, inp["pose_out"], inp["final"]):
            fp.write(np.ascontiguousarray(a).tobytes())
    exe = host_build.native(tmp_path, "landmark_table.cpp", hip=True)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("landmark_table ok"), (r.returncode, r.stderr[-400:])
    out = {line.split(" ", 1)[0]: line.split()[1:] for line in r.stdout.splitlines()[:-1]}
    num = lambda k: np.array(out[k], np.int64)
    rows, n = (int(v) for v in want["counts_out"][:2])
    assert np.array_equal(num("mask"), mask.reshape(-1)) and mask.sum() >= 3
    assert np.array_equal(num("counts"), want["counts_out"]) and np.array_equal(num("start"), want["start_out"][:rows + 1])
    assert np.array_equal(num("obs"), want["obs_out"][:n].reshape(-1)) and np.array_equal(num("landmarks"), want["landmarks_out"].reshape(-1))
    assert np.array_equal(num("obs_counts"), want["obs_counts_out"][:rows]) and np.array_equal(num("verdicts"), want["frame_verdict"])
    assert np.array_equal(num("stats"), want["stats"].reshape(-1)) and num("call").tolist() == [K.OK]
    assert np.array_equal(np.array(out["poses"], np.float64), want["poses"].reshape(-1))


def test_registration_sharing_view_and_add_views(gpu, monkeypatch):
    """Registration.sharing_view -> consensus -> refine -> add_views on one small batch, no host step between them: the mask is
    the host build's, and the new table is what the host build and the statement make of what the refinement left on the
    device.  Then add_views_and_regenerate from the same table: the same bytes again (the reference's remove_view is this
    re-run), regenerate behind it on (lm_room, obs_room), one wait."""
    import single_view_checker as V
    from test_gpu_single_view import RATE, device_params
    from cv_amd import _lib, triangulation
    from cv_amd.landmark_table import add_views_and_regenerate
    from cv_amd.registration import Registration
    torch = gpu
    rigs = [V.Rig(61, 200, none=(4, 90)), V.Rig(62, 180, merged=(5, 6), none=(8,), outliers=(11, 12, 13)), V.Rig(63, 120)]
    b = V.Batch(rigs, 512)
    Fr, cap = len(rigs), b.cap
    best = np.full((Fr, cap, 3, 2), V.NO_ID, np.uint32)
    decision, counts = np.zeros((Fr, cap), np.uint32), np.zeros(b.n_blocks, np.uint32)
    for s, r in enumerate(rigs):
        rows = b.matches[s, :r.n, 1]
        best[s, :r.n, 0, 0] = np.where(r.merged, b.best[s, :r.n, 0, 0], rows)
        best[s, :r.n, 1, 0] = np.where(r.merged, b.best[s, :r.n, 1, 0], V.NO_ID)
        best[s, :r.n, :, 1] = (10, 50, 90)
        decision[s, :r.n] = np.where(r.merged, 2, 1)
        counts[b.ik[s]] = r.n
    old_obs = b.obs[:b.n_obs].astype(np.int64)
    for blk in range(b.n_blocks):                                     # the stored views' feature counts
        if blk not in b.ik:
            counts[blk] = int(old_obs[old_obs[:, 0] == blk, 1].max(initial=-1)) + 1
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    cw = np.random.default_rng(1).integers(0, 256, (32, 64), dtype=np.uint8)
    reg = Registration(torch, cap, Fr, 2, cw, (V.CAM["fx"], V.CAM["fy"], V.CAM["cx"], V.CAM["cy"], 0.0, None), n_hypotheses=512, max_candidates=64,
                       estimations_per_block=0, block_size=64)
    try:
        # what match_views() leaves, set by hand: the matcher's search is not what this test is about
        reg._cur, reg._fb, reg._calls = reg._sets[0], np.asarray(b.ik, np.uint32), 1
        reg.best.copy_(t(best.view(np.int32)))
        reg.decision.copy_(t(decision.view(np.int32)))
        d_kps, d_counts, d_world = t(b.kps.view(np.uint8).reshape(b.n_blocks, cap, 28)), t(counts.view(np.int32)), t(b.world)
        d_poses = t(b.poses)
        table = triangulation.LandmarkTable(torch, start=b.obs_start, obs=b.obs[:b.n_obs])
        torch.cuda.synchronize()
        d_mask = reg.sharing_view(table)
        reg.consensus(d_kps, d_counts, d_world, b.n_world, d_merge_ok=d_mask, stream_to_wait=reg.rs_stream())
        st = V.settings(single_view_optimization_rate=RATE, single_view_patience=100, single_view_filter_loop_iterations=2)
        out = reg.refine(d_poses, table.d_start, table.d_obs, b.n_landmarks, params=device_params(st), stream=torch.cuda.current_stream(dev))
        added = reg.add_views(table, d_poses)
        reg.sync()
        mask = d_mask.cpu().numpy()[:Fr]
        assert np.array_equal(mask, K.sharing_view(b.obs_start, b.obs, table.n_obs, best, decision))
        assert mask.sum() == sum(int(r.merged.sum()) for r in rigs) == 2
        pose, verdict, final, n_final, stats = out.host()
        assert list(verdict[:Fr]) == [V.OK] * 3
        inp = dict(start=b.obs_start, obs=b.obs, n_obs=table.n_obs, n_landmarks=b.n_landmarks, n_world=b.n_world, split=None, split_count=None,
                   split_room=0, cap=cap, n_blocks=b.n_blocks, ik=np.asarray(b.ik, np.uint32), n_frames=Fr, counts=counts,
                   matches=reg.originals.cpu().numpy().view(np.uint32)[:Fr].copy(), nmatches=reg.noriginals.cpu().numpy().view(np.uint32)[:Fr].copy(),
                   final=np.ascontiguousarray(final[:Fr], np.uint8), verdict=np.ascontiguousarray(verdict[:Fr], np.uint32),
                   pose_out=np.ascontiguousarray(pose[:Fr], np.float64).reshape(Fr, 12), best=best, skip=None, obs_room=added.obs_room,
                   lm_room=added.lm_room, poses=b.poses)
        got = tensors_as_outputs(added, inp)
        res = K.check_against_statement(inp, got, fill=0)
        assert res["frame_verdict"] == [K.OK] * 3 and res["counts"][2:] == [2, 0] and all(s[0] > 60 for s in res["stats"])
        want = K.add_views(inp)
        rows, n = res["counts"][:2]
        assert np.array_equal(got["start_out"], want["start_out"]) and np.array_equal(got["obs_out"][:n], want["obs_out"][:n])
        assert np.array_equal(got["landmarks_out"], want["landmarks_out"]) and np.array_equal(got["poses"], want["poses"])
        # the same call again, regenerate behind it, one wait
        waits = []
        monkeypatch.setattr(type(reg.cons), "sync", lambda self, _f=type(reg.cons).sync: (waits.append("rs_sync"), _f(self))[1])
        monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: waits.append("synchronize"))
        again, result = add_views_and_regenerate(torch, reg, table, d_kps, d_poses, np.array([0, b.n_blocks], np.uint32))
        assert waits == ["rs_sync"]
        monkeypatch.undo()
        torch.cuda.synchronize()
        got2 = tensors_as_outputs(again, inp)
        for k in ("start_out", "obs_out", "counts_out", "landmarks_out", "obs_counts_out", "frame_verdict", "stats", "call_verdict"):
            assert np.array_equal(got2[k], got[k]), k
        assert result.world.shape[0] == added.lm_room and result.filter.n_landmarks == added.lm_room
        assert np.all(result.filter.lm_state.cpu().numpy()[rows:] == _lib.RS_OF_SINGLE)
        assert np.all(result.world_reason.cpu().numpy()[rows:] == _lib.TRI_TOO_FEW)
    finally:
        reg.close()
