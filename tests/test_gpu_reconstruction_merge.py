"""The reconstruction-merge kernels (cv_amd/csrc/rs_reconstruction_merge.hip) against the host build of the same header
(tests/reconstruction_merge_checker.py): every output buffer is compared in bytes, WHOLE — both sides start from the same
fill pattern, so a word a call should have written and did not shows, and so does one it should have left alone.  Where the
tables are clean and small enough to walk in Python the device's buffers are held to the independent statement
(tests/reconstruction_merge_statement.py) as well.  Run with -m gpu.

Shapes: T = RS_LT_TILE rows of either table are one workgroup's tile of the scans (256 threads x 4 rows), the workgroup that
scans the tile sums takes 256 of them per pass; a row whose lists hold more than 64 entries together is walked by its wave, 64
entries a step; cap_per_img = 8 and at most 40 blocks, so the large tables list a {block, feature} in many rows — the kernels
do not care, d_landmarks_out takes the lowest key on both sides.  One test stands on either side of the 65 536 blocks up to which
the destination's blocks are marked in an LDS bitmap."""
import numpy as np
import pytest

import reconstruction_merge_checker as K
from test_reconstruction_merge_math import BOUND

pytestmark = pytest.mark.gpu

CAP, N_BLOCKS, BRIDGE = 8, 40, 19
DST_BLOCKS, SRC_BLOCKS = list(range(0, 19)), list(range(20, 40))


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


def uploader(torch):
    from cv_amd import _lib
    dev = torch.device("cuda", 0)
    return lambda a: None if a is None else _lib.device_bytes(torch, a, dev)


def back(d, want, names):
    return {k: d[k].cpu().numpy().view(want[k].dtype).reshape(want[k].shape) for k in names}


def device_incorporate(torch, cons, inp, sync=True, over=None):
    """rs_incorporate_reconstruction_device on the arrays of a call -> dict of the output buffers as the host checker shapes them"""
    from cv_amd import _lib
    from cv_amd.reconstruction_merge import ReconstructionMerge
    up = uploader(torch)
    p = lambda t: None if t is None else t.data_ptr()
    d_in = {k: up(inp[k]) for k in ("dst_start", "dst_obs", "src_start", "src_obs", "map", "map_count", "src_pose", "skip")}
    want = K.incorporate_outputs(inp)
    d = {k: up(want[k]) for k in K.IR_OUTPUTS}                          # the host's fill, byte for byte
    a = dict(obs_room=inp["obs_room"], lm_room=inp["lm_room"], src_blocks=[int(b) for b in inp["src_blocks"]])
    a.update(over or {})
    ReconstructionMerge(cons).incorporate_device(
        p(d_in["dst_start"]), p(d_in["dst_obs"]), inp["n_dst_obs"], inp["n_dst"], p(d_in["src_start"]), p(d_in["src_obs"]), inp["n_src_obs"],
        inp["n_src"], p(d_in["map"]), p(d_in["map_count"]), inp["map_room"], inp["cap"], inp["n_blocks"], a["src_blocks"], inp["bridge_block"],
        p(d_in["src_pose"]), p(d_in["skip"]), a["obs_room"], a["lm_room"], *(p(d[k]) for k in K.IR_OUTPUTS),
        stream_to_wait=_lib.wait_handle(torch.cuda.current_stream(torch.device("cuda", 0))))
    if sync:
        cons.sync()
    return back(d, want, K.IR_OUTPUTS)


def assert_same(got, want, names=K.IR_OUTPUTS):
    for k in names:
        g, w = got[k].view(np.uint8).reshape(len(want[k]), -1), want[k].view(np.uint8).reshape(len(want[k]), -1)
        if not np.array_equal(g, w):
            bad = np.flatnonzero((g != w).any(1))
            raise AssertionError((k, len(bad), bad[:10], got[k][bad[:4]], want[k][bad[:4]]))


def check(torch, cons, inp, statement=False):
    """device == host build in every byte of every output buffer -> the host result"""
    want = K.incorporate(inp)
    got = device_incorporate(torch, cons, inp)
    assert_same(got, want)
    if statement:
        K.check_incorporate_against_statement(inp, got, BOUND)
    return want


def csr(rng, n, blocks, max_len=3, long_rows=()):
    """n rows of 0 .. max_len observations over `blocks` (`long_rows`: {row: length}), features below CAP -> start, obs"""
    lens = rng.integers(0, max_len + 1, n)
    for r, length in dict(long_rows).items():
        lens[r] = length
    start = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    total = int(start[-1])
    obs = np.stack([np.asarray(blocks)[rng.integers(0, len(blocks), total)], rng.integers(0, CAP, total)], 1).astype(np.uint32).reshape(-1, 2)
    return start, obs


def raw_inputs(seed, n_dst, n_src, pairs, dst_long=(), src_long=(), skip=None, pad=3, extra_room=0):
    """A call over two tables made by csr(): the destination over DST_BLOCKS and the bridging frame's block, the source over
    SRC_BLOCKS and the bridging frame's block"""
    rng = np.random.default_rng(seed)
    ds, dobs = csr(rng, n_dst, DST_BLOCKS + [BRIDGE], long_rows=dst_long)
    ss, sobs = csr(rng, n_src, SRC_BLOCKS + [BRIDGE], long_rows=src_long)
    full = lambda o: np.concatenate([o, np.full((pad, 2), K.FILL32, np.uint32)])
    m = np.full((max(len(pairs), 1), 2), K.FILL32, np.uint32)
    if len(pairs):
        m[:len(pairs)] = np.array(pairs, np.uint32).reshape(-1, 2)
    n_dst_obs, n_src_obs = len(dobs) + pad, len(sobs) + pad
    return dict(dst_start=ds, dst_obs=full(dobs), n_dst_obs=n_dst_obs, n_dst=n_dst, src_start=ss, src_obs=full(sobs), n_src_obs=n_src_obs,
                n_src=n_src, map=m, map_count=np.array([len(pairs)], np.uint32), map_room=max(len(pairs), 1), cap=CAP, n_blocks=N_BLOCKS,
                src_blocks=np.array(rng.permutation(SRC_BLOCKS), np.uint32), bridge_block=BRIDGE, src_pose=K.random_pose(rng),
                skip=None if skip is None else np.array(skip, np.uint32), obs_room=n_dst_obs + n_src_obs + extra_room,
                lm_room=n_dst + n_src + extra_room, poses=np.stack([K.random_pose(rng) for _ in range(N_BLOCKS)]))


def spread_pairs(n_src, n_dst, n=12):
    """a one-to-one map over rows spread through both tables, their first, last and tile-boundary rows among them"""
    T = tile()
    pick = lambda m: sorted({r for r in (0, 1, m // 3, m // 2, T - 1, T, T + 1, m - 2, m - 1) if 0 <= r < m})[:n]
    return list(zip(pick(n_src), reversed(pick(n_dst))))


@pytest.mark.parametrize("n_dst", ["0", "1", "T-1", "T", "T+1"])
def test_row_counts_of_each_table_around_a_tile(gpu, cons, n_dst):
    T = tile()
    sizes = {"0": 0, "1": 1, "T-1": T - 1, "T": T, "T+1": T + 1}
    for k, n_src in enumerate(sizes.values()):
        inp = raw_inputs(100 * k + sizes[n_dst], sizes[n_dst], n_src, spread_pairs(n_src, sizes[n_dst]), extra_room=k % 2)
        want = check(gpu, cons, inp)
        assert want["call_verdict"][0] == K.OK and want["counts_out"][2] == len(spread_pairs(n_src, sizes[n_dst]))


def test_destination_rows_beyond_one_pass_of_the_tile_sums(gpu, cons):
    T = tile()
    n_dst, n_src = 256 * T + 3, T + 1
    pairs = [(0, n_dst - 1), (T, 255 * T), (T - 1, 256 * T + 1), (5, 7)]
    inp = raw_inputs(5, n_dst, n_src, pairs, dst_long={256 * T: 70, 256 * T + 2: 65}, src_long={T: 66})
    want = check(gpu, cons, inp)
    assert want["call_verdict"][0] == K.OK and want["counts_out"][0] > n_dst + T // 2 and want["counts_out"][2] == 4


def test_rows_at_the_wave_walks_boundaries_on_both_sides_of_a_tile_boundary(gpu, cons):
    """source rows of 0, 1, 63, 64, 65 and 300 observations below and above row T, mapped and new; destination rows long enough
    that old list + mapped list crosses 64 either way"""
    T = tile()
    lengths = (0, 1, 63, 64, 65, 300)
    src_long = {T - 6 + k: n for k, n in enumerate(lengths)}                       # rows T-6 .. T-1
    src_long.update({T + k: n for k, n in enumerate(reversed(lengths))})           # rows T .. T+5
    src_long.update({T + 10 + k: n for k, n in enumerate(lengths)})                # the same lengths again, unmapped
    dst_long = {T - 2: 64, T - 1: 60, T: 3, T + 1: 65, T + 2: 300, 7: 0}
    pairs = [(T - 6 + k, d) for k, d in enumerate((T - 2, T - 1, T, T + 1, T + 2, 7))]
    pairs += [(T + k, d) for k, d in enumerate((20, 21, 2 * T - 1, 2 * T, 2 * T + 1, 2 * T + 2))]
    inp = raw_inputs(9, 2 * T + 5, T + 40, pairs, dst_long=dst_long, src_long=src_long)
    want = check(gpu, cons, inp)
    assert want["call_verdict"][0] == K.OK and want["counts_out"][2] == len(pairs) and want["counts_out"][5] > 0
    keys = want["src_key_out"]
    assert keys[T - 1] == 7 and want["obs_counts_out"][7] > 200                    # an empty row takes most of 300
    assert keys[T - 2] == T + 2 and want["obs_counts_out"][T + 2] > 300 + 40       # 300 old, most of 65 kept
    assert np.all(keys[T + 10 + np.arange(1, 6)] >= 2 * T + 5)                     # new rows
    skipped = dict(inp, skip=np.array([1 if k % 3 == 0 else 0 for k in range(len(SRC_BLOCKS))], np.uint32))
    check(gpu, cons, skipped)


LDS_BLOCKS = 65536                       # kIrLdsBlocks of cv_amd/csrc/rs_reconstruction_merge.hip:46


def many_blocks_case(n_blocks, dst_blocks, src_views, cap, skip=None):
    """Two small clean tables in a pool of n_blocks blocks.  The destination's rows name dst_blocks in turn and, once, a block
    that is not the pool's; the source's name src_views, the bridging frame's block 2 and a block that is not the pool's."""
    outside = n_blocks + 3
    bridge = 2
    dst_rows = [[(b, k % cap)] + ([(bridge, 0)] if k == 0 else []) for k, b in enumerate(dst_blocks)] + [[(dst_blocks[0], cap - 1), (outside, 0)], []]
    src_rows = [[(v, f) for v in src_views] for f in range(cap)] + [[(bridge, 1)], [(outside, 0)]]
    pairs = [(0, 1), (len(src_rows) - 2, 0)]
    inp = K.incorporate_inputs(dst_rows, src_rows, pairs, src_views, bridge, cap=cap, n_blocks=8, skip=skip, seed=n_blocks)
    few = inp["poses"]
    inp["poses"] = np.ascontiguousarray(few[np.arange(n_blocks) % len(few)] + (np.arange(n_blocks) // len(few))[:, None] * 1e-3)
    inp["n_blocks"] = n_blocks
    return inp


@pytest.mark.parametrize("n_blocks", [LDS_BLOCKS, LDS_BLOCKS + 1])
def test_destination_blocks_on_either_side_of_the_lds_bitmap(gpu, cons, n_blocks):
    """cv_amd/csrc/rs_reconstruction_merge.hip:115, k_ir_check: `in_lds = n_blocks <= kIrLdsBlocks` with kIrLdsBlocks = 65536
    — up to 65536 blocks the destination's blocks are marked in an LDS bitmap and its set bits handed on, above it they go to
    the block words with global atomics.  65536 is the last size of the first branch, 65537 the first of the second.  The
    destination names block 0, block 65535 (the last bit of the bitmap's last word) and, at 65537, block 65536; the source's
    views lie on both sides of them.  Kept marks and destination marks must be the statement's: a clean merge where the views
    are no destination's, SHARED_BLOCK where a kept view is block 65535 or block 65536 — a mark missed at the edge would merge,
    one too many would refuse.  An observation whose block is not the pool's is skipped by both branches: it marks nothing, and
    the row keeps it as it is.  cap_per_img 1 and 2."""
    top = n_blocks - 1
    dst_blocks = [0, LDS_BLOCKS - 1] + ([LDS_BLOCKS] if n_blocks > LDS_BLOCKS else [])
    for cap in (1, 2):
        # the source's views around the destination's blocks: nothing shared
        clean = many_blocks_case(n_blocks, dst_blocks, [1, LDS_BLOCKS - 3, LDS_BLOCKS - 2], cap)
        want = check(gpu, cons, clean, statement=True)
        assert want["call_verdict"][0] == K.OK and want["counts_out"][2] == 2 and want["counts_out"][5] >= 2
        assert np.any(want["obs_out"][:, 0] == n_blocks + 3)                       # the outside observation stays in its row
        skipped = many_blocks_case(n_blocks, dst_blocks, [1, LDS_BLOCKS - 3, top], cap, skip=[0, 0, 1])
        assert check(gpu, cons, skipped, statement=True)["call_verdict"][0] == K.OK    # a skipped view is not kept: at 65536 blocks `top` is the destination's and refuses nothing
        # a kept view that the destination names: the first block, the last bit of the bitmap, the block above it
        for shared in dst_blocks:
            both = many_blocks_case(n_blocks, dst_blocks, [1, LDS_BLOCKS - 3, shared], cap)
            assert check(gpu, cons, both, statement=True)["call_verdict"][0] == K.SHARED_BLOCK, shared
    if n_blocks > LDS_BLOCKS:
        # the destination stops below the boundary, the source's views straddle it
        straddle = many_blocks_case(n_blocks, [0, LDS_BLOCKS - 1], [LDS_BLOCKS - 2, LDS_BLOCKS], 2)
        assert check(gpu, cons, straddle, statement=True)["call_verdict"][0] == K.OK


@pytest.mark.parametrize("name", list(K.designed_incorporate_cases()))
def test_designed_cases(gpu, cons, name):
    from test_reconstruction_merge_math import BAD_TABLES
    check(gpu, cons, K.designed_incorporate_cases()[name], statement=name not in BAD_TABLES)


@pytest.mark.parametrize("seed", range(6))
def test_random_merges(gpu, cons, seed):
    inp = K.random_incorporate(40 + seed, n_dst=60 + 7 * seed, n_src=50 + 11 * seed, dst_views=12, src_views=14, n_pairs=20, collide=seed % 2 == 0,
                               extra_room=seed % 3)
    check(gpu, cons, inp, statement=True)


def test_the_bytes_do_not_depend_on_arrival_order_or_on_the_call_before(gpu, cons):
    T = tile()
    pairs = spread_pairs(2 * T, 3 * T, n=9)
    inp = raw_inputs(21, 3 * T, 2 * T, pairs, dst_long={5: 200, T: 90}, src_long={0: 300, T - 1: 130, T: 64, T + 1: 65})
    first = device_incorporate(gpu, cons, inp)
    second = device_incorporate(gpu, cons, inp)
    assert_same(second, first)
    other = raw_inputs(22, T + 7, 5, [(0, 0), (1, 1)], src_long={2: 500})          # another shape: the scratch is laid out differently
    check(gpu, cons, other)
    assert_same(device_incorporate(gpu, cons, inp), first)
    assert_same(first, K.incorporate(inp))


def test_a_refused_call_launches_nothing(gpu, cons):
    from cv_amd import _lib
    inp = K.designed_incorporate_cases()["a map of one"]
    fill = K.incorporate_outputs(inp)

    def call(**over):
        try:
            got = device_incorporate(gpu, cons, inp, over=over)
        except _lib.AkzError as e:
            return e.status, None
        return 0, got

    # device_incorporate makes fresh buffers per call; a refused one returns before it reads them back, so look at a call that
    # is refused behind an accepted layout: the same arguments with one room too small, then the block list broken
    for over in (dict(obs_room=inp["obs_room"] - 1), dict(lm_room=inp["lm_room"] - 1), dict(src_blocks=[6, 7, 7]), dict(src_blocks=[6, 7, 4]),
                 dict(src_blocks=[6, 7, 99])):
        assert call(**over)[0] == -1, over
    status, got = call()
    assert status == 0 and got["call_verdict"][0] == K.OK
    # and in place: buffers the refused call was handed keep every byte
    from cv_amd.reconstruction_merge import ReconstructionMerge
    up = uploader(gpu)
    d_in = {k: up(inp[k]) for k in ("dst_start", "dst_obs", "src_start", "src_obs", "map", "map_count", "src_pose")}
    d = {k: up(fill[k]) for k in K.IR_OUTPUTS}
    with pytest.raises(_lib.AkzError):
        ReconstructionMerge(cons).incorporate_device(
            d_in["dst_start"], d_in["dst_obs"], inp["n_dst_obs"], inp["n_dst"], d_in["src_start"], d_in["src_obs"], inp["n_src_obs"], inp["n_src"],
            d_in["map"], d_in["map_count"], inp["map_room"], inp["cap"], inp["n_blocks"], [6, 7, 8], inp["bridge_block"], d_in["src_pose"], None,
            inp["obs_room"], inp["lm_room"] - 1, *(d[k] for k in K.IR_OUTPUTS))
    with pytest.raises(_lib.AkzError):                                              # an output over the source table
        ReconstructionMerge(cons).incorporate_device(
            d_in["dst_start"], d_in["dst_obs"], inp["n_dst_obs"], inp["n_dst"], d_in["src_start"], d_in["src_obs"], inp["n_src_obs"], inp["n_src"],
            d_in["map"], d_in["map_count"], inp["map_room"], inp["cap"], inp["n_blocks"], [6, 7, 8], inp["bridge_block"], d_in["src_pose"], None,
            inp["obs_room"], inp["lm_room"], d["poses"], d_in["src_obs"], *(d[k] for k in K.IR_OUTPUTS[2:]))
    cons.sync()
    assert_same(back(d, fill, K.IR_OUTPUTS), fill)
    assert np.array_equal(back(d_in, inp, ("src_obs",))["src_obs"], inp["src_obs"])


# ---- the map ------------------------------------------------------------------------------------------------------------
def device_merge_map(torch, cons, inp):
    from cv_amd import _lib
    from cv_amd.reconstruction_merge import ReconstructionMerge
    up = uploader(torch)
    d_in = {k: up(inp[k]) for k in ("matches", "nmatches", "final", "best", "counts", "src_landmarks")}
    want = K.map_outputs(inp)
    d = {k: up(want[k]) for k in ("map", "map_count")}
    ReconstructionMerge(cons).merge_map_device(d_in["matches"], d_in["nmatches"], d_in["final"], d_in["best"], inp["n_world"], inp["n_dst"], inp["cap"],
                                               inp["slot"], d_in["counts"], d_in["src_landmarks"], inp["n_blocks"], inp["bridge_block"], d["map"],
                                               d["map_count"], stream_to_wait=_lib.wait_handle(torch.cuda.current_stream(torch.device("cuda", 0))))
    cons.sync()
    return back(d, want, ("map", "map_count"))


@pytest.mark.parametrize("name", list(K.designed_map_cases()))
def test_designed_maps(gpu, cons, name):
    inp, want = K.designed_map_cases()[name]
    got = device_merge_map(gpu, cons, inp)
    assert_same(got, K.merge_map(inp), ("map", "map_count"))
    assert [tuple(int(v) for v in e) for e in got["map"][:int(got["map_count"][0])]] == want


@pytest.mark.parametrize("n", ["0", "1", "cap"])
def test_the_map_at_match_counts_up_to_the_capacity(gpu, cons, n):
    """cap = 600: features and matches are walked 256 at a time; merged rows, features without a source landmark, matches that
    are not final and matches that name nothing among them"""
    cap, n_dst = 600, 900
    rng = np.random.default_rng(3)
    n = {"0": 0, "1": 1, "cap": cap}[n]
    feats = rng.permutation(cap)[:n]
    matches, final, best = [], [], {}
    for k, j in enumerate(feats):
        j = int(j)
        if k % 7 == 3:
            best[j] = (int(rng.integers(0, n_dst)), int(rng.integers(0, n_dst)))
            matches.append((j, n_dst + cap + j))                                    # slot 1's merged row
        else:
            matches.append((j, int(rng.integers(0, n_dst + (20 if k % 11 == 5 else 0)))))   # some name nothing
        final.append(int(k % 5 != 4))
    src = {int(j): int(1000 + j) for j in rng.permutation(cap)[:450]}
    inp = K.map_inputs(matches, final=final, cap=cap, n_world=n_dst, n_dst=n_dst, best=best or None, src_landmarks=src)
    got = device_merge_map(gpu, cons, inp)
    assert_same(got, K.merge_map(inp), ("map", "map_count"))
    count = int(got["map_count"][0])
    assert (count == 0) == (n == 0 or (n == 1 and int(feats[0]) not in src)) and (n < cap or 250 < count < 450)
    assert np.all(np.diff(got["map"][:count, 0].astype(np.int64)) > 0)              # ascending feature order (source keys are 1000 + feature)


# ---- normalise -----------------------------------------------------------------------------------------------------------
def device_normalize(torch, cons, inp):
    from cv_amd import _lib
    from cv_amd.reconstruction_merge import ReconstructionMerge
    up = uploader(torch)
    d_in = {k: up(inp[k]) for k in ("counts", "landmarks", "world")}
    want = K.normalize_outputs(inp)
    names = ("poses", "constraint_poses", "stats", "verdict")
    d = {k: up(want[k]) for k in names}
    ReconstructionMerge(cons).normalize_device([int(b) for b in inp["view_blocks"]], d_in["counts"], d_in["landmarks"], inp["cap"], inp["n_blocks"],
                                               d_in["world"], inp["n_world"], d["poses"], d["constraint_poses"] if inp["n_constraints"] else None,
                                               inp["n_constraints"], d["stats"], d["verdict"],
                                               stream_to_wait=_lib.wait_handle(torch.cuda.current_stream(torch.device("cuda", 0))))
    cons.sync()
    return back(d, want, names)


NR_NAMES = ("poses", "constraint_poses", "stats", "verdict")


@pytest.mark.parametrize("n_features", ["0", "1", "255", "256", "257", "cap"])
def test_normalise_over_feature_and_view_counts(gpu, cons, n_features):
    """the mean, the poses and the constraint translations are the host build's bits; NOT_NORMAL leaves every byte as it was"""
    cap = 700
    n = {"0": 0, "1": 1, "255": 255, "256": 256, "257": 257, "cap": cap}[n_features]
    for n_views in (1, 2, 300):
        inp = K.normalize_inputs(1000 + n + n_views, n, n_views, cap=cap, w_zero=(3,), none=(5, 6), no_landmark=(9,), n_constraints=n_views % 3 * 130)
        want = K.normalize(inp)
        got = device_normalize(gpu, cons, inp)
        assert_same(got, want, NR_NAMES)
        assert want["verdict"][0] == (K.NR_NOT_NORMAL if n == 0 else K.NR_OK)
        if n == 0:
            assert np.array_equal(got["poses"], inp["poses"]) and np.array_equal(got["constraint_poses"], inp["constraint_poses"])
        K.check_normalize_against_statement(inp, got, BOUND)


@pytest.mark.parametrize("name", list(K.designed_normalize_cases()))
def test_designed_normalisations(gpu, cons, name):
    inp = K.designed_normalize_cases()[name]
    got = device_normalize(gpu, cons, inp)
    assert_same(got, K.normalize(inp), NR_NAMES)
    K.check_normalize_against_statement(inp, got, BOUND)


def test_bad_indices_of_a_normalisation_write_nothing(gpu, cons):
    inp = K.normalize_inputs(3, 4, 3)
    outside = dict(inp, view_blocks=np.array([inp["view_blocks"][0], inp["n_blocks"]], np.uint32))
    above = dict(inp, counts=np.where(inp["counts"] > 0, inp["cap"] + 1, 0).astype(np.uint32))
    for case in (outside, above):
        got = device_normalize(gpu, cons, case)
        assert_same(got, K.normalize(case), NR_NAMES)
        assert got["verdict"][0] == K.NR_BAD_INDEX and np.array_equal(got["poses"], inp["poses"])


# ---- the chain and the native mirror ---------------------------------------------------------------------------------------
def two_reconstructions(seed=4, n_views=12, n_landmarks=500):
    """One observation_filter_checker scene cut in two: the destination holds blocks [0, 6) and, after its add_views, the
    bridging frame's block 6; the source holds blocks [6, 12).  A landmark seen on both sides has a row in each table; where
    the bridging frame sees it and the destination saw it before, the frame's feature is a final match of its landmark."""
    import observation_filter_checker as F
    sc = F.scene(seed, n_views=n_views, n_landmarks=n_landmarks, lengths=(4, 9), outlier_fraction=0.0)
    half = bridge = n_views // 2
    cap = sc["kps"].shape[1]
    start, obs = sc["start"].astype(np.int64), sc["obs"].astype(np.int64)
    dst_rows, src_rows, matches, src_lm = [], [], [], np.full((n_views, cap), K.NONE, np.uint32)
    for l in range(n_landmarks):
        row = [(int(b), int(f)) for b, f in obs[start[l]:start[l + 1]]]
        d_old = [o for o in row if o[0] < half]
        at_bridge = [o for o in row if o[0] == bridge]
        s = [o for o in row if o[0] >= half]
        if s:
            for b, f in s:
                src_lm[b, f] = len(src_rows)
            src_rows.append(s)
        if d_old:
            if at_bridge:
                matches.append((at_bridge[0][1], len(dst_rows)))
            dst_rows.append(d_old + at_bridge)
        elif at_bridge:                                                             # add_landmark: the frame's feature alone
            dst_rows.append(at_bridge)
    counts = np.array([int(obs[obs[:, 0] == b, 1].max(initial=-1)) + 1 for b in range(n_views)], np.uint32)
    m = np.full((1, cap, 2), K.FILL32, np.uint32)
    m[0, :len(matches)] = np.array(matches, np.uint32)
    fm = np.zeros((1, cap), np.uint8)
    fm[0, :len(matches)] = 1
    return dict(sc=sc, cap=cap, n_views=n_views, half=half, bridge=bridge, dst_rows=dst_rows, src_rows=src_rows, matches=m, final=fm,
                nmatches=np.array([len(matches)], np.uint32), counts=counts, src_landmarks=src_lm, n_matches=len(matches))


def test_merge_reconstructions_waits_once_and_its_world_table_is_the_host_tables(gpu, cons, monkeypatch):
    from test_gpu_landmark_table import rs_camera
    from cv_amd import _lib, triangulation
    from cv_amd.covisibility import Covisibility
    from cv_amd.reconstruction import ObservationFilter, merge_reconstructions
    torch = gpu
    dev = torch.device("cuda", 0)
    two = two_reconstructions()
    sc, cap, n_views, bridge = two["sc"], two["cap"], two["n_views"], two["bridge"]
    dst_table, src_table = triangulation.LandmarkTable(torch, lists=two["dst_rows"]), triangulation.LandmarkTable(torch, lists=two["src_rows"])
    d_poses, d_kps = torch.from_numpy(sc["poses"].copy()).to(dev), _lib.device_bytes(torch, sc["kps"].view(np.uint8), dev)
    cam, prm = rs_camera(sc["cam"]), ObservationFilter.params(minimum_robust_landmarks=8)
    cv = Covisibility.params(optimization_robust_covisibility_minimum_landmarks=4, optimization_minimum_landmarks=4)
    src_pose = sc["poses"][bridge].copy()
    torch.cuda.synchronize()
    waits = []
    monkeypatch.setattr(type(cons), "sync", lambda self, _f=type(cons).sync: (waits.append("rs_sync"), _f(self))[1])
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: waits.append("synchronize"))
    merge_map, merged, (world, reason), result = merge_reconstructions(
        torch, cons, dst_table, src_table, d_kps, cap, cam, d_poses, (0, two["half"]), (two["half"], n_views), bridge, src_pose, 0, two["matches"],
        two["nmatches"], two["final"], two["counts"], two["src_landmarks"], params=prm, cv_params=cv)
    assert waits == ["rs_sync"]
    monkeypatch.undo()
    # the host build of the same two steps
    minp = dict(matches=two["matches"], nmatches=two["nmatches"], final=two["final"], best=None, n_world=dst_table.n_landmarks,
                n_dst=dst_table.n_landmarks, cap=cap, slot=0, counts=two["counts"], src_landmarks=two["src_landmarks"], n_blocks=n_views,
                bridge_block=bridge)
    hmap = K.merge_map(minp)
    n_map = int(hmap["map_count"][0])
    assert n_map == two["n_matches"] > 50
    u32 = lambda t: t.cpu().numpy().view(np.uint32)
    assert np.array_equal(u32(merge_map.map).reshape(-1, 2)[:n_map], hmap["map"][:n_map]) and int(u32(merge_map.map_count)[0]) == n_map
    inp = K.incorporate_inputs(two["dst_rows"], two["src_rows"], [tuple(int(v) for v in e) for e in hmap["map"][:n_map]],
                               list(range(two["half"] + 1, n_views)), bridge, cap=cap, n_blocks=n_views, map_room=cap, pad=0)
    inp["poses"], inp["src_pose"] = sc["poses"].copy(), src_pose
    host = K.incorporate(inp)
    rows, total = int(host["counts_out"][0]), int(host["counts_out"][1])
    assert host["call_verdict"][0] == K.OK and host["counts_out"][2] == n_map and int(u32(merged.call_verdict)[0]) == K.OK
    assert np.array_equal(u32(merged.counts_out), host["counts_out"])
    assert np.array_equal(u32(merged.obs_start_out), host["start_out"]) and np.array_equal(u32(merged.obs_out)[:total], host["obs_out"][:total])
    assert np.array_equal(u32(merged.landmarks_out), host["landmarks_out"]) and np.array_equal(u32(merged.src_key_out), host["src_key_out"])
    # the world table of the merged reconstruction: the triangulation of the host's table with exactly the filled counts
    table = triangulation.LandmarkTable(torch, start=host["start_out"][:rows + 1], obs=host["obs_out"][:total])
    h_poses = torch.from_numpy(host["poses"]).to(dev)
    w2, r2 = table.new_world(), torch.zeros((rows,), dtype=torch.uint8, device=dev)
    triangulation.triangulate_landmarks_device(cons._h, table, d_kps, cap, n_views, h_poses, cam, prm.triangulate, w2, r2,
                                               _lib.wait_handle(torch.cuda.current_stream(dev)))
    cons.sync()
    w, r = world.cpu().numpy(), reason.cpu().numpy()
    assert np.array_equal(w[:rows].view(np.uint64), w2.cpu().numpy().view(np.uint64)) and np.array_equal(r[:rows], r2.cpu().numpy())
    assert np.all(r[rows:] == _lib.TRI_TOO_FEW) and (r[:rows] == _lib.TRI_OK).sum() > 100
    assert result.world.shape[0] >= rows


def test_the_native_mirror_gives_the_same_table(gpu, cons, tmp_path):
    """cv_sfm::ReconstructionMerge of include/akaze.hpp from a process without Python (tests/cpp/reconstruction_merge.cpp)"""
    import subprocess

    import host_build
    inp = K.random_incorporate(77, n_dst=80, n_src=70, dst_views=12, src_views=14, n_pairs=20, extra_room=0)
    want = K.incorporate(inp)
    skip = inp["skip"] if inp["skip"] is not None else np.zeros(len(inp["src_blocks"]), np.uint32)
    path = tmp_path / "call.bin"
    with open(path, "wb") as fp:
        fp.write(np.array([inp["n_blocks"], inp["cap"], inp["n_dst"], inp["n_dst_obs"], inp["n_src"], inp["n_src_obs"], inp["map_room"],
                           len(inp["src_blocks"]), inp["bridge_block"], int(inp["skip"] is not None)], np.uint32).tobytes())
        for a in (inp["dst_start"], inp["dst_obs"][:inp["n_dst_obs"]], inp["src_start"], inp["src_obs"][:inp["n_src_obs"]], inp["map"][:inp["map_room"]],
                  inp["map_count"], inp["src_blocks"], skip, inp["src_pose"], inp["poses"]):
            fp.write(np.ascontiguousarray(a).tobytes())
    exe = host_build.native(tmp_path, "reconstruction_merge.cpp", hip=True)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("reconstruction_merge ok"), (r.returncode, r.stderr[-400:])
    out = {line.split(" ", 1)[0]: line.split()[1:] for line in r.stdout.splitlines()[:-1]}
    num = lambda k: np.array(out[k], np.int64)
    rows, n = (int(v) for v in want["counts_out"][:2])
    assert np.array_equal(num("counts"), want["counts_out"]) and np.array_equal(num("start"), want["start_out"][:rows + 1])
    assert np.array_equal(num("obs"), want["obs_out"][:n].reshape(-1)) and np.array_equal(num("landmarks"), want["landmarks_out"].reshape(-1))
    assert np.array_equal(num("obs_counts"), want["obs_counts_out"][:rows]) and np.array_equal(num("src_key"), want["src_key_out"][:inp["n_src"]])
    assert num("call").tolist() == [K.OK] and want["counts_out"][2] >= 3 and want["counts_out"][4] >= 10
    assert np.array_equal(np.array(out["poses"], np.float64), want["poses"].reshape(-1))
