"""The host's execution of include/akz_reconstruction_merge_math.h (tests/cpp/reconstruction_merge_host.c through
host_build.load) held to the independent statement of tests/reconstruction_merge_statement.py: every integer output exactly,
rows as lists in the documented order; poses, the mean and the scaled translations under one bound.  No GPU needed — the
device is held to this host build byte for byte in tests/test_gpu_reconstruction_merge.py.

The bound: the largest absolute difference from the float64 statement (numpy's inverse and matmul) over every scene of this
file — rotations from random axis-angles, |t| <= 10, points at distance 1 to 20 — was measured as MEASURED_MAX; the tests
assert 4 times that, the margin for numpy's matmul order differing between builds.  The products are of at most three
orthonormal matrices, so the measured maximum itself has to lie below 1e-12 (asserted)."""
import numpy as np
import pytest

import reconstruction_merge_checker as K
import reconstruction_merge_statement as S

MEASURED_MAX = 1.0658141036401503e-14
BOUND = 4 * MEASURED_MAX

INCORPORATE = K.designed_incorporate_cases()
BAD_TABLES = ("descending starts in the destination", "descending starts in the source", "a last start above n_obs")
NORMALIZE = K.designed_normalize_cases()
MAPS = K.designed_map_cases()


def test_the_bound_is_the_measured_one_and_small():
    assert MEASURED_MAX < 1e-12 and BOUND == 4 * MEASURED_MAX


@pytest.mark.parametrize("name", [n for n in INCORPORATE if n not in BAD_TABLES])
def test_designed_incorporations_equal_the_statement(name):
    inp = INCORPORATE[name]
    st, _ = K.check_incorporate_against_statement(inp, K.incorporate(inp), BOUND)
    want = {"a block in both tables": S.SHARED_BLOCK, "a kept feature at the capacity": S.BAD_INDEX}.get(name, S.OK)
    assert st["verdict"] == want


def test_what_the_designed_incorporations_decide():
    run = lambda name: K.incorporate(INCORPORATE[name])
    counts = lambda name: [int(v) for v in run(name)["counts_out"]]
    n_dst, dst_obs = 6, 12
    assert counts("an empty map") == [n_dst + 5, dst_obs + 10, 0, 0, 5, 3]                   # source rows 3 and 5 take no key
    assert counts("a map of one") == [n_dst + 4, dst_obs + 10, 1, 0, 4, 3]
    assert counts("every source landmark mapped") == [n_dst, dst_obs + 7, 6, 0, 0, 3]
    assert counts("two entries with one destination")[2:4] == [1, 2] and counts("two entries with one source")[2:4] == [1, 2]
    assert counts("an entry that names a landmark outside the source")[2:4] == [1, 1]
    assert counts("an entry that names a landmark outside the destination")[2:4] == [1, 1]
    assert counts("an outside entry still names its other landmark")[2:4] == [0, 2]
    assert counts("a source whose every observation is the bridging frame's") == [n_dst, dst_obs, 1, 0, 0, 2]
    o = run("source tombstones")
    assert [int(v) for v in o["src_key_out"][:5]] == [K.NONE, 6, K.NONE, 0, K.NONE] and int(o["counts_out"][4]) == 1
    o = run("a map of one")
    assert K.out_rows(o)[2] == [(0, 1), (2, 1), (3, 1), (4, 1), (6, 0), (7, 0)]             # the old list, then the source's kept ones
    assert [int(v) for v in o["src_key_out"][:7]] == [2, 6, 7, K.NONE, 8, K.NONE, 9]
    assert counts("a skipped view")[5] == 3 + 3 and counts("every view skipped") == [n_dst, dst_obs, 1, 0, 0, 13]
    assert counts("a map count above its room")[2:4] == [2, 0] and counts("a map count below its room")[2:4] == [1, 0]


@pytest.mark.parametrize("name", BAD_TABLES)
def test_a_broken_table_is_refused_and_the_destination_stays(name):
    inp = INCORPORATE[name]
    o = K.incorporate(inp)
    assert int(o["call_verdict"][0]) == S.BAD_TABLE
    assert np.array_equal(o["poses"], inp["poses"])
    assert np.all(o["src_key_out"][:inp["n_src"]] == K.NONE) and np.all(o["landmarks_out"][5:] == K.NONE)
    if "destination" in name:                                    # its own starts are broken: as many empty rows
        assert [int(v) for v in o["counts_out"]] == [inp["n_dst"], 0, 0, 0, 0, 0]
        assert np.all(o["start_out"] == 0) and np.all(o["obs_counts_out"][:inp["lm_room"]] == 0) and np.all(o["landmarks_out"] == K.NONE)
        assert np.all(o["obs_out"] == K.FILL32)
    else:
        assert [int(v) for v in o["counts_out"]] == [inp["n_dst"], 12, 0, 0, 0, 0]
        assert K.out_rows(o) == [list(r) for r in K.dst_small()]
        assert np.all(o["start_out"][inp["n_dst"]:] == 12) and np.all(o["obs_counts_out"][inp["n_dst"]:inp["lm_room"]] == 0)


@pytest.mark.parametrize("seed", range(12))
def test_random_incorporations_equal_the_statement(seed):
    inp = K.random_incorporate(seed, n_dst=[30, 0, 7][seed % 3], n_src=[30, 9, 0][(seed // 3) % 3], collide=seed % 2 == 0, extra_room=seed % 4)
    K.check_incorporate_against_statement(inp, K.incorporate(inp), BOUND)


def test_the_transform_is_the_inverse_of_from_camera_poses():
    """pose.rs:322-324 gives world_transform = inverse(b) * a; lib.rs:1824 inverts it: inverse(a) * b, formed directly here"""
    rng = np.random.default_rng(5)
    for _ in range(50):
        a, b = K.random_pose(rng), K.random_pose(rng)
        t = np.zeros(12)
        K.lib().mr_transform(a.ctypes.data, b.ctypes.data, t.ctypes.data)
        want = np.linalg.inv(np.linalg.inv(S.pose4(b)) @ S.pose4(a))[:3].reshape(12)
        assert np.max(np.abs(t - want)) <= BOUND


@pytest.mark.parametrize("name", list(MAPS))
def test_designed_maps(name):
    inp, want = MAPS[name]
    o = K.merge_map(inp)
    n = int(o["map_count"][0])
    assert [tuple(int(v) for v in e) for e in o["map"][:n]] == want
    assert np.all(o["map"][n:] == K.FILL32)                     # entries behind the count are not written


def test_the_map_is_the_statements_on_clean_matches():
    rng = np.random.default_rng(11)
    for _ in range(20):
        cap = 16
        feats = rng.permutation(cap)[:rng.integers(0, cap + 1)]
        src = {int(j): int(100 + j) for j in rng.permutation(cap)[:12]}
        matches = [(int(j), int(rng.integers(0, 6))) for j in feats]
        o = K.merge_map(K.map_inputs(matches, cap=cap, src_landmarks=src))
        view_landmarks = [src.get(j) for j in range(cap)]
        want = S.merge_map({j: [d] for j, d in matches}, view_landmarks)
        assert [tuple(int(v) for v in e) for e in o["map"][:int(o["map_count"][0])]] == want


@pytest.mark.parametrize("name", list(NORMALIZE))
def test_designed_normalisations_equal_the_statement(name):
    inp = NORMALIZE[name]
    o = K.normalize(inp)
    K.check_normalize_against_statement(inp, o, BOUND)
    not_normal = name in ("no robust point", "no feature", "only points at w == 0")
    assert int(o["verdict"][0]) == (S.NR_NOT_NORMAL if not_normal else S.NR_OK)
    if not_normal:
        assert o["stats"][0] == 0.0 and o["stats"][1] == 0.0
    if name == "a point at w == 0":
        assert o["stats"][1] == 4.0
    if name == "one point":
        first = o["poses"][inp["view_blocks"][0]].reshape(3, 4)
        assert np.max(np.abs(first - np.eye(3, 4))) <= BOUND                                   # the first view is the origin


@pytest.mark.parametrize("n_features,n_views", [(0, 1), (1, 2), (255, 300), (256, 2), (257, 1), (700, 300)])
def test_normalisations_over_the_thread_counts_equal_the_statement(n_features, n_views):
    inp = K.normalize_inputs(100 + n_features, n_features, n_views, w_zero=(3,), none=(5, 6))
    o = K.normalize(inp)
    K.check_normalize_against_statement(inp, o, BOUND)


def test_bad_indices_of_a_normalisation_write_nothing():
    inp = K.normalize_inputs(3, 4, 3)
    outside = dict(inp, view_blocks=np.array([inp["view_blocks"][0], inp["n_blocks"]], np.uint32))
    above = dict(inp, counts=np.where(inp["counts"] > 0, inp["cap"] + 1, 0).astype(np.uint32))
    for case in (outside, above):
        o = K.normalize(case)
        assert int(o["verdict"][0]) == S.NR_BAD_INDEX and np.array_equal(o["poses"], inp["poses"])
        assert np.array_equal(o["constraint_poses"], inp["constraint_poses"])
        K.check_normalize_against_statement(case, o, BOUND)


def test_is_normal_is_rusts():
    L = K.lib()
    tiny = np.finfo(np.float64).tiny
    for x, want in ((1.0, 1), (-2.5, 1), (0.0, 0), (-0.0, 0), (tiny, 1), (tiny / 2, 0), (np.inf, 0), (-np.inf, 0), (np.nan, 0),
                    (np.finfo(np.float64).max, 1)):
        assert L.mr_is_normal(float(x)) == want, x
