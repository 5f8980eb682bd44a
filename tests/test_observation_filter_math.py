"""The host build of include/akz_observation_filter_math.h (tests/observation_filter_checker.py) held to the independent numpy
statement of cv-sfm's filter_non_robust_observations (tests/observation_filter_statement.py).

Decisions are compared EXACTLY: keep flags, states, triangulator reasons, robust bits, counts, verdicts and both compacted
lists.  The two sides find a landmark's point with different eigen-solvers (cyclic Jacobi / LAPACK), so a decision can differ
only where a distance lies within the solvers' rounding of its threshold.  Measured on the scenes below, the largest difference
between the two sides' distances is 5.6e-16 for the cosine distance (threshold 1e-5) and 1.5e-16 for the sine distance of a pair
(threshold 1e-1; no solver there, only the order of the products).  The exclusion band is 4 times the measured value, the cap on
excluded landmarks is zero: the seeds are chosen so that the statement alone finds no distance inside the band, and that is
asserted before anything is compared."""
import numpy as np
import pytest

import observation_filter_checker as F
import observation_filter_statement as S

MEASURED_COSINE, MEASURED_SINE = 5.6e-16, 1.5e-16
BAND_COSINE, BAND_SINE = 4 * MEASURED_COSINE, 4 * MEASURED_SINE
KEYS = ("keep", "state", "reason", "robust", "verdict", "stats", "start_out", "obs_out", "split_out", "counts")


def both(sc, recon_start, view_start, skip=None, **kw):
    h = F.filter_table(sc["kps"], sc["poses"], sc["cam"], sc["start"], sc["obs"], recon_start, view_start, F.settings(**kw), skip=skip,
                       distance=True)
    s = S.filter_table(sc["kps"], sc["poses"], sc["cam5"], sc["start"], sc["obs"], recon_start, view_start, S.settings(**kw), skip=skip)
    return h, s


def assert_outside_band_then_equal(sc, h, s):
    n_lm = len(sc["start"]) - 1
    lens = np.diff(sc["start"].astype(np.int64))
    pair_second = np.zeros(len(sc["obs"]), bool)
    pair_second[sc["start"][:-1][lens == 2].astype(np.int64) + 1] = True
    m = s["compared"] & ~np.isnan(s["dist"])
    cos, sin = m & ~pair_second, m & pair_second
    hd = h["dist"][:len(sc["obs"])]
    worst_cos = np.abs(hd[cos] - s["dist"][cos]).max() if cos.any() else 0.0
    worst_sin = np.abs(hd[sin] - s["dist"][sin]).max() if sin.any() else 0.0
    print("largest distance difference, host build - statement: cosine %.3g sine %.3g" % (worst_cos, worst_sin))
    assert worst_cos <= BAND_COSINE and worst_sin <= BAND_SINE
    # nothing the statement compared lies where the solvers' rounding could decide
    assert not np.any(np.abs(s["dist"][cos] - 1e-5) <= BAND_COSINE)
    assert not np.any(np.abs(s["dist"][sin] - 1e-1) <= BAND_SINE)
    for k in KEYS:
        want = s[k]
        got = h[k][:len(want)]
        assert np.array_equal(got, want), k
    # behind the valid rows the host build wrote nothing
    kept, split = (int(c) for c in s["counts"])
    assert np.all(h["obs_out"][kept:] == F.FILL32) and np.all(h["split_out"][split:] == F.FILL32)
    assert h["start_out"][n_lm] == kept


@pytest.mark.parametrize("seed", [1, 2])
def test_scene_decisions_equal_the_statement(seed):
    """12 views, 4 000 landmarks of 3 to 8 observations, 0.5 px noise, 30 % of them with one observation displaced by 40 to 120 px"""
    sc = F.scene(seed)
    n_lm = len(sc["start"]) - 1
    h, s = both(sc, np.array([0, n_lm], np.uint32), np.array([0, 12], np.uint32))
    near = (s["dist"] > 0.5e-5) & (s["dist"] < 2e-5)
    assert 0.02 < near.sum() / len(sc["obs"]) < 0.05          # the threshold cuts through the populated part of the distribution
    assert_outside_band_then_equal(sc, h, s)
    st = h["stats"][0]
    assert st[F.S_LANDMARKS] == n_lm and 0.2 < st[F.S_OBS_SPLIT] / len(sc["obs"]) < 0.35 and st[F.S_KICKED] > 1000
    # every observation of the list beyond the threshold: the last one in list order stays
    all_fail = [l for l in np.flatnonzero(h["state"][:n_lm] == F.KICKED) if np.all(s["dist"][sc["start"][l]:sc["start"][l + 1]] > 1e-5)]
    assert len(all_fail) > 500
    for l in all_fail:
        k = h["keep"][sc["start"][l]:sc["start"][l + 1]]
        assert k[-1] == 1 and not k[:-1].any()
    assert h["verdict"][0] == F.OK and st[F.S_ROBUST_AFTER] < st[F.S_ROBUST_BEFORE]


def test_mixed_lengths_three_reconstructions_equal_the_statement():
    """lists of 0 to 8 (singles, pairs with the sine test), three reconstructions, the middle one skipped"""
    sc = F.scene(5, n_landmarks=1500, lengths=(0, 8))
    recon_start, view_start, skip = np.array([0, 500, 1100, 1500], np.uint32), np.array([0, 12, 12, 12], np.uint32), np.array([0, 1, 0], np.uint32)
    # the views are shared here: the view ranges only give each reconstruction its count (12, 0, 0)
    h, s = both(sc, recon_start, view_start, skip=skip)
    assert_outside_band_then_equal(sc, h, s)
    assert list(h["verdict"][:3]) == [F.OK, F.RECON_SKIPPED, F.OK]
    assert np.all(h["state"][500:1100] == F.SKIPPED) and np.all(h["robust"][500:1100] == 0)
    assert np.all(h["keep"][sc["start"][500]:sc["start"][1100]] == 1)
    hist = np.bincount(h["state"][:1500], minlength=7)
    assert hist[F.KEPT] and hist[F.SINGLE] and hist[F.PAIR_SPLIT] and hist[F.KICKED] and hist[F.SKIPPED]


# ---- hand-built lists ------------------------------------------------------------------------------------------------
def look_at(centre, target):
    """a WorldToCamera pose [3][4] at `centre` whose +z looks at `target`"""
    z = np.asarray(target, float) - centre
    z /= np.linalg.norm(z)
    x = np.cross([0.0, 1.0, 0.0], z)
    x /= np.linalg.norm(x)
    r = np.stack([x, np.cross(z, x), z])
    return np.hstack([r, (-r @ centre).reshape(3, 1)])


def bearing(pose, X):
    q = pose[:, :3] @ X + pose[:, 3]
    return q / np.linalg.norm(q)


X0 = np.array([0.2, -0.1, 5.0])
CENTRES = [np.array(c, float) for c in ([-1, 0, 0], [1, 0.2, 0], [0, 1, 0.3], [0.5, -1, 0.1])]
POSES = [look_at(c, [0, 0, 5]) for c in CENTRES]


def agree(poses, bearings, n_views=0xFFFFFFFF, **kw):
    """the host build's answer, asserted equal to the statement's"""
    h = F.filter_list(poses, bearings, F.settings(n_views=n_views, **kw))
    s = S.filter_landmark([(np.asarray(p, float).reshape(3, 4), np.asarray(b, float)) for p, b in zip(poses, bearings)], S.settings(**kw), n_views)
    assert h["state"] == s["state"] and list(h["keep"]) == [int(k) for k in s["keep"]] and h["reason"] == s["reason"]
    assert h["robust"] == int(s["before"]) | int(s["after"]) << 1
    assert h["n_split"] == len(s["keep"]) - sum(s["keep"])
    return h, s


def test_nothing_happens_to_lists_of_none_and_one():
    h, _ = agree([], [])
    assert h["state"] == F.SINGLE and h["robust"] == 0 and h["reason"] == F.NO_SOLVE and h["n_split"] == 0
    h, _ = agree(POSES[:1], [bearing(POSES[0], X0)], n_views=1)       # min(3, 1) = 1 observation would do: the pair test needs two
    assert h["state"] == F.SINGLE and list(h["keep"]) == [1] and h["robust"] == 0


def test_pairs_pass_and_fail_the_sine_test():
    good = [bearing(p, X0) for p in POSES[:2]]
    h, s = agree(POSES[:2], good)
    assert h["state"] == F.KEPT and list(h["keep"]) == [1, 1] and s["dist"][1] < 1e-12 and h["reason"] == F.NO_SOLVE
    assert h["robust"] == 0                                            # two observations among many views: fewer than three
    bad = [good[0], bearing(POSES[1], X0 + [0.0, 1.5, 0.0])]           # off the epipolar plane by far more than asin(0.1)
    h, s = agree(POSES[:2], bad)
    assert h["state"] == F.PAIR_SPLIT and list(h["keep"]) == [1, 0] and s["dist"][1] > 0.1 and h["n_split"] == 1


def test_two_views_make_pairs_robust():
    good = [bearing(p, X0) for p in POSES[:2]]
    h, _ = agree(POSES[:2], good, n_views=2)                           # min(3, 2) = 2
    assert h["state"] == F.KEPT and h["robust"] == 3
    h, _ = agree(POSES[:2], good, n_views=3)
    assert h["robust"] == 0
    bad = [good[0], bearing(POSES[1], X0 + [0.0, 1.5, 0.0])]
    h, _ = agree(POSES[:2], bad, n_views=2)
    assert h["state"] == F.PAIR_SPLIT and h["robust"] == 1            # robust before, a single observation after


def test_one_outlier_is_kicked_and_all_failing_leaves_the_last():
    exact = [bearing(p, X0) for p in POSES]
    h, s = agree(POSES, exact)
    assert h["state"] == F.KEPT and h["robust"] == 3 and h["reason"] == 0 and max(s["dist"]) < 1e-12
    # a small displacement of one observation of four: the other three outvote it
    one = list(exact)
    one[2] = bearing(POSES[2], X0 + [0.05, 0.0, 0.0])
    h, s = agree(POSES, one)
    assert h["state"] == F.KICKED and list(h["keep"]) == [1, 1, 0, 1] and h["robust"] == 3 and h["n_split"] == 1
    # three observations of three different points: every distance is beyond the threshold, the last stays
    wild = [bearing(POSES[0], X0), bearing(POSES[1], X0 + [0.5, 0.5, 0.0]), bearing(POSES[2], X0 - [0.5, 0.0, 1.0])]
    h, s = agree(POSES[:3], wild)
    assert min(s["dist"]) > 1e-5
    assert h["state"] == F.KICKED and list(h["keep"]) == [0, 0, 1] and h["n_split"] == 2 and h["robust"] == 1


def test_a_point_behind_a_camera_splits_the_landmark():
    flipped = [-bearing(p, X0) for p in POSES[:3]]
    h, _ = agree(POSES[:3], flipped)
    assert h["state"] == F.NO_POINT and h["reason"] == S.TRI_CHEIRALITY and list(h["keep"]) == [1, 0, 0] and h["n_split"] == 2
    assert h["robust"] == 1


def test_a_nan_pose_splits_the_landmark_and_nothing_is_robust():
    poses = [p.copy() for p in POSES[:3]]
    poses[1][0, 0] = np.nan
    h, _ = agree(poses, [bearing(p, X0) for p in POSES[:3]])
    assert h["state"] == F.NO_POINT and h["reason"] == S.TRI_NOT_FINITE and list(h["keep"]) == [1, 0, 0]
    h2, _ = agree(poses[:2], [bearing(p, X0) for p in POSES[:2]], n_views=2)     # a NaN loss counts as 1.0: split
    assert h2["state"] == F.PAIR_SPLIT


def test_a_nan_distance_keeps_the_observation():
    """The comparison is `>`.  Cameras A (at the origin) and B (at (1, 0, 1), looking down -x) see X = (0, 0, 1) along their
    optical axes, camera C stands IN X: pose * point is the zero vector, its bearing 0 / 0.  Every entry is an integer, so the
    design matrix is exact and the host build's Jacobi solver returns (0, 0, 1, 1) exactly."""
    a = np.hstack([np.eye(3), np.zeros((3, 1))])
    rb = np.array([[0.0, 0, 1], [0, 1, 0], [-1, 0, 0]])
    b = np.hstack([rb, (-rb @ np.array([1.0, 0, 1])).reshape(3, 1)])
    c = np.hstack([np.eye(3), np.array([[0.0], [0.0], [-1.0]])])
    z = np.array([0.0, 0.0, 1.0])
    point, why = F.triangulate([a, b, c], [z, z, z])
    assert why == 0 and list(point) == [0.0, 0.0, 1.0, 1.0]
    assert np.isnan(F.transformed_distance(c, point, z))
    assert F.transformed_distance(a, point, z) == 0.0 and F.transformed_distance(b, point, z) == 0.0
    h = F.filter_list([a, b, c], [z, z, z])
    assert h["state"] == F.KEPT and list(h["keep"]) == [1, 1, 1] and h["n_split"] == 0
    # the same camera with a bearing that truly disagrees is still kept: its distance is NaN whatever it saw
    h = F.filter_list([a, b, c], [z, z, np.array([1.0, 0.0, 0.0])])
    assert h["state"] == F.KEPT and list(h["keep"]) == [1, 1, 1]


def test_the_verdict_turns_at_the_minimum():
    sc = F.scene(7, n_landmarks=120)
    n_lm = 120
    rs, vs = np.array([0, n_lm], np.uint32), np.array([0, 12], np.uint32)
    base = F.filter_table(sc["kps"], sc["poses"], sc["cam"], sc["start"], sc["obs"], rs, vs)
    after = int(base["stats"][0, F.S_ROBUST_AFTER])
    assert 32 < after < n_lm and base["verdict"][0] == F.OK
    for minimum, want in ((after, F.OK), (after + 1, F.FEW_LANDMARKS), (0, F.OK)):
        h, s = both(sc, rs, vs, minimum_robust_landmarks=minimum)
        assert h["verdict"][0] == want == s["verdict"][0]
        assert np.array_equal(h["keep"], base["keep"])                  # a rejected reconstruction's table is still written
    assert F.lib().of_verdict(31, 32) == F.FEW_LANDMARKS and F.lib().of_verdict(32, 32) == F.OK


def test_bad_indices_and_bad_ranges_leave_things_as_they_are():
    sc = F.scene(9, n_landmarks=200)
    obs = sc["obs"].copy()
    n_lm = 200
    bad_lm = [3, 64, 199]
    obs[sc["start"][3], 0] = 12                      # a block past the views
    obs[sc["start"][64 + 1] - 1, 1] = 200            # a feature past the capacity, in the list's last place
    obs[sc["start"][199] + 1, 0] = 0xFFFFFFFF
    rs, vs = np.array([0, n_lm], np.uint32), np.array([0, 12], np.uint32)
    h = F.filter_table(sc["kps"], sc["poses"], sc["cam"], sc["start"], obs, rs, vs)
    ref = F.filter_table(sc["kps"], sc["poses"], sc["cam"], sc["start"], sc["obs"], rs, vs)
    for l in range(n_lm):
        a, b = sc["start"][l], sc["start"][l + 1]
        if l in bad_lm:
            assert h["state"][l] == F.BAD_INDEX and h["reason"][l] == S.TRI_BAD_INDEX and h["robust"][l] == 0 and np.all(h["keep"][a:b] == 1)
        else:
            assert h["state"][l] == ref["state"][l] and np.array_equal(h["keep"][a:b], ref["keep"][a:b])
    # start arrays that do not ascend: that reconstruction alone is refused
    rs3, vs3 = np.array([0, 100, 50, 200], np.uint32), np.array([0, 12, 12, 12], np.uint32)
    h = F.filter_table(sc["kps"], sc["poses"], sc["cam"], sc["start"], sc["obs"], rs3, vs3)
    assert h["verdict"][0] == F.OK and h["verdict"][1] == F.BAD_RANGE and h["verdict"][2] == F.BAD_RANGE and np.all(h["stats"][1:3] == 0)
    assert np.all(h["state"][100:200] == F.SKIPPED) and np.array_equal(h["state"][:100], ref["state"][:100])
    start = sc["start"].copy()
    start[150], start[151] = start[151], start[150]            # a descent inside the second reconstruction's part of obs_start
    h = F.filter_table(sc["kps"], sc["poses"], sc["cam"], start, sc["obs"], np.array([0, 100, 200], np.uint32), np.array([0, 12, 12], np.uint32))
    assert h["verdict"][1] == F.BAD_RANGE and h["verdict"][0] != F.BAD_RANGE and np.all(h["keep"] == np.where(np.arange(len(h["keep"])) < sc["start"][100], ref["keep"], 1))
    vs_bad = np.array([0, 13], np.uint32)                        # more views than blocks
    h = F.filter_table(sc["kps"], sc["poses"], sc["cam"], sc["start"], sc["obs"], rs, vs_bad)
    assert h["verdict"][0] == F.BAD_RANGE and np.all(h["state"][:n_lm] == F.SKIPPED)
