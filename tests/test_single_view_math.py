"""include/akz_single_view_math.h as the host compiler builds it (tests/single_view_checker.py) against the independent numpy
statement of the same procedure (tests/single_view_statement.py): poses within four times the measured difference, every
decision equal, and no comparison of the statement's inside the band around its threshold where the two could disagree.  No GPU
needed; tests/test_gpu_single_view.py holds the kernel to this host build bit for bit.

A finding the sanity test records: on a noise-free scene with the true pose perturbed, a run of
single_view_simple_optimize_l2 lowers both summed-gradient norms, the mean cosine distance and the rotation error, and RAISES
the translation error — depth 4 to 10 in a narrow field of view leaves a valley along which a sideways shift and a turn trade
against each other, the run descends into it and the 50-iterations-without-improvement rule ends it there."""
import numpy as np
import pytest

import single_view_checker as V
import single_view_statement as S

RATE = 0.02
# the largest |pose entry of the host build - pose entry of the statement| over CASES, measured with this file's
# test_poses_within_four_times_the_measured_difference (printed there): libm's sin / cos against the portable ones, the
# Euclidean point against the homogeneous transform, the tree against the sequential sum
MEASURED_POSE_DIFFERENCE = 2.33e-14
# the largest |value the host build compares - value the statement compares| in is_observation_consistent over CASES, each side
# under its own final pose
MEASURED_DISTANCE_DIFFERENCE = 2.76e-15

MANY = list(range(0, 90, 3)) + list(range(1, 90, 3))     # two thirds of 90 matches 20 - 40 px off
COUNTS = np.r_[0, 1, 2, 3, 40, 1, 2, 3, 1 + np.arange(82) % 5]
# name -> (rig, settings on top of RATE / patience 400, verdict, stage)
CASES = {
    "ok": (dict(seed=1, n=90, none=(3, 50), outliers=(5, 20, 77), merged=(8, 9), obs_counts=COUNTS), dict(), V.OK, V.STAGE_MINIMUM),
    "cut": (dict(seed=2, n=90, none=(4,), outliers=(6,)), dict(single_view_optimization_num_matches=40), V.OK, V.STAGE_MINIMUM),
    "patience 0": (dict(seed=3, n=80), dict(single_view_patience=0), V.OK, V.STAGE_MINIMUM),
    "patience 1": (dict(seed=3, n=80), dict(single_view_patience=1), V.OK, V.STAGE_MINIMUM),
    "no model": (dict(seed=4, n=80, has_model=False), dict(), V.NO_MODEL, V.STAGE_MODEL),
    "few landmarks": (dict(seed=5, n=40, none=range(0, 40, 4)), dict(), V.FEW_LANDMARKS, V.STAGE_LANDMARKS),
    "lost half in the loop": (dict(seed=6, n=90, outliers=MANY), dict(), V.LOST_HALF, V.STAGE_RUN0 + 1),
    "lost half at the last run": (dict(seed=6, n=90, outliers=MANY), dict(single_view_filter_loop_iterations=1), V.LOST_HALF, V.STAGE_RUN0 + 1),
    "lost half at the final count": (dict(seed=6, n=90, outliers=MANY), dict(single_view_filter_loop_iterations=0), V.LOST_HALF, V.STAGE_FINAL),
    "few robust": (dict(seed=7, n=50), dict(), V.FEW_ROBUST, V.STAGE_MINIMUM),
}


def settings_of(extra):
    kw = dict(single_view_optimization_rate=RATE, single_view_patience=400)
    kw.update(extra)
    return V.settings(**kw), S.settings(**kw)


def others_of(sc):
    return [[(sc.obs_pose[k].reshape(3, 4), sc.obs_bearing[k]) for k in range(int(sc.obs_start[i]), int(sc.obs_start[i + 1]))] for i in range(sc.n)]


_results = {}


def both(name):
    """(rig, scene, host result, statement result, the statement's comparisons), computed once per case"""
    if name not in _results:
        rig_kw, extra, _, _ = CASES[name]
        r = V.Rig(**rig_kw)
        sc = r.scene()
        hst, sst = settings_of(extra)
        near = []
        _results[name] = (r, sc, V.refine(sc, r.pose_in, r.inliers, hst, has_model=r.has_model),
                          S.refine(sc.bearing, sc.world, others_of(sc), r.pose_in, r.inliers, sst, has_model=r.has_model, near=near), near)
    return _results[name]


@pytest.mark.parametrize("name", list(CASES))
def test_every_case_reaches_its_verdict_at_its_stage(name):
    _, _, h, s, _ = both(name)
    assert (h["verdict"], h["stage"]) == CASES[name][2:]
    assert s["verdict"] == h["verdict"]


def test_the_inputs_reach_both_breaks_and_the_small_patiences():
    _, _, h, s, _ = both("ok")
    stops = h["run_stop"][:6]
    assert stops[0] == 399 and (stops < 399).any()                     # the last-iteration break, then the no-improvement break
    assert [w for _, _, w in s["runs"]].count("last") >= 1 and [w for _, _, w in s["runs"]].count("stabilized") >= 1
    r, _, h0, s0, _ = both("patience 0")
    assert list(h0["run_stop"][:6]) == [0] * 6 and np.array_equal(h0["pose"], r.pose_in)      # iterations == 0: the pose untouched
    assert [w for _, _, w in s0["runs"]] == ["exhausted"] * 6
    _, _, h1, s1, _ = both("patience 1")
    assert list(h1["run_stop"][:6]) == [0] * 6 and not np.array_equal(h1["pose"], r.pose_in)  # one step, left by the last-iteration break
    assert [w for _, _, w in s1["runs"]] == ["last"] * 6


def test_poses_within_four_times_the_measured_difference():
    worst = 0.0
    for name in CASES:
        _, _, h, s, _ = both(name)
        if s["pose"] is not None:
            assert h["verdict"] in (V.OK, V.NO_MODEL)
            worst = max(worst, float(np.abs(h["pose"] - s["pose"]).max()))
    print("largest pose difference", worst)
    assert worst <= 4.0 * MEASURED_POSE_DIFFERENCE


def test_decisions_are_equal_and_no_comparison_lies_in_the_band():
    worst = 0.0
    for name in CASES:
        r, sc, h, s, near = both(name)
        hst, sst = settings_of(CASES[name][1])
        for (m, stop, _), hm, hs in zip(s["runs"], h["run_matches"], h["run_stop"]):
            assert m == hm and (stop is None or stop == hs), name                 # selection counts and stopping iterations
        if s["final"] is None:
            continue
        assert np.array_equal(s["final"], h["final"]) and s["robust"] == h["robust"], name
        # the values compared, each side under its own final pose (a rejected scene: under the statement's)
        pose_h = h["pose"] if h["verdict"] == V.OK else None
        others = others_of(sc)
        for i in range(sc.n):
            if pose_h is None or len(others[i]) == 0:
                continue
            mine = []
            S.is_observation_consistent(s["pose"], sc.bearing[i], others[i], sst, mine)
            theirs = V.consistency_values(sc, i, pose_h, hst)
            assert len(mine) == len(theirs), (name, i)
            worst = max(worst, max(abs(a - b) for (a, _), b in zip(mine, theirs)))
        band = 4.0 * MEASURED_DISTANCE_DIFFERENCE
        assert not [(v, t) for v, t in near if abs(v - t) <= band], name
    print("largest difference of a compared value", worst)
    assert worst <= 4.0 * MEASURED_DISTANCE_DIFFERENCE


def test_the_gradient_is_the_statements():
    r = V.Rig(9, 50)
    for i in range(50):
        b = V.bearings_of(r.new_px[i:i + 1])[0]
        w = r.world[i]
        ok, g = V.landmark_delta(r.pose_in, b, V.euclidean(w))
        d = S.landmark_delta(r.pose_in, b, w)
        assert ok and np.allclose(g[:3], d[0], rtol=0, atol=1e-13) and np.allclose(g[3:], d[1], rtol=0, atol=1e-14)
    # Projective::point gives None for w == 0: skipped on both sides; a NaN anywhere zeroes that vector alone
    w = np.array([0.0, 0.0, 1.0, 0.0])
    assert V.landmark_delta(r.pose_in, b, V.euclidean(w))[0] == 0 and S.landmark_delta(r.pose_in, b, w) is None
    g = V.world_pose_gradient(np.zeros(3), b)
    assert np.array_equal(g, np.zeros(6))                             # 0 / 0 in the rotation, the translation is exactly zero


def test_sum_order_costs_what_rounding_allows():
    """akz_sv_sum_tree (shipped) against akz_sv_sum_sequential (the reference's order): each is a sum of n terms whose rounding
    error is at most (n - 1) u sum |g| (u = 2^-53), so the two differ by twice that at the most."""
    r = V.Rig(13, 2048)
    lm = np.hstack([V.bearings_of(r.new_px), r.points])
    tree, seq = V.gradient_sum(r.pose_in, lm), V.gradient_sum(r.pose_in, lm, sequential=True)
    mags = np.zeros(6)
    for i in range(len(lm)):
        mags += np.abs(V.landmark_delta(r.pose_in, lm[i, :3], lm[i, 3:])[1])
    diff = np.abs(tree - seq)
    print("tree - sequential", diff, "relative to the sums", diff / np.abs(seq))
    assert np.all(diff <= 2.0 * 2047 * 2.0 ** -53 * mags) and diff.max() > 0.0
    st, sr = S.gradient_sum(r.pose_in, [(lm[i, :3], r.world[i]) for i in range(len(lm))])
    assert np.allclose(seq[:3], st, rtol=0, atol=1e-10) and np.allclose(seq[3:], sr, rtol=0, atol=1e-11)


def test_a_run_on_a_noise_free_scene_does_what_the_text_does():
    r = V.Rig(1, 300, perturb=1e-3)
    b = V.bearings_of(r.new_px)
    lm = np.hstack([b, r.points])

    def residual(p):
        x = r.points @ p[:, :3].T + p[:, 3]
        return float(np.mean(1.0 - np.sum(x / np.linalg.norm(x, axis=1, keepdims=True) * b, 1)))

    q, it = V.optimize(r.pose_in, RATE, 400, lm)
    g0, g1 = V.gradient_sum(r.pose_in, lm), V.gradient_sum(q, lm)
    assert it == 399
    assert np.linalg.norm(g1[:3]) < 0.1 * np.linalg.norm(g0[:3]) and np.linalg.norm(g1[3:]) < 0.1 * np.linalg.norm(g0[3:])
    assert residual(q) < 0.1 * residual(r.pose_in)
    (rot0, tr0), (rot1, tr1) = r.pose_error(r.pose_in), r.pose_error(q)
    assert rot1 < rot0
    assert tr1 > tr0          # the finding in the head of this file: the text trades the turn for a shift
    # no landmarks: the pose untouched
    p, it = V.optimize(r.pose_in, RATE, 400, np.zeros((0, 6)))
    assert it == 0 and np.array_equal(p, r.pose_in)
