"""include/akz_three_view_constraint_math.h, built for the host (tests/three_view_constraint_checker.py), against the
independent numpy statement of tests/three_view_constraint_statement.py.  No GPU.

Measured on the scenes below (host build in the header's one-wave order against the statement's sequential sums): the worst
deviation of a pose entry is 1.59e-14 (64 landmarks, patience 4096; 1.0e-15 at patience <= 64), of a scale 7.8e-15.  Asserted
at ten times that.  The one-wave order against the reference's sequential order inside the host build itself: at most
1.2e-16 on a pose entry over the same scenes — the price of the order a wavefront needs."""
import numpy as np
import pytest

import three_view_constraint_checker as T
import three_view_constraint_statement as S
from three_view_statement import invert

MEASURED_POSE, MEASURED_SCALE, MEASURED_ORDER = 1.6e-14, 7.8e-15, 1.2e-16
POSE_TOL, SCALE_TOL, ORDER_TOL = 10 * MEASURED_POSE, 10 * MEASURED_SCALE, 10 * MEASURED_ORDER

# (seed, landmarks, patience); the cap is 256 so that every landmark is used
SCENES = [(1, 24, 1), (2, 24, 2), (3, 64, 64), (4, 65, 64), (5, 100, 2), (6, 256, 64), (7, 128, 1), (8, 64, 4096), (9, 200, 64), (10, 31, 64)]


@pytest.fixture(scope="module")
def scenes():
    return {seed: T.scene(seed, n) for seed, n, _ in SCENES}


def test_generator_yields_every_requested_scene(scenes):
    assert len(scenes) == len(SCENES)
    for seed, n, _ in SCENES:
        sc = scenes[seed]
        assert sc.n == n and sc.landmarks.shape == (n, 3, 3) and sc.closest_pair(256) > T.PAIR_MARGIN
        assert np.allclose(np.linalg.norm(sc.landmarks, axis=2), 1.0, atol=1e-15)


@pytest.mark.parametrize("seed,n,patience", SCENES)
def test_host_build_against_the_statement(scenes, seed, n, patience):
    sc = scenes[seed]
    ref = S.constraint(sc.world, sc.landmarks, dict(constraint_patience=patience, optimization_maximum_landmarks=256))
    got = T.constraint(sc.world, sc.landmarks, T.settings(constraint_patience=patience, optimization_maximum_landmarks=256))
    assert got["verdict"] == ref["verdict"] == T.OK
    assert (got["landmarks"], got["used"], got["pairs"]) == (ref["landmarks"], ref["used"], ref["pairs"]) == (n, n, ref["pairs"])
    assert ref["pairs"] >= 100 and ref["closest"] > T.PAIR_MARGIN
    assert got["stats"][T.S_STAGE] == 3
    dev = max(float(np.max(np.abs(got["poses"][k] - ref["poses"][k]))) for k in range(2))
    ds = max(abs(got["original_scale"] - ref["original_scale"]), abs(got["final_scale"] - ref["final_scale"]))
    print(f"seed {seed} n {n} patience {patience}: pose {dev:.3g} scale {ds:.3g}")
    assert dev <= POSE_TOL and ds <= SCALE_TOL
    # the optimiser moved the poses, and the result is back at the original scale
    rel = T.relative_poses(sc.world)
    assert not np.array_equal(rel, got["poses"])
    assert abs(S.scale_of(*got["poses"]) - got["original_scale"]) <= 8 * np.finfo(float).eps * got["original_scale"]


def test_pose_product_and_relative_poses(scenes):
    """Entries are sums of at most four products; each rounding is half an ulp of a partial sum no larger than the sum of
    the products' magnitudes, so 8 ulps of that sum bound both sides' difference."""
    sc = scenes[3]
    a, b = sc.world[1], sc.world[2]
    bound = 8 * np.finfo(float).eps * (np.abs(S.mat4(a)) @ np.abs(S.mat4(b)))[:3]
    assert np.all(np.abs(T.pose_mul(a, b) - S.compose(a, b)) <= bound)
    ref = [S.compose(sc.world[k], S.inverse(sc.world[0])) for k in (1, 2)]
    assert np.max(np.abs(T.relative_poses(sc.world) - np.stack(ref))) <= 64 * np.finfo(float).eps * 4.0


def test_empty_list_returns_the_poses_unchanged(scenes):
    rel = T.relative_poses(scenes[1].world)
    out = T.adaptive_optimize(rel, 5, np.zeros((0, 3, 3)))
    assert out.tobytes() == rel.tobytes()
    ref = S.adaptive_optimize(list(rel), 5, np.zeros((0, 3, 3)))
    assert np.array_equal(np.stack(ref), rel)
    # zero iterations: the poses go through two inversions only
    lm = scenes[1].landmarks
    assert np.max(np.abs(T.adaptive_optimize(rel, 0, lm) - rel)) <= 16 * np.finfo(float).eps * 4.0


def test_minimum_counts_the_whole_list_and_the_optimiser_the_first_maximum(scenes):
    sc = scenes[10]   # 31 landmarks
    full = T.constraint(sc.world, sc.landmarks[:30], T.settings(constraint_patience=8, optimization_maximum_landmarks=10))
    head = T.constraint(sc.world, sc.landmarks[:10], T.settings(constraint_patience=8, optimization_maximum_landmarks=10, optimization_minimum_landmarks=10))
    assert full["verdict"] == head["verdict"] == T.OK and (full["landmarks"], full["used"]) == (30, 10) and head["landmarks"] == 10
    assert full["poses"].tobytes() == head["poses"].tobytes() and full["pairs"] == head["pairs"]
    ref = S.constraint(sc.world, sc.landmarks[:30], dict(constraint_patience=8, optimization_maximum_landmarks=10))
    assert ref["verdict"] == 0 and ref["used"] == 10 and ref["pairs"] == full["pairs"]
    assert max(float(np.max(np.abs(full["poses"][k] - ref["poses"][k]))) for k in range(2)) <= POSE_TOL
    # 23 of a list of 23 is too few whatever the cap; the head of a list of 30 is not
    for cap in (10, 64):
        few = T.constraint(sc.world, sc.landmarks[:23], T.settings(constraint_patience=8, optimization_maximum_landmarks=cap))
        assert few["verdict"] == T.FEW_LANDMARKS == S.constraint(sc.world, sc.landmarks[:23], dict(optimization_maximum_landmarks=cap))["verdict"]
        assert list(few["stats"]) == [23, 0, 0, 0, 0, 0, 0, 1] and np.all(np.isnan(few["poses"]))
    assert T.constraint(sc.world, sc.landmarks[:24], T.settings(constraint_patience=1))["verdict"] == T.OK


def test_few_bearing_pairs(scenes):
    tight = T.scene(77, 40, spread=0.05)
    ref = S.constraint(tight.world, tight.landmarks, dict(constraint_patience=4))
    got = T.constraint(tight.world, tight.landmarks, T.settings(constraint_patience=4))
    assert ref["verdict"] == got["verdict"] == T.FEW_BEARING_PAIRS and ref["pairs"] == got["pairs"] < 3
    assert got["stats"][T.S_STAGE] == 2 and got["used"] == 40 and got["final_scale"] == 0.0
    assert abs(got["original_scale"] - ref["original_scale"]) <= SCALE_TOL
    # the same list passes when no pair is asked for
    assert T.constraint(tight.world, tight.landmarks, T.settings(constraint_patience=4, robust_view_num_robust_bearing_pair=0))["verdict"] == T.OK


def test_a_rate_that_is_not_finite_becomes_zero():
    inf, nan = float("inf"), float("nan")
    assert T.rate(0.0, 0.0) == 0.0 and T.rate(1.0, 0.0) == 0.0 and T.rate(nan, 1.0) == 0.0 and T.rate(1.0, nan) == 0.0
    assert T.rate(inf, 1.0) == 0.0 and T.rate(inf, inf) == 0.0 and T.rate(1.0, inf) == 0.0
    assert T.rate(1.0, 2.0) == 0.5 and T.rate(3.0, 3.0) == 1.0
    # all sums zero: both rates 0 / 0, the poses stay
    inv = np.stack([invert(p) for p in T.relative_poses(T.scene(1, 24).world)])
    assert np.array_equal(T.adaptive_step(np.zeros(16), 1.0 / 24, inv), inv)
    # the statement says the same
    assert S.rates(np.zeros(12), np.zeros(4), 1.0 / 24)[1] == [0.0] * 4
    assert S.rates(np.ones(12), np.zeros(4), 1.0)[1] == [0.0] * 4


def test_translation_rate_is_zero_on_a_well_posed_scene(scenes):
    """three_view_gradients passes negated translations: every translation gradient is exactly zero, the
    translation's rate is 0 / 0 and becomes 0; only the rotations move."""
    sc = scenes[3]
    trace = []
    ref = S.constraint(sc.world, sc.landmarks, dict(constraint_patience=16), trace)
    assert ref["verdict"] == 0 and len(trace) == 16
    assert all(r[0] == 0.0 and r[2] == 0.0 and 0.0 < r[1] <= 1.0 and 0.0 < r[3] <= 1.0 for r in trace)
    inv = np.stack([invert(p) for p in T.relative_poses(sc.world)])
    for seq in (False, True):
        nets = T.sums(inv, sc.landmarks, sequential=seq)
        assert np.all(nets[[0, 1, 2, 6, 7, 8, 12, 14]] == 0.0) and np.all(nets[[13, 15]] > 0.0)


def test_one_wave_order_against_the_sequential_order(scenes):
    worst, differ = 0.0, False
    for seed, n, patience in SCENES:
        sc = scenes[seed]
        st = T.settings(constraint_patience=patience, optimization_maximum_landmarks=256)
        a, b = T.constraint(sc.world, sc.landmarks, st), T.constraint(sc.world, sc.landmarks, st, sequential=True)
        assert (a["verdict"], a["pairs"], a["used"]) == (b["verdict"], b["pairs"], b["used"])
        worst = max(worst, float(np.max(np.abs(a["poses"] - b["poses"]))))
        inv = np.stack([invert(p) for p in T.relative_poses(sc.world)])
        differ |= T.sums(inv, sc.landmarks).tobytes() != T.sums(inv, sc.landmarks, sequential=True).tobytes()
    print(f"one-wave order against sequential order: {worst:.3g}")
    assert worst <= ORDER_TOL
    assert differ     # the two orders are not the same arithmetic: some sum differs in its last bits
    # up to 64 landmarks a lane holds one landmark, beyond that it adds its own in ascending order first
    sc = scenes[6]
    inv = np.stack([invert(p) for p in T.relative_poses(sc.world)])
    lanes = np.zeros((64, 16))
    for l in range(64):
        for i in range(l, 256, 64):
            lanes[l] = lanes[l] + T.sums(inv, sc.landmarks[i:i + 1], sequential=True)
    for m in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[np.arange(64) ^ m]
    assert lanes[0].tobytes() == T.sums(inv, sc.landmarks).tobytes() and np.all(lanes == lanes[0])
