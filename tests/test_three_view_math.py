"""include/akz_three_view_math.h, compiled for the host (tests/cpp/three_view_host.c through tests/three_view_checker.py),
against the independent numpy statement of tests/three_view_statement.py.  No GPU: the device's half of the parity
(host build == HIP, bit for bit) is tests/test_gpu_three_view.py.

Tolerances are 10 x the largest deviation measured on these very cases with gcc 13 / numpy's LAPACK on x86-64:
  per-landmark gradients        measured 8.4e-17   GRAD_TOL = 8.4e-16
  poses after an optimiser run  measured 1.4e-15   POSE_TOL = 1.4e-14
  poses after the procedure     measured 6.6e-15   FULL_TOL = 6.6e-14   (translations of a few units, nine eigh against Jacobi)
  exact data, 300 iterations    the poses move by 2.3e-16 at the most    STILL_TOL = 2.3e-15
"""
import numpy as np
import pytest

import three_view_checker as K
import three_view_statement as S

GRAD_TOL, POSE_TOL, FULL_TOL, STILL_TOL = 8.4e-16, 1.4e-14, 6.6e-14, 2.3e-15
MARGIN = 1e-9


def inverted(poses):
    return np.stack([S.invert(p) for p in poses])


# ---- 1. gradients ----
@pytest.mark.parametrize("noise", [0.0, 0.5])
def test_gradients_against_the_statement(noise):
    worst = 0.0
    for seed in range(6):
        rig = K.Rig(seed, 64, noise=noise, perturb=2e-3)
        inv = inverted(rig.pose_in)
        want = S.landmark_gradients(inv, rig.common[:, 0], rig.common[:, 1], rig.common[:, 2])
        got = np.stack([K.gradients(inv, c, f, s) for c, f, s in rig.common])
        assert np.all(np.isfinite(got))
        worst = max(worst, np.max(np.abs(got - want)))
    print(f"largest gradient deviation at noise {noise}: {worst:.3g}")
    assert worst <= GRAD_TOL


def degenerate_landmarks():
    """(inverted poses, c, f, s): a bearing parallel to a translation (its cross product with it is exactly zero, the
    normalisation divides 0 by 0) and two identical bearings (the two epipolar normals coincide, the triangulation's z is zero)."""
    rig = K.Rig(3, 8, perturb=2e-3)
    inv = inverted(rig.pose_in)
    inv[0] = np.hstack([np.eye(3), [[1.0], [0.0], [0.0]]])
    c, f, s = rig.common[0]
    return [(inv, np.array([1.0, 0.0, 0.0]), f, s), (inv, c, c.copy(), s)]


def test_degenerate_landmarks_give_zero_vectors_not_nan():
    cases = degenerate_landmarks()
    for inv, c, f, s in cases:
        g = K.gradients(inv, c, f, s)
        assert np.all(np.isfinite(g)), g
        want = S.landmark_gradients(inv, c, f, s)[0]
        assert np.max(np.abs(g - want)) <= GRAD_TOL
    # Se3TangentSpace::new works per VECTOR: the NaN of ftoc x c zeroes all of the first rotation gradient and nothing else
    g = K.gradients(*cases[0])
    assert np.all(g[3:6] == 0.0) and np.any(g[9:12] != 0.0)


# ---- 4. the translation-gradient fact ----
def test_translation_gradients_are_zero_on_a_well_posed_scene():
    """Scene "rig 11": 64 points 3 - 9 units in front of all three cameras, 0.5 px noise, poses 2 mrad off.
    three_view_gradients hands two_view_same_space_triangulate_sine_l1 the negated translations (epipolar.rs:118, 128,
    139); w = |z|^2 / z.(t x b) then is negative for every point in front of both cameras, from_homogeneous turns the
    bearing to -a and the cheirality filter drops the point.  All three translation gradients are exactly zero; the
    rotation gradients are not.  With the sign the function's own doc comment implies they would be live."""
    rig = K.Rig(11, 64, noise=0.5, perturb=2e-3)
    inv = inverted(rig.pose_in)
    g = np.stack([K.gradients(inv, c, f, s) for c, f, s in rig.common])
    assert np.all(g[:, 0:3] == 0.0) and np.all(g[:, 6:9] == 0.0)
    assert np.all(np.linalg.norm(g[:, 3:6], axis=1) > 0) and np.all(np.linalg.norm(g[:, 9:12], axis=1) > 0)
    # the same function with the translation itself triangulates every one of them in front of both cameras
    L = K.lib()
    for c, f, s in rig.common:
        fc = inv[0][:, :3] @ f
        t = np.ascontiguousarray(inv[0][:, 3])
        p = np.zeros(3)
        a, b = np.ascontiguousarray(c), np.ascontiguousarray(fc)
        assert L.tv_sine_l1(t.ctypes.data, a.ctypes.data, b.ctypes.data, p.ctypes.data) == 1 and 2.0 < p[2] < 10.0
        nt = np.ascontiguousarray(-t)
        assert L.tv_sine_l1(nt.ctypes.data, a.ctypes.data, b.ctypes.data, p.ctypes.data) == 0


# ---- 2. optimiser runs ----
@pytest.fixture(scope="module")
def runs():
    out = {}
    for n in (40, 256):
        rig = K.Rig(7, n, noise=0.5, perturb=2e-3)
        for it in (1, 50, 51, 300):
            out[n, it] = (rig, K.optimize(rig.pose_in, 0.001, it, rig.common), S.optimize(list(rig.pose_in), 0.001, it, rig.common))
    return out


@pytest.mark.parametrize("n", [40, 256])
@pytest.mark.parametrize("iterations", [1, 50, 51, 300])
def test_optimiser_runs_against_the_statement(runs, n, iterations):
    rig, (got, stop), (want, want_stop) = runs[n, iterations]
    dev = np.max(np.abs(got - np.stack(want)))
    print(f"n {n} iterations {iterations}: stop {stop}, deviation {dev:.3g}, moved {np.max(np.abs(got - rig.pose_in)):.3g}")
    assert stop == want_stop == iterations - 1, "a run that still improves leaves at its last iteration"
    assert dev <= POSE_TOL
    assert np.max(np.abs(got - rig.pose_in)) > 1e-7 * iterations, "the run moved the poses"


def exact_rig(n):
    rig = K.Rig(7, n)
    pts = rig.points[:n]
    unit = lambda v: v / np.linalg.norm(v, axis=1, keepdims=True)
    lm = np.stack([unit(pts), unit(pts @ rig.first[:, :3].T + rig.first[:, 3]), unit(pts @ rig.second[:, :3].T + rig.second[:, 3])], 1)
    return np.stack([rig.first, rig.second]), lm


@pytest.mark.parametrize("n", [40, 256])
def test_exact_data_stop_rule(n):
    """Exact bearings and exact poses.  The summed gradients are rounding noise of 1e-16, not exactly zero — but a step of
    0.001 / n times that does not change one bit of a pose, so every iteration sums the same numbers, the strict `best > norm`
    improves at iteration 0 only, and the host build leaves by the no-improvement rule at iteration 50 (not at 49, not at 299).
    The statement agrees, and the poses stay where they are."""
    poses, lm = exact_rig(n)
    got, stop = K.optimize(poses, 0.001, 300, lm)
    want, want_stop = S.optimize(list(poses), 0.001, 300, lm)
    print(f"n {n}: stop {stop} / {want_stop}, moved {np.max(np.abs(got - poses)):.3g}")
    assert stop == want_stop == 50
    assert np.max(np.abs(got - poses)) <= STILL_TOL
    assert np.max(np.abs(got - np.stack(want))) <= POSE_TOL


def test_no_improvement_rule_and_strict_comparison():
    """Gradients that are exactly zero from the first iteration on: landmarks whose three bearings coincide with a translation
    direction give NaN -> zero vectors, every norm is 0.0, `best > 0.0` improves once (from infinity) and `0.0 > 0.0`
    never again: 50 iterations later, at iteration 50, the run leaves with the poses untouched."""
    rig = K.Rig(5, 4)
    poses = np.stack([np.hstack([np.eye(3), [[1.0], [0.0], [0.0]]]), np.hstack([np.eye(3), [[2.0], [0.0], [0.0]]])])
    x = np.array([1.0, 0.0, 0.0])
    lm = np.stack([np.stack([x, x, x])] * 4)
    got, stop = K.optimize(poses, 0.001, 300, lm)
    assert stop == 50 and np.array_equal(got, poses)
    assert S.optimize(list(poses), 0.001, 300, lm)[1] == 50
    assert K.optimize(poses, 0.001, 50, lm)[1] == 49, "the last-iteration break comes first when iterations == 50"
    del rig


# ---- 5. summation order ----
@pytest.mark.parametrize("n", [40, 256, 1000])
def test_fixed_tree_against_sequential_sum(n):
    """What the fixed order of the sum over landmarks costs: the same text adding the gradients one after another."""
    rig = K.Rig(9, n, noise=0.5, perturb=2e-3)
    tree, stop_t = K.optimize(rig.pose_in, 0.001, 300, rig.common)
    seq, stop_s = K.optimize(rig.pose_in, 0.001, 300, rig.common, sequential=True)
    print(f"n {n}: tree against sequential {np.max(np.abs(tree - seq)):.3g}")
    assert stop_t == stop_s
    assert np.max(np.abs(tree - seq)) <= POSE_TOL


# ---- 3. the full procedure ----
QUICK = dict(three_view_patience=60, three_view_filter_loop_iterations=2)


def both(rig, **kw):
    st = K.settings(**kw)
    host = K.init_triple(rig.pose_in, rig.common, rig.first_only, rig.second_only, st)
    want = S.init_triple(rig.pose_in, list(rig.common), list(rig.first_only), list(rig.second_only), K.settings_dict(st))
    return host, want


def compare(host, want):
    assert host["verdict"] == want["verdict"]
    assert host["scales"] == want["scales"]
    st = host["stats"]
    if "median" in want:
        assert abs(host["median"] - want["median"]) <= 1e-12 * want["median"]
    if "pairs" in want:
        assert host["pairs"] == want["pairs"]
    runs = len(want["run_matches"])
    assert list(st[K.S_RUN_MATCHES:K.S_RUN_MATCHES + runs]) == want["run_matches"] and np.all(st[K.S_RUN_MATCHES + runs:K.S_RUN_STOP] == 0xFFFFFFFF)
    made = len(want["run_stop"])
    assert list(st[K.S_RUN_STOP:K.S_RUN_STOP + made]) == want["run_stop"] and np.all(st[K.S_RUN_STOP + made:K.S_ROBUST] == 0xFFFFFFFF)
    if "robust" in want:
        assert host["robust"] == want["robust"]
    if want["verdict"] == 0:
        for k in ("combined", "first_ok", "second_ok"):
            assert np.array_equal(host[k], np.array(want[k], np.uint8)), k
        assert np.max(np.abs(host["poses"] - np.stack(want["poses"]))) <= FULL_TOL
    else:
        assert np.all(np.isnan(host["poses"])) and np.all(host["combined"] == 255), "a rejected triple's poses and masks are left alone"


def test_full_procedure_against_the_statement():
    """Seeds 0 .. 11; a scene where some compared quantity lies within a relative 1e-9 of its threshold is dropped (the
    statement alone decides that), and at most 1 % of the scenes may be: with 12 scenes, none."""
    dropped = 0
    for seed in range(12):
        rig = K.Rig(seed, 120, noise=0.5, perturb=2e-3, n_first=15, n_second=17, outliers=10)
        host, want = both(rig, **QUICK)
        if S.closest_margin(want["near"]) < MARGIN:
            dropped += 1
            continue
        assert want["verdict"] == 0 and 0 < sum(want["combined"]) < 120
        compare(host, want)
    assert dropped <= 0.01 * 12


def verdict_scene(rig, expect, **kw):
    host, want = both(rig, **dict(QUICK, **kw))
    assert S.closest_margin(want["near"]) >= MARGIN
    assert want["verdict"] == S.VERDICTS[expect]
    compare(host, want)
    return host


def test_verdict_few_scales():
    host = verdict_scene(K.Rig(1, 15, noise=0.5, perturb=2e-3), "few_scales")
    assert host["scales"] == 15 and host["stats"][K.S_STAGE] == 1


def test_verdict_few_bearing_pairs():
    """Exactly two robust bearing pairs: the pair threshold is put between the second and the third largest of the pairs'
    smallest-over-the-views cosine distance."""
    rig = K.Rig(1, 40, noise=0.5, perturb=2e-3)
    d = np.min([1 - rig.common[:, k] @ rig.common[:, k].T for k in range(3)], axis=0)[np.triu_indices(40, 1)]
    d = np.sort(d)[::-1]
    host = verdict_scene(rig, "few_bearing_pairs", robust_view_bearing_pair_minimum_cosine_distance=float((d[1] + d[2]) / 2))
    assert host["pairs"] == 2 and host["stats"][K.S_STAGE] == 2
    verdict_scene(rig, "ok", robust_view_bearing_pair_minimum_cosine_distance=float((d[2] + d[3]) / 2))


def test_verdict_few_matches():
    host = verdict_scene(K.Rig(1, 31, noise=0.5, perturb=2e-3), "few_matches")
    assert host["stats"][K.S_RUN_MATCHES] == 31 and host["stats"][K.S_STAGE] == 3


def test_verdict_lost_half():
    """60 of 100 matches are 40 px off in the second view: the first filter's cosine distance of 1.0 lets them through, the
    filter after the first run (1e-5) does not, and 40 <= 100 / 2."""
    host = verdict_scene(K.Rig(1, 100, noise=0.5, perturb=2e-3, outliers=60), "lost_half")
    assert host["stats"][K.S_RUN_MATCHES] == 100 and host["stats"][K.S_RUN_MATCHES + 1] == 40 and host["stats"][K.S_STAGE] == 4


def test_verdict_few_robust():
    host = verdict_scene(K.Rig(1, 40, noise=0.5, perturb=2e-3, outliers=9), "few_robust", three_view_filter_loop_iterations=0)
    assert host["robust"] == 31 and host["stats"][K.S_STAGE] == 12


def test_take_ignores_what_lies_behind_the_last_landmark_taken():
    """take(n): with a cap of 33 landmarks every run takes 33, and the masks still cover all 80 matches."""
    rig = K.Rig(2, 80, noise=0.5, perturb=2e-3)
    st = K.settings(three_view_optimization_landmarks=33, **QUICK)
    a = K.init_triple(rig.pose_in, rig.common, rig.first_only, rig.second_only, st)
    assert a["verdict"] == 0 and list(a["stats"][K.S_RUN_MATCHES:K.S_RUN_MATCHES + 3]) == [33, 33, 33]
    assert len(a["combined"]) == 80 and a["combined"][40:].sum() > 0
