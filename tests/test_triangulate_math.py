"""include/akz_triangulate_math.h on the CPU (built by tests/triangulate_checker.py from tests/cpp/triangulate_host.c): the
reference's own pin, an independent solver (numpy / LAPACK), and the rules around the eigen-solve.  The GPU kernels are held
to this build bit for bit in tests/test_gpu_triangulate.py."""
import numpy as np

import triangulate_checker as tc


def bearing(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def euclid(p):
    return p[:3] / p[3]


def doc_test_pose():
    """cv-geom/src/triangulation.rs:31-32: CameraToCamera::from_parts((0.1, 0.1, 0.1), Rotation3::new((0.1, 0.1, 0.1)))."""
    return np.hstack([tc.rodrigues([0.1, 0.1, 0.1]), np.full((3, 1), 0.1)])


def test_reference_doc_test_pin_through_triangulate_relative():
    """cv-geom/src/triangulation.rs:26-38: the triangulated point lies within 1e-6 of (0.3, 0.1, 2.0)."""
    X = np.array([0.3, 0.1, 2.0])
    pose = doc_test_pose()
    a, b = bearing(X), bearing(pose[:, :3] @ X + pose[:, 3])
    ident = np.hstack([np.eye(3), np.zeros((3, 1))])
    p, why = tc.observations([ident, pose], [a, b])          # triangulate_relative = (identity, a), (pose, b)
    assert why == 0
    d = np.linalg.norm(euclid(p) - X)
    print("doc-test distance", d)
    assert d < 1e-6
    assert abs(np.linalg.norm(p[:3]) - 1.0) < 1e-15 and p[3] > 0          # Projective form


def test_reference_pin_with_2_3_8_32_exact_views():
    X = np.array([0.3, 0.1, 2.0])
    rng = np.random.default_rng(0xD0C)
    for n in (2, 3, 8, 32):
        poses = tc.random_poses(rng, n)
        poses[0] = np.hstack([np.eye(3), np.zeros((3, 1))])
        poses[1] = doc_test_pose()
        bs = [bearing(P[:, :3] @ X + P[:, 3]) for P in poses]
        p, why = tc.observations(poses, bs)
        assert why == 0, (n, why)
        d = np.linalg.norm(euclid(p) - X)
        print(n, "views: distance", d)
        assert d < 1e-6, (n, d)


def numpy_design_matrix(poses, bearings):
    A = np.zeros((4, 4))
    for P, b in zip(poses, bearings):
        term = P - np.outer(b, b) @ P
        A += term.T @ term
    return A


def test_against_lapack_on_noisy_scenes():
    """An independent solver: numpy eigh (LAPACK) on a design matrix built in numpy, signed-smallest eigenvalue.  2 000
    scenes: points 2-10 units deep, 2-32 views at least 0.1 apart, pixel noise up to 0.5 px at f = 1000.  A scene is compared
    only when LAPACK's (l2 - l1) >= 1e-6 * l4 (the two smallest eigenvalues are told apart); at most 5 % of the scenes may be
    filtered out.  Share this test itself excludes: 0 of 2 000 (0 %); smallest (l2 - l1) / l4 seen 1.7e-3; worst distance to
    LAPACK 4.1e-13 (relative).
    Tolerance: distance <= 1e-6 * max(1, |p|), the reference's doc-test tolerance."""
    rng = np.random.default_rng(0x7A1)
    f, n_scenes = 1000.0, 2000
    filtered, worst, min_gap = 0, 0.0, np.inf
    for s in range(n_scenes):
        n = int(rng.integers(2, 33))
        poses = tc.random_poses(rng, n)
        X = np.array([rng.uniform(-2, 2), rng.uniform(-1.5, 1.5), rng.uniform(2, 10)])
        bs = []
        for P in poses:
            x, y = tc.project(P, X, f, 0.0, 0.0)
            bs.append(bearing([(x + rng.uniform(-0.5, 0.5)) / f, (y + rng.uniform(-0.5, 0.5)) / f, 1.0]))
        lam, vec = np.linalg.eigh(numpy_design_matrix(poses, bs))
        gap = (lam[1] - lam[0]) / lam[3]
        min_gap = min(min_gap, gap)
        if gap < 1e-6:
            filtered += 1
            continue
        want = vec[:, 0] / vec[3, 0]
        p, why = tc.observations(poses, bs)
        assert why in (0, 5), (s, why)
        if why == 5:                               # behind a camera by LAPACK's point too, or the scene fails
            assert any((P[:, :3].T @ b) @ want[:3] < 0 for P, b in zip(poses, bs)), s
            continue
        d = np.linalg.norm(euclid(p) - want[:3])
        worst = max(worst, d / max(1.0, np.linalg.norm(want[:3])))
        assert d <= 1e-6 * max(1.0, np.linalg.norm(want[:3])), (s, n, d)
    print(f"filtered {filtered} of {n_scenes}; smallest (l2 - l1) / l4 {min_gap:.3g}; worst relative distance to LAPACK {worst:.3g}")
    assert filtered <= 0.05 * n_scenes


def two_view_case():
    X = np.array([0.2, -0.1, 4.0])
    ident = np.hstack([np.eye(3), np.zeros((3, 1))])
    P1 = np.hstack([np.eye(3), np.array([[-0.5], [0.0], [0.0]])])
    P2 = np.hstack([np.eye(3), np.array([[0.0], [-0.5], [0.0]])])
    poses = [ident, P1, P2]
    return X, poses, [bearing(P[:, :3] @ X + P[:, 3]) for P in poses]


def test_reason_1_too_few_observations():
    X, poses, bs = two_view_case()
    for robust in (False, True):
        p, why = tc.observations(poses[:1], bs[:1], robust=robust)
        assert why == 1 and p.tobytes() == tc.NONE.tobytes()
        p, why = tc.observations(poses[:0], bs[:0], robust=robust)
        assert why == 1 and p.tobytes() == tc.NONE.tobytes()


def test_reason_2_parallel_bearings_and_the_minimum_observation_count():
    X, poses, bs = two_view_case()
    # three observations, good parallax: robust
    p, why = tc.observations(poses, bs, robust=True)
    assert why == 0 and np.linalg.norm(euclid(p) - X) < 1e-9
    # two observations are too few for robust_minimum_observations = 3 ...
    p, why = tc.observations(poses[:2], bs[:2], robust=True)
    assert why == 2 and p.tobytes() == tc.NONE.tobytes()
    # ... unless the reconstruction has only two views: min(3, 2) = 2 (cv-sfm/src/lib.rs:2913-2917)
    p, why = tc.observations(poses[:2], bs[:2], robust=True, st=tc.settings(n_views=2))
    assert why == 0 and np.linalg.norm(euclid(p) - X) < 1e-9
    # the same without the robustness test
    assert tc.observations(poses[:2], bs[:2], robust=False)[1] == 0
    # parallel bearings: a point so far away that no pair has 1 - cos > 1e-3
    far = np.array([0.0, 0.0, 1e4])
    bf = [bearing(P[:, :3] @ far + P[:, 3]) for P in poses]
    p, why = tc.observations(poses, bf, robust=True)
    assert why == 2 and p.tobytes() == tc.NONE.tobytes()
    # only the pair (1, 2) has enough parallax, no pair with observation 0 does: camera 0 sits between cameras 1 and 2,
    # and the search over the pairs that the accumulation pass did not see finds it
    X2 = np.array([0.0, 0.0, 3.0])
    lst = [np.hstack([np.eye(3), -np.array(c, np.float64).reshape(3, 1)]) for c in ([0.0, 0, 0], [-0.3, 0, 0], [0.3, 0, 0])]
    bl = [bearing(P[:, :3] @ X2 + P[:, 3]) for P in lst]
    d01, d02, d12 = 1 - bl[0] @ bl[1], 1 - bl[0] @ bl[2], 1 - bl[1] @ bl[2]
    assert max(d01, d02) < 0.5 * d12
    only12 = tc.settings(min_cos=float(0.75 * d12))
    assert tc.observations(lst, bl, robust=True, st=only12)[1] == 0
    assert tc.observations(lst, bl, robust=True, st=tc.settings(min_cos=float(1.25 * d12)))[1] == 2


def test_reason_4_nan_pose():
    X, poses, bs = two_view_case()
    bad = [P.copy() for P in poses]
    bad[1][0, 3] = np.nan
    for robust in (False, True):
        p, why = tc.observations(bad, bs, robust=robust)
        assert why == 4 and p.tobytes() == tc.NONE.tobytes()
    bad[1][0, 3] = np.inf
    assert tc.observations(bad, bs)[1] == 4


def test_reason_5_point_behind_a_camera():
    X, poses, bs = two_view_case()
    flipped = list(bs)
    flipped[1] = -bs[1]                 # the same line of sight, seen "backwards": the design matrix is the same
    p, why = tc.observations(poses, flipped)
    assert why == 5 and p.tobytes() == tc.NONE.tobytes()
    p, why = tc.observations(poses, bs)
    assert why == 0


def test_reason_3_needs_a_sweep_limit():
    """With finite input the cyclic Jacobi iteration converges in a handful of sweeps: reason 3 cannot be reached at the
    reference's max_iterations = 1000.  It is reached — not faked — by a sweep limit too small for the matrix: one sweep
    does not diagonalise a full 4 x 4 matrix to 1e-12."""
    X, poses, bs = two_view_case()
    p, why = tc.observations(poses, bs, st=tc.settings(max_sweeps=1))
    assert why == 3 and p.tobytes() == tc.NONE.tobytes()
    assert tc.observations(poses, bs, st=tc.settings(max_sweeps=30))[1] == 0


def test_negative_zero_in_w_is_negated():
    """Projective::from_homogeneous (cv-core/src/point.rs:20-25): is_sign_negative is the sign BIT, so a vector whose w is
    -0.0 is negated as a whole and leaves with w = +0.0, while w = +0.0 leaves it alone.  The eigen-solve itself cannot
    produce the case with finite input — V starts as the identity, whose zeros are +0, and c * 0 - s * 0 / s * 0 + c * 0 give
    +0 for either sign of s — so the rule is held on the step itself (akz_tri_from_homogeneous), which akz_tri_solve calls."""
    x = np.array([3.0, -4.0, 12.0])                                    # |xyz| = 13
    neg = tc.from_homogeneous([x[0], x[1], x[2], -0.0])
    assert neg[:3].tolist() == (-x / 13.0).tolist() and neg[3] == 0.0 and not np.signbit(neg[3])
    pos = tc.from_homogeneous([x[0], x[1], x[2], 0.0])
    assert pos[:3].tolist() == (x / 13.0).tolist() and pos[3] == 0.0 and not np.signbit(pos[3])
    # ordinary signs of w: negative flips everything, positive nothing; all four are divided by |xyz|
    assert tc.from_homogeneous([3.0, -4.0, 12.0, -26.0]).tolist() == [-3.0 / 13, 4.0 / 13, -12.0 / 13, 2.0]
    assert tc.from_homogeneous([3.0, -4.0, 12.0, 26.0]).tolist() == [3.0 / 13, -4.0 / 13, 12.0 / 13, 2.0]
    # zeros in xyz keep / change their sign bit with the rest
    z = tc.from_homogeneous([0.0, 0.0, 2.0, -0.0])
    assert np.signbit(z[0]) and np.signbit(z[1]) and z[2] == -1.0 and not np.signbit(z[3])
    # through the solve: a diagonal matrix needs no rotation, the eigenvectors are the unit vectors, w = +0 stays +0 ...
    p, why = tc.solve(np.diag([1e-9, 1.0, 2.0, 3.0]))
    assert why == 0 and p.tolist() == [1.0, 0.0, 0.0, 0.0] and not np.signbit(p[3])
    # ... and a null vector (1, 0, 0, -1e-3) comes out with w > 0, x < 0
    v = np.array([1.0, 0.0, 0.0, -1e-3]); v /= np.linalg.norm(v)
    p, why = tc.solve(np.eye(4) - np.outer(v, v))
    assert why == 0 and p[3] > 0 and p[0] < 0
    # the FloatOrd key (another function) on the two zeros and around them
    key = tc.lib().tri_float_ord
    assert key(-0.0) < key(0.0) and key(-1e-300) < key(-0.0) and key(0.0) < key(1e-300)
    assert key(-np.inf) < key(-1.0) < key(1.0) < key(np.inf)


def test_float_ord_selection_on_a_tiny_negative_eigenvalue():
    """The eigenvector is chosen by FloatOrd, the signed total order (cv-geom/src/triangulation.rs:111-115) — not by the
    abs().to_bits() key of cv-core/src/pose.rs:282: on eigenvalues (-1e-17, +1e-18, 1, 2) the signed order takes the first
    column, the absolute-value key would take the second."""
    A = np.diag([-1e-17, 1e-18, 1.0, 2.0])
    p, why = tc.solve(A)
    assert why == 0 and p.tolist() == [1.0, 0.0, 0.0, 0.0]
    lam = np.diag(A)
    assert int(np.argmin(np.abs(lam))) == 1 and int(np.argmin(lam)) == 0
    # equal keys: the first wins (Iterator::min_by_key)
    p, why = tc.solve(np.diag([1.0, 0.5, 0.5, 2.0]))
    assert why == 0 and p.tolist() == [0.0, 1.0, 0.0, 0.0]


def test_merged_list_is_first_landmark_then_second_and_robustness_sees_both():
    """triangulate_merged_landmark_robust (cv-sfm/src/lib.rs:2958-2972): the observations of landmark best0 followed by those
    of best1; neither half alone is robust (one observation each), the concatenation is."""
    rng = np.random.default_rng(3)
    cam = tc.camera(1000.0, 1000.0, 960.0, 540.0)
    kps, poses, start, obs, pts = tc.synthetic_map(rng, 8, 64, 4, noise=0.0, max_len=0)
    # landmarks 0 and 1 are the same point seen from blocks 0, 1 and 2, 3; landmark 2 = blocks 4, 5, 6
    X = np.array([0.3, -0.2, 5.0])
    lists = [[(0, 0), (1, 0)], [(2, 0), (3, 0)], [(4, 0), (5, 0), (6, 0)], []]
    for l in lists:
        for b, j in l:
            kps[b, j]["x"], kps[b, j]["y"] = tc.project(poses[b].reshape(3, 4), X, 1000.0, 960.0, 540.0)
    start = np.cumsum([0] + [len(l) for l in lists]).astype(np.uint32)
    obs = np.array([o for l in lists for o in l], np.uint32)
    world, reason = tc.landmarks(kps, poses, cam, start, obs)
    assert reason.tolist() == [2, 2, 0, 1]                               # two observations each: below the minimum of 3
    best = np.full((1, 64, 3, 2), 0xFFFFFFFF, np.uint32)
    dec = np.zeros((1, 64), np.uint32); ok = np.zeros((1, 64), np.uint8)
    best[0, 5, 0, 0], best[0, 5, 1, 0] = 0, 1; dec[0, 5] = 2; ok[0, 5] = 1     # admitted
    best[0, 6, 0, 0], best[0, 6, 1, 0] = 1, 0; dec[0, 6] = 2; ok[0, 6] = 1     # the other order
    best[0, 7, 0, 0], best[0, 7, 1, 0] = 0, 1; dec[0, 7] = 2; ok[0, 7] = 0     # not admitted
    best[0, 8, 0, 0], best[0, 8, 1, 0] = 0, 1; dec[0, 8] = 1; ok[0, 8] = 1     # not a merge candidate
    best[0, 9, 0, 0], best[0, 9, 1, 0] = 0, 77; dec[0, 9] = 2; ok[0, 9] = 1    # a landmark that does not exist
    table = np.full((4 + 64, 4), 7.25)
    r = tc.merged(kps, poses, cam, start, obs, best, dec, ok, 4, table)
    assert r[0, 5] == 0 and r[0, 6] == 0 and r[0, 9] == 6 and (np.delete(r[0], [5, 6, 9]) == 255).all()
    # (keypoints are f32: 6e-5 px at x ~ 1000, times depth^2 / (baseline * f) = 25 / (0.5 * 1000) -> a few 1e-6 of depth)
    assert np.linalg.norm(euclid(table[4 + 5]) - X) < 2e-5
    untouched = np.delete(np.arange(68), [4 + 5, 4 + 6, 4 + 9])
    assert (table[untouched] == 7.25).all() and table[4 + 9].tobytes() == tc.NONE.tobytes()
    # the order of the list is the order of the sum: rows 5 and 6 hold the same observations in different order
    P = poses.reshape(-1, 3, 4)
    bl = []
    for b, j in lists[0] + lists[1]:
        o = np.empty(3)
        tc.lib().tri_calibrate(cam, kps[b, j]["x"], kps[b, j]["y"], o.ctypes.data)
        bl.append(o)
    p01, _ = tc.observations(P[[0, 1, 2, 3]], bl, robust=True)
    p10, _ = tc.observations(P[[2, 3, 0, 1]], bl[2:] + bl[:2], robust=True)
    assert table[4 + 5].tobytes() == p01.tobytes() and table[4 + 6].tobytes() == p10.tobytes()


def test_bad_indices_give_reason_6_and_read_nothing():
    rng = np.random.default_rng(4)
    cam = tc.camera(1000.0, 1000.0, 960.0, 540.0)
    kps, poses, start, obs, pts = tc.synthetic_map(rng, 6, 32, 12, max_len=6)
    obs = obs.copy()
    l = int(np.argmax(np.diff(start.astype(np.int64)) >= 3))
    good, _ = tc.landmarks(kps, poses, cam, start, obs)
    obs[start[l] + 1, 0] = 6                                             # block == n_blocks
    world, reason = tc.landmarks(kps, poses, cam, start, obs)
    assert reason[l] == 6 and world[l].tobytes() == tc.NONE.tobytes()
    keep = np.arange(12) != l
    assert world[keep].tobytes() == good[keep].tobytes()
    obs[start[l] + 1] = (0, 32)                                          # feature == cap
    assert tc.landmarks(kps, poses, cam, start, obs)[1][l] == 6
    # a list that runs past the observation array
    world, reason = tc.landmarks(kps, poses, cam, start, obs, n_obs=int(start[-1]) - 1)
    assert reason[11] == 6 or start[11] == start[12]
