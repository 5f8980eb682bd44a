"""An independent float64 statement of what cv-sfm's register_frame_subset does behind its consensus (cv-sfm/src/lib.rs:
1625-1775), in numpy, written from the Rust text: the homogeneous transform, normalisation and division of landmark_delta in
every iteration, sequential sums over the matches, numpy.linalg.eigh for the triangulations, np.sin / np.cos in nalgebra's
Rodrigues formula.  It shares no text with include/akz_single_view_math.h; tests/test_single_view_math.py holds the header's
host build to it.

Poses are WorldToCamera 3 x 4 arrays [R | t]; bearings are unit 3-vectors; world points homogeneous 4-vectors (w < 0: None).
"""
import numpy as np

OK, NO_MODEL, FEW_LANDMARKS, LOST_HALF, FEW_ROBUST, BAD_INDEX = range(6)


def from_homogeneous(p):
    """Projective::from_homogeneous (cv-core/src/point.rs:20-25)"""
    p = np.array(p, np.float64)
    if np.signbit(p[3]):
        p = -p
    with np.errstate(all="ignore"):
        return p / np.linalg.norm(p[:3])


def transform(pose, point):
    """Pose::transform (cv-core/src/pose.rs:125-133)"""
    return from_homogeneous(np.append(pose[:, :3] @ point[:3] + pose[:, 3] * point[3], point[3]))


def clean(v):
    """Se3TangentSpace::new (cv-core/src/so3.rs:23-34)"""
    return np.zeros(3) if np.any(np.isnan(v)) else v


def world_pose_gradient(t, b):
    """cv-geom/src/epipolar.rs:188-193 -> (translation, rotation)"""
    with np.errstate(all="ignore"):
        return clean((t @ b) * b - t), clean(np.cross(t / np.linalg.norm(t), b))


def landmark_delta(pose, bearing, world_point):
    """cv-optimize/src/single_view_optimizer.rs:4-14 -> (translation, rotation) or None"""
    c = transform(pose, world_point)
    if c[3] == 0.0:                      # Point3::from_homogeneous
        return None
    with np.errstate(all="ignore"):
        return world_pose_gradient(c[:3] / c[3], bearing)


def from_scaled_axis(w):
    """Rotation3::from_scaled_axis (nalgebra): Rodrigues in from_axis_angle's arrangement"""
    theta = np.linalg.norm(w)
    if not theta > 0:
        return np.eye(3)
    ux, uy, uz = w / theta
    s, c = np.sin(theta), np.cos(theta)
    o = 1.0 - c
    return np.array([[ux * ux * o + c, ux * uy * o - uz * s, ux * uz * o + uy * s],
                     [ux * uy * o + uz * s, uy * uy * o + c, uy * uz * o - ux * s],
                     [ux * uz * o - uy * s, uy * uz * o + ux * s, uz * uz * o + c]])


def apply_delta(translation, rotation, pose):
    """delta.isometry() * pose (so3.rs:57-60)"""
    r = from_scaled_axis(rotation)
    return np.hstack([r @ pose[:, :3], (r @ translation + r @ pose[:, 3])[:, None]])


def gradient_sum(pose, landmarks):
    """the reference's sum: the matches one after another (numpy.cumsum adds in order); landmarks = [(bearing, world point)].
    landmark_delta for all matches at once — the same operations as the function above, one row per match."""
    if len(landmarks) == 0:
        return np.zeros(3), np.zeros(3)
    b = np.array([l[0] for l in landmarks], np.float64)
    p = np.array([l[1] for l in landmarks], np.float64)
    with np.errstate(all="ignore"):
        c = np.hstack([p[:, :3] @ pose[:, :3].T + pose[:, 3] * p[:, 3:4], p[:, 3:4]])
        c = np.where(np.signbit(c[:, 3:4]), -c, c)
        c = c / np.linalg.norm(c[:, :3], axis=1, keepdims=True)
        none = c[:, 3] == 0.0
        t = c[:, :3] / c[:, 3:4]
        tg = np.sum(t * b, 1, keepdims=True) * b - t
        rg = np.cross(t / np.linalg.norm(t, axis=1, keepdims=True), b)
    tg[np.isnan(tg).any(1) | none] = 0.0
    rg[np.isnan(rg).any(1) | none] = 0.0
    return np.cumsum(tg, 0)[-1], np.cumsum(rg, 0)[-1]


def optimize(pose, rate, iterations, landmarks):
    """single_view_simple_optimize_l2 (single_view_optimizer.rs:80-135) -> (pose, the iteration the loop was left at, why:
    "none" / "stabilized" / "last" / "exhausted")"""
    pose = np.array(pose, np.float64).reshape(3, 4)
    if len(landmarks) == 0:
        return pose, 0, "none"
    best_t = best_r = np.inf
    no_improve_for = 0
    inv_len = 1.0 / len(landmarks)
    iteration, why = 0, "exhausted"
    while iteration < iterations:
        st, sr = gradient_sum(pose, landmarks)
        no_improve_for += 1
        t, r = np.linalg.norm(st), np.linalg.norm(sr)
        if best_t > t:
            best_t, no_improve_for = t, 0
        if best_r > r:
            best_r, no_improve_for = r, 0
        if no_improve_for >= 50:
            why = "stabilized"
            break
        pose = apply_delta(st * inv_len * rate, sr * inv_len * rate, pose)
        if iteration == iterations - 1:
            why = "last"
            break
        iteration += 1
    return pose, iteration, why


def triangulate(observations):
    """LinearEigenTriangulator::triangulate_observations (cv-geom/src/triangulation.rs:82-130)"""
    if len(observations) < 2:
        return None
    a = np.zeros((4, 4))
    for pose, b in observations:
        term = pose - np.outer(b, b) @ pose
        a += term.T @ term
    if not np.all(np.isfinite(a)):
        return None
    _, v = np.linalg.eigh(a)
    p = from_homogeneous(v[:, 0])
    if not np.all(np.isfinite(p)):
        return None
    for pose, b in observations:
        if np.signbit((pose[:, :3].T @ b) @ p[:3]):
            return None
    return p


def loss(t, a, b):
    """cv-geom/src/epipolar.rs:197-233"""
    ca, cb = np.cross(a, t), np.cross(b, t)
    with np.errstate(all="ignore"):
        r = abs(a @ (cb / np.linalg.norm(cb))) if ca @ ca < cb @ cb else abs(b @ (ca / np.linalg.norm(ca)))
    return 1.0 if (np.isnan(r) or np.signbit(a @ b)) else r


def invert(pose):
    r, t = pose[:, :3], pose[:, 3]
    return np.hstack([r.T, (-r.T @ t)[:, None]])


def compose(a, b):
    return np.hstack([a[:, :3] @ b[:, :3], (a[:, :3] @ b[:, 3] + a[:, 3])[:, None]])


def is_observation_consistent(pose, bearing, others, st, near=None):
    """cv-sfm/src/lib.rs:2622-2655; others = [(pose, bearing)].  `near` collects (value, threshold) of every comparison made."""
    if len(others) == 0:
        return False                       # "unreachable" in the reference
    if len(others) == 1:
        total = compose(others[0][0], invert(pose))
        v = loss(total[:, 3], total[:, :3] @ bearing, others[0][1])
        if near is not None:
            near.append((v, st["maximum_sine_distance"]))
        return bool(v < st["maximum_sine_distance"])
    everyone = list(others) + [(pose, bearing)]
    p = triangulate(everyone)
    if p is None:
        return False
    ok = True
    for q, b in everyone:
        v = 1.0 - transform(q, p)[:3] @ b
        if near is not None:
            near.append((v, st["maximum_cosine_distance"]))
        ok = ok and bool(v < st["maximum_cosine_distance"])
    return ok


def settings(**kw):
    st = dict(maximum_cosine_distance=1e-5, maximum_sine_distance=1e-1, single_view_optimization_rate=1e-3,
              single_view_optimization_num_matches=2048, single_view_filter_loop_iterations=5, single_view_patience=100000,
              single_view_minimum_landmarks=32, single_view_minimum_robust_landmarks=64)
    assert all(k in st for k in kw)
    st.update(kw)
    return st


def refine(bearing, world, others, pose_in, inliers, st, has_model=True, near=None):
    """register_frame_subset from its consensus on (lib.rs:1606-1775).  bearing [n][3], world [n][4] (w < 0: None), others[i] =
    the other observations [(pose, bearing)] of original match i; `inliers` index the matches with a world point.
    -> dict(verdict, pose, final [n] bool or None, robust, runs = [(matches entering, stopping iteration, why)], selected =
    the indices each re-selection took)"""
    n = len(bearing)
    some = [i for i in range(n) if world[i][3] >= 0.0]
    out = dict(verdict=OK, pose=None, final=None, robust=0, runs=[], selected=[])
    if len(some) < st["single_view_minimum_landmarks"]:
        return dict(out, verdict=FEW_LANDMARKS)
    if not has_model:
        return dict(out, verdict=NO_MODEL, pose=np.array(pose_in, np.float64).reshape(3, 4))
    num = st["single_view_optimization_num_matches"]
    chosen = [some[k] for k in list(inliers)[:num]]
    pose = np.array(pose_in, np.float64).reshape(3, 4)
    robust_minimum_matches = len(chosen) // 2
    consistent = lambda i: is_observation_consistent(pose, bearing[i], others[i], st, near)
    for run in range(st["single_view_filter_loop_iterations"] + 1):
        if len(chosen) <= robust_minimum_matches:
            out["runs"].append((len(chosen), None, None))
            return dict(out, verdict=LOST_HALF)
        pose, it, why = optimize(pose, st["single_view_optimization_rate"], st["single_view_patience"], [(bearing[i], world[i]) for i in chosen])
        out["runs"].append((len(chosen), it, why))
        if run < st["single_view_filter_loop_iterations"]:
            chosen = []
            for i in range(n):
                if len(chosen) == num:
                    break
                if consistent(i) and world[i][3] >= 0.0:
                    chosen.append(i)
            out["selected"].append(list(chosen))
    final = np.array([consistent(i) for i in range(n)], bool)
    out.update(final=final, robust=int(sum(1 for i in range(n) if final[i] and world[i][3] >= 0.0)))
    if out["robust"] <= robust_minimum_matches:
        return dict(out, verdict=LOST_HALF, stage="final")
    if int(final.sum()) < st["single_view_minimum_robust_landmarks"]:
        return dict(out, verdict=FEW_ROBUST)
    return dict(out, pose=pose)
