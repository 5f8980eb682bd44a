"""An independent float64 statement of cv-sfm's three-view constraint, in numpy, written from the reference's text:
three_view_adaptive_optimize_l2 (cv-optimize/src/three_view_optimizer.rs:203-272) and optimize_three_view
(cv-sfm/src/lib.rs:1939-2062) behind its shuffle and sort.  Sums over landmarks are sequential, as the reference's are; poses
are multiplied as 4 x 4 matrices; np.sin / np.cos in Rodrigues' formula.  The gradients of a landmark are those of
tests/three_view_statement.py.  It shares no text with include/akz_three_view_constraint_math.h;
tests/test_three_view_constraint_math.py holds the header's host build to it.

Poses are 3 x 4 arrays [R | t]; a landmark is its three unit bearings (c, f, s).
"""
import numpy as np

from three_view_statement import exp_so3, landmark_gradients

DEFAULTS = dict(optimization_minimum_landmarks=24, optimization_maximum_landmarks=64, constraint_patience=4096,
                robust_view_num_robust_bearing_pair=3, robust_view_bearing_pair_minimum_cosine_distance=1e-2)
VERDICTS = dict(ok=0, few_landmarks=1, few_bearing_pairs=2, bad_index=3)


def mat4(pose):
    return np.vstack([np.asarray(pose, np.float64).reshape(3, 4), [0.0, 0.0, 0.0, 1.0]])


def inverse(pose):
    """Isometry3::inverse"""
    r, t = pose[:, :3], pose[:, 3]
    return np.hstack([r.T, -(r.T @ t)[:, None]])


def compose(a, b):
    """a * b"""
    return (mat4(a) @ mat4(b))[:3]


def rates(net, norm_sums, inv_len):
    """(l2 [12], [trate1, rrate1, trate2, rrate2]) of one iteration's sums (three_view_optimizer.rs:233-249)"""
    l2 = net * inv_len
    std = norm_sums * inv_len
    out = []
    with np.errstate(all="ignore"):
        for v in range(4):
            rate = np.linalg.norm(l2[3 * v:3 * v + 3]) / std[v]
            out.append(rate if np.isfinite(rate) else 0.0)
    return l2, out


def sums(inv, c, f, s):
    """the landmarks' gradients and their four norms, added one landmark after another"""
    g = np.ascontiguousarray(landmark_gradients(inv, c, f, s))                     # [n][12]
    norms = np.ascontiguousarray(np.sqrt(np.sum(g.reshape(len(g), 4, 3) ** 2, axis=2)))   # [n][4]
    return np.add.reduce(g, axis=0), np.add.reduce(norms, axis=0)


def adaptive_optimize(poses, iterations, landmarks, trace=None):
    """-> [first, second].  `trace`, a list, receives the four rates of every iteration."""
    lm = np.asarray(landmarks, np.float64).reshape(-1, 3, 3)
    if len(lm) == 0:
        return [np.array(p, np.float64) for p in poses]
    c, f, s = (np.ascontiguousarray(lm[:, k]) for k in range(3))
    inv_len = 1.0 / len(lm)
    inv = [inverse(np.asarray(p, np.float64)) for p in poses]
    for _ in range(iterations):
        net, norm_sums = sums(inv, c, f, s)
        l2, rate = rates(net, norm_sums, inv_len)
        if trace is not None:
            trace.append(rate)
        for k in range(2):
            translation, rotation = l2[6 * k:6 * k + 3] * rate[2 * k], l2[6 * k + 3:6 * k + 6] * rate[2 * k + 1]
            r = exp_so3(rotation)
            delta = np.hstack([r, (r @ translation)[:, None]])
            inv[k] = compose(delta, inv[k])
    return [inverse(p) for p in inv]


def scale_of(first, second):
    return np.linalg.norm(first[:, 3]) + np.linalg.norm(second[:, 3])


def pair_distances(landmarks):
    """[3][pairs]: 1 - a . b in each of the three views for every i < j"""
    lm = np.asarray(landmarks, np.float64).reshape(-1, 3, 3)
    iu = np.triu_indices(len(lm), 1)
    return np.stack([(1.0 - lm[:, k] @ lm[:, k].T)[iu] for k in range(3)])


def constraint(world_poses, landmarks, settings=None, trace=None):
    """world_poses: the three views' WorldToCamera poses; landmarks: the list behind the caller's shuffle and sort.
    -> dict(verdict, landmarks, and as far as reached: used, pairs, closest (how near a pair came to the threshold),
    original_scale, final_scale, poses)."""
    st = dict(DEFAULTS, **(settings or {}))
    lm = np.asarray(landmarks, np.float64).reshape(-1, 3, 3)
    out = dict(verdict=None, landmarks=len(lm))
    if len(lm) < st["optimization_minimum_landmarks"]:
        out["verdict"] = VERDICTS["few_landmarks"]
        return out
    w = [np.asarray(p, np.float64).reshape(3, 4) for p in world_poses]
    first, second = compose(w[1], inverse(w[0])), compose(w[2], inverse(w[0]))
    out["original_scale"] = scale_of(first, second)
    opti = lm[:st["optimization_maximum_landmarks"]]
    thr = st["robust_view_bearing_pair_minimum_cosine_distance"]
    d = pair_distances(opti)
    out["used"] = len(opti)
    out["pairs"] = int(np.sum(np.all(d > thr, axis=0)))
    out["closest"] = float(np.min(np.abs(d - thr))) if d.size else np.inf
    if out["pairs"] < st["robust_view_num_robust_bearing_pair"]:
        out["verdict"] = VERDICTS["few_bearing_pairs"]
        return out
    first, second = adaptive_optimize([first, second], st["constraint_patience"], opti, trace)
    out["final_scale"] = scale_of(first, second)
    with np.errstate(all="ignore"):
        relative_scale = out["original_scale"] / out["final_scale"]
    for p in (first, second):
        p[:, 3] = p[:, 3] * relative_scale
    out["poses"] = [first, second]
    out["verdict"] = VERDICTS["ok"]
    return out
