"""An independent float64 statement of cv-sfm's three-view bootstrap, in numpy, written from the definitions: sequential
sums over landmarks, numpy.linalg.eigh for the triangulations, np.sin / np.cos in Rodrigues' formula.  It shares no text
with include/akz_three_view_math.h; tests/test_three_view_math.py holds the header's host build to it.

Poses are CameraToCamera 3 x 4 arrays [R | t]; bearings are unit 3-vectors.
"""
import numpy as np


# ---- geometry ----
def unit(v):
    with np.errstate(all="ignore"):
        return v / np.linalg.norm(v)


def invert(pose):
    r, t = pose[:, :3], pose[:, 3]
    return np.hstack([r.T, (-r.T @ t)[:, None]])


def exp_so3(w):
    theta = np.linalg.norm(w)
    if not theta > 0:
        return np.eye(3)
    u = w / theta
    k = np.array([[0, -u[2], u[1]], [u[2], 0, -u[0]], [-u[1], u[0], 0]])
    return np.cos(theta) * np.eye(3) + np.sin(theta) * k + (1 - np.cos(theta)) * np.outer(u, u)


def from_homogeneous(p):
    p = np.array(p, np.float64)
    if np.signbit(p[3]):
        p = -p
    with np.errstate(all="ignore"):
        return p / np.linalg.norm(p[:3])


def triangulate(observations):
    """Linear-Eigen: the eigenvector of the smallest eigenvalue of sum (P - b b^T P)^T (P - b b^T P); None behind a camera."""
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


IDENT = np.hstack([np.eye(3), np.zeros((3, 1))])


def to_camera(c, others):
    p = triangulate([(IDENT, c)] + others)
    return None if p is None else from_homogeneous(p)


def transform_bearing(pose, p):
    return from_homogeneous(np.append(pose[:, :3] @ p[:3] + pose[:, 3] * p[3], p[3]))[:3]


def tri_margins(first, second, c, f, s):
    """(largest of the three cosine distances, largest of the three incidence cosine distances) or None."""
    p = to_camera(c, [(first, f), (second, s)])
    if p is None:
        return None
    fc, sc = first[:, :3].T @ f, second[:, :3].T @ s
    cos = max(1 - p[:3] @ c, 1 - transform_bearing(first, p) @ f, 1 - transform_bearing(second, p) @ s)
    inc = max(1 - c @ fc, 1 - c @ sc, 1 - fc @ sc)
    return cos, inc


def tri_robust(first, second, c, f, s, max_cos, min_inc, near=None):
    m = tri_margins(first, second, c, f, s)
    if m is None:
        return False
    if near is not None:
        near.extend([(m[0], max_cos), (m[1], min_inc)])
    return bool(m[0] < max_cos and m[1] > min_inc)


def loss(t, a, b):
    ca, cb = np.cross(a, t), np.cross(b, t)
    with np.errstate(all="ignore"):
        r = abs(a @ unit(cb)) if ca @ ca < cb @ cb else abs(b @ unit(ca))
    return 1.0 if (np.isnan(r) or np.signbit(a @ b)) else r


def bi_robust(pose, a, b, max_sine, near=None):
    v = loss(pose[:, 3], pose[:, :3] @ a, b)
    if near is not None:
        near.append((v, max_sine))
    return bool(v < max_sine)


# ---- the gradients (cv-geom/src/epipolar.rs), for n landmarks at once: arrays [n][3], one row per landmark ----
def _dot(a, b):
    return np.sum(a * b, axis=-1, keepdims=True)


def _unit(v):
    return v / np.sqrt(_dot(v, v))


def sine_l1(t, a, b):
    """-> (points [n][3] with A as the origin, valid [n])"""
    t = np.broadcast_to(t, a.shape)
    ca, cb = np.cross(a, t), np.cross(b, t)
    first = (np.sqrt(_dot(ca, ca)) < np.sqrt(_dot(cb, cb)))[:, 0]
    nb, na = _unit(cb), _unit(ca)
    a2 = np.where(first[:, None], _unit(a - _dot(a, nb) * nb), a)
    b2 = np.where(first[:, None], b, _unit(b - _dot(b, na) * na))
    z = np.cross(a2, b2)
    w = _dot(z, z) / _dot(z, np.cross(t, b2))
    p = np.hstack([a2, w])
    p = np.where(np.signbit(w), -p, p)
    p = p / np.sqrt(_dot(p[:, :3], p[:, :3]))
    ok = np.all(np.isfinite(p), axis=1) & ~np.signbit(_dot(p[:, :3], a2))[:, 0] & ~np.signbit(_dot(p[:, :3], b2))[:, 0] & (p[:, 3] != 0)
    return p[:, :3] / p[:, 3:4], ok


def rotation_gradient(t, a, b):
    t = np.broadcast_to(t, a.shape)
    return np.cross(_unit(np.cross(b, t)), _unit(np.cross(a, t)))


def clean(v):
    return np.where(np.any(np.isnan(v), axis=1, keepdims=True), 0.0, v)


def three_view_gradients(c, f, ftoc, s, stoc):
    """[n][12]: first translation, first rotation, second translation, second rotation"""
    with np.errstate(all="ignore"):
        stof = stoc - ftoc
        rot_cf, rot_cs, rot_fs = rotation_gradient(ftoc, c, f), rotation_gradient(stoc, c, s), rotation_gradient(stof, f, s)
        p, ok = sine_l1(-stoc, c, s)
        p = p - ftoc
        trans_f = np.where(ok[:, None], p - _dot(p, f) * f, 0.0)
        p, ok = sine_l1(-ftoc, c, f)
        p = p - stoc
        trans_s = np.where(ok[:, None], p - _dot(p, s) * s, 0.0)
        p, ok = sine_l1(-stof, f, s)
        p = p + ftoc
        trans_c = np.where(ok[:, None], _dot(p, c) * c - p, 0.0)
        return np.hstack([clean(trans_f * (2 / 3) + trans_c * (1 / 3)), clean(rot_cf * (2 / 3) - rot_fs * (1 / 3)),
                          clean(trans_s * (2 / 3) + trans_c * (1 / 3)), clean(rot_cs * (2 / 3) + rot_fs * (1 / 3))])


def landmark_gradients(inv, c, f, s):
    c, f, s = (np.atleast_2d(np.asarray(x, np.float64)) for x in (c, f, s))
    return three_view_gradients(c, f @ inv[0][:, :3].T, inv[0][:, 3], s @ inv[1][:, :3].T, inv[1][:, 3])


# ---- the optimiser (cv-optimize/src/three_view_optimizer.rs:126-200) ----
def optimize(poses, rate, iterations, landmarks):
    """-> ([first, second], the iteration the loop was left at).  The landmarks' gradients are added one after another."""
    if len(landmarks) == 0:
        return [p.copy() for p in poses], 0
    lm = np.asarray(landmarks, np.float64).reshape(-1, 3, 3)
    c, f, s = (np.ascontiguousarray(lm[:, k]) for k in range(3))
    inv = [invert(p) for p in poses]
    best = np.full(4, np.inf)
    no_improve = 0
    iteration = 0
    for iteration in range(iterations):
        net = np.add.reduce(np.ascontiguousarray(landmark_gradients(inv, c, f, s)), axis=0)   # row after row
        delta = net * (rate / len(lm))
        no_improve += 1
        for k in range(4):
            n = np.linalg.norm(net[3 * k:3 * k + 3])
            if best[k] > n:
                best[k] = n
                no_improve = 0
        if no_improve >= 50:
            break
        for k in range(2):
            r = exp_so3(delta[6 * k + 3:6 * k + 6])
            inv[k] = np.hstack([r @ inv[k][:, :3], (r @ delta[6 * k:6 * k + 3] + r @ inv[k][:, 3])[:, None]])
    return [invert(p) for p in inv], iteration


# ---- the procedure (cv-sfm/src/lib.rs:1002-1300) ----
DEFAULTS = dict(maximum_cosine_distance=1e-5, maximum_sine_distance=1e-1, robust_observation_incidence_minimum_cosine_distance=1e-3,
                robust_view_bearing_pair_minimum_cosine_distance=1e-2, optimization_rate=0.001, robust_view_num_robust_bearing_pair=3,
                three_view_minimum_relative_scales=16, three_view_filter_loop_iterations=8, three_view_optimization_landmarks=1024,
                three_view_patience=65536, three_view_minimum_robust_matches=32, hard_minimum_matches=32)
VERDICTS = dict(ok=0, few_scales=1, few_bearing_pairs=2, few_matches=3, lost_half=4, few_robust=5, bad_index=6)


def relative_scale(first, second, c, f, s, st, near=None):
    if not tri_robust(first, second, c, f, s, 1.0, st["robust_observation_incidence_minimum_cosine_distance"], near):
        return None
    fp, sp = to_camera(c, [(first, f)]), to_camera(c, [(second, s)])
    if fp is None or sp is None or fp[3] == 0 or sp[3] == 0:
        return None
    with np.errstate(all="ignore"):
        fp, sp = fp[:3] / fp[3], sp[:3] / sp[3]
        r = (fp @ fp) / (sp @ sp)
    return r if np.isfinite(r) and abs(r) >= np.finfo(np.float64).tiny else None


def init_triple(pose_in, common, first_only, second_only, settings=None):
    """common: list of (c, f, s) bearings; first_only / second_only: lists of (c, other).  -> dict with verdict, poses,
    masks, counts, and `near`: every (quantity, threshold) pair a decision compared."""
    st = dict(DEFAULTS, **(settings or {}))
    out = dict(verdict=None, near=[], run_matches=[], run_stop=[])
    near = out["near"]
    first, second = pose_in[0].copy(), pose_in[1].copy()
    inc = st["robust_observation_incidence_minimum_cosine_distance"]
    ratios = [r for r in (relative_scale(first, second, c, f, s, st, near) for c, f, s in common) if r is not None]
    out["scales"] = len(ratios)
    if len(ratios) < st["three_view_minimum_relative_scales"]:
        out["verdict"] = VERDICTS["few_scales"]
        return out
    out["median"] = float(np.sqrt(sorted(ratios)[len(ratios) // 2]))
    second[:, 3] = second[:, 3] * out["median"]

    def take(max_cos):
        got = []
        for c, f, s in common:
            if len(got) == st["three_view_optimization_landmarks"]:
                break
            if tri_robust(first, second, c, f, s, max_cos, inc, near):
                got.append((c, f, s))
        return got

    opti = take(1.0)
    pairs = 0
    thr = st["robust_view_bearing_pair_minimum_cosine_distance"]
    if opti:
        m = [np.array([o[k] for o in opti]) for k in range(3)]
        d = [1 - x @ x.T for x in m]
        iu = np.triu_indices(len(opti), 1)
        for x in d:
            v = x[iu]
            k = np.argmin(np.abs(v - thr)) if len(v) else None
            if k is not None:
                near.append((v[k], thr))
        pairs = int(np.sum((d[0][iu] > thr) & (d[1][iu] > thr) & (d[2][iu] > thr)))
    out["pairs"] = pairs
    if pairs < st["robust_view_num_robust_bearing_pair"]:
        out["verdict"] = VERDICTS["few_bearing_pairs"]
        return out
    minimum = len(opti) // 2
    for run in range(st["three_view_filter_loop_iterations"] + 1):
        out["run_matches"].append(len(opti))
        if len(opti) < st["hard_minimum_matches"]:
            out["verdict"] = VERDICTS["few_matches"]
            return out
        if len(opti) <= minimum:
            out["verdict"] = VERDICTS["lost_half"]
            return out
        (first, second), stop = optimize([first, second], st["optimization_rate"], st["three_view_patience"], opti)
        out["run_stop"].append(stop)
        if run < st["three_view_filter_loop_iterations"]:
            opti = take(st["maximum_cosine_distance"])
    mc = st["maximum_cosine_distance"]
    out["combined"] = [tri_robust(first, second, c, f, s, mc, 0.0, near) for c, f, s in common]
    out["first_ok"] = [bi_robust(first, a, b, st["maximum_sine_distance"], near) for a, b in first_only]
    out["second_ok"] = [bi_robust(second, a, b, st["maximum_sine_distance"], near) for a, b in second_only]
    out["robust"] = sum(tri_robust(first, second, c, f, s, mc, inc, near) for c, f, s in common)
    out["poses"] = [first, second]
    if out["robust"] <= minimum:
        out["verdict"] = VERDICTS["lost_half"]
    elif out["robust"] < st["three_view_minimum_robust_matches"]:
        out["verdict"] = VERDICTS["few_robust"]
    else:
        out["verdict"] = VERDICTS["ok"]
    return out


def closest_margin(near):
    """the smallest relative distance between a compared quantity and its threshold"""
    return min((abs(v - t) / max(abs(t), 1e-300) for v, t in near if t != 0.0 and np.isfinite(v)), default=np.inf)
