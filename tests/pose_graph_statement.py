"""An independent float64 statement of cv-sfm's pose-graph relaxation, written from the Rust text with numpy — it does not
include include/akz_pose_graph_math.h, uses numpy's arccos / sin / cos and a sequential sum, and knows nothing of waves.

  ThreeViewConstraint::edge_constraints               cv-sfm/src/lib.rs:167-180
  VSlam::constrain_view                               cv-sfm/src/lib.rs:1892-1936
  apply_constraints / compute_momentum_bundle_adjust  cv-sfm/src/lib.rs:2358-2414
  CameraToCamera::se3 / from_se3                      cv-core/src/pose.rs:54-66
  Skew3 from Rotation3                                cv-core/src/so3.rs:263-275

Poses are [3][4] arrays [R | t].  A graph is a dict view -> list of (other view, expected other-to-view [3][4]), which is
what flatten_constraints builds."""
import numpy as np

RATE = 1e-3          # graph_optimization_rate, cv-sfm/src/settings.rs:477-479
ITERATIONS = 1024    # optimization_iterations, settings.rs:461-463


def mul(a, b):
    """the product of two isometries: {Ra Rb, Ra tb + ta}"""
    out = np.empty((3, 4))
    out[:, :3] = a[:, :3] @ b[:, :3]
    out[:, 3] = a[:, :3] @ b[:, 3] + a[:, 3]
    return out


def inverse(p):
    out = np.empty((3, 4))
    out[:, :3] = p[:, :3].T
    out[:, 3] = -(p[:, :3].T @ p[:, 3])
    return out


def exp(w):
    """Rotation3::from_scaled_axis"""
    w = np.asarray(w, np.float64)
    theta = np.linalg.norm(w)
    if not theta > 0.0:
        return np.eye(3)
    u = w / theta
    k = np.array([[0.0, -u[2], u[1]], [u[2], 0.0, -u[0]], [-u[1], u[0], 0.0]])
    return np.cos(theta) * np.eye(3) + np.sin(theta) * k + (1.0 - np.cos(theta)) * np.outer(u, u)


def log(r):
    """Skew3::from(Rotation3): scaled_axis = axis * angle, angle = acos(clamp((trace - 1) / 2, -1, 1)), axis =
    Unit::try_new((m32 - m23, m13 - m31, m21 - m12), EPSILON), zero when try_new refuses or a component is NaN"""
    r = np.asarray(r, np.float64)
    with np.errstate(invalid="ignore"):
        angle = np.arccos(np.clip((np.trace(r) - 1.0) / 2.0, -1.0, 1.0))
    v = np.array([r[2, 1] - r[1, 2], r[0, 2] - r[2, 0], r[1, 0] - r[0, 1]])
    n = np.linalg.norm(v)
    if not n > np.finfo(np.float64).eps:
        return np.zeros(3)
    w = v / n * angle
    return np.zeros(3) if np.any(np.isnan(w)) else w


def se3(delta):
    """CameraToCamera::se3: translation, then the rotation's Skew3"""
    return np.concatenate([delta[:, 3], log(delta[:, :3])])


def from_se3(v):
    """CameraToCamera::from_se3 = from_parts(translation, exp(rotation)): the translation is not rotated"""
    return np.hstack([exp(v[3:]), np.asarray(v[:3], np.float64).reshape(3, 1)])


def edge_constraints(views, first, second):
    """the six (target, (other, expected other-to-target)) of a constraint, in the reference's order"""
    v0, v1, v2 = (int(x) for x in views)
    f2s = mul(second, inverse(first))
    return [(v0, (v2, inverse(second))), (v0, (v1, inverse(first))), (v1, (v0, first)), (v1, (v2, inverse(f2s))), (v2, (v1, f2s)),
            (v2, (v0, second))]


def flatten(constraints):
    """flatten_constraints over a list of (views, first, second): view -> [(other, expected)] in the list's order"""
    graph = {}
    for views, first, second in constraints:
        for target, entry in edge_constraints(views, first, second):
            graph.setdefault(target, []).append(entry)
    return graph


def constrain_view(poses, view, graph, rate=RATE):
    """-> the view's new pose, or None (no constraint, or a net delta that is not finite)"""
    if view not in graph:
        return None
    inv = inverse(poses[view])
    net = np.zeros(6)
    with np.errstate(invalid="ignore"):
        for other, expected in graph[view]:
            net = net + se3(mul(mul(expected, poses[other]), inv))
        net = net * rate
    if not np.all(np.isfinite(net)):
        return None
    return mul(from_se3(net), poses[view])


def relax(poses, graph, iterations=ITERATIONS, rate=RATE):
    """apply_constraints on a dict or list of poses -> (poses, rounds run, views that returned None in the last round).
    Stops where the device stops: at the first round in which a view WITH constraints returns None."""
    poses = {v: np.array(p, np.float64) for v, p in (poses.items() if isinstance(poses, dict) else enumerate(poses))}
    if sum(1 for v in poses if v in graph) < 3:
        return poses, 0, [v for v in poses if v not in graph]
    for k in range(iterations):
        new = {v: constrain_view(poses, v, graph, rate) for v in poses}
        bad = [v for v, p in new.items() if p is None and v in graph]
        poses = {v: (poses[v] if p is None else p) for v, p in new.items()}
        if bad:
            return poses, k + 1, bad
    return poses, iterations, []


def residual(poses, graph):
    """the largest |se3(expected * w_other * w_view^-1)| over the graph's edges"""
    worst = 0.0
    for view, entries in graph.items():
        inv = inverse(poses[view])
        for other, expected in entries:
            worst = max(worst, float(np.linalg.norm(se3(mul(mul(expected, poses[other]), inv)))))
    return worst
