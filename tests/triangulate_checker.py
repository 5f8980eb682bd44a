"""The CPU checker of the triangulation kernels for the tests: tests/cpp/triangulate_host.c (thin wrappers around
include/akz_triangulate_math.h) as host_build.load compiles it — the host compiler, no contraction to FMA, as the kernels —
loaded with ctypes; plus the synthetic maps both test files use."""
import ctypes as C

import numpy as np

import host_build

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("response", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("octave", "<u4"),
                     ("class_id", "<u4")])
NONE = np.array([0.0, 0.0, 0.0, -1.0])


class Settings(C.Structure):
    """akz_tri_settings (include/akz_triangulate_math.h)."""
    _fields_ = [("eps", C.c_double), ("max_sweeps", C.c_int), ("robust_minimum_observations", C.c_uint),
                ("n_views", C.c_uint), ("incidence_minimum_cosine_distance", C.c_double)]


class Camera(C.Structure):
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("skew", C.c_double),
                ("k1", C.c_double), ("use_k1", C.c_int32), ("reserved", C.c_int32)]


def settings(eps=1e-12, max_sweeps=1000, robust_minimum_observations=3, n_views=0xFFFFFFFF, min_cos=1e-3):
    return Settings(eps, max_sweeps, robust_minimum_observations, n_views, min_cos)


def camera(fx, fy, cx, cy, skew=0.0, k1=None):
    return Camera(fx, fy, cx, cy, skew, k1 or 0.0, int(k1 is not None), 0)


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    L = host_build.load("triangulate_host.c")
    vp, u32 = C.c_void_p, C.c_uint32
    sp, cp = C.POINTER(Settings), C.POINTER(Camera)
    L.tri_observations.argtypes = [vp, vp, u32, C.c_int, sp, vp]
    L.tri_landmarks.argtypes = [vp, u32, u32, vp, cp, vp, vp, u32, u32, sp, vp, vp]
    L.tri_landmarks.restype = None
    L.tri_merged.argtypes = [vp, u32, u32, vp, cp, vp, vp, u32, u32, sp, vp, vp, vp, u32, u32, vp, vp]
    L.tri_merged.restype = None
    L.tri_pairs_scene.argtypes = [vp, vp, u32, vp, u32, cp, cp, vp, vp, u32, sp, vp, vp]
    L.tri_pairs_scene.restype = None
    L.tri_solve.argtypes = [vp, C.c_double, C.c_int, vp]
    L.tri_from_homogeneous.argtypes = [vp]
    L.tri_from_homogeneous.restype = None
    L.tri_accumulate.argtypes = [vp, vp, vp]
    L.tri_accumulate.restype = None
    L.tri_float_ord.argtypes = [C.c_double]
    L.tri_float_ord.restype = C.c_uint64
    L.tri_calibrate.argtypes = [cp, C.c_float, C.c_float, vp]
    L.tri_calibrate.restype = None
    _lib = L
    return L


def observations(poses, bearings, robust=False, st=None):
    """(point [4], reason) of one list: poses [n][3][4], bearings [n][3]."""
    P = np.ascontiguousarray(poses, np.float64).reshape(-1, 12)
    B = np.ascontiguousarray(bearings, np.float64).reshape(-1, 3)
    assert len(P) == len(B)
    out = np.empty(4, np.float64)
    st = st or settings()
    why = lib().tri_observations(P.ctypes.data, B.ctypes.data, len(P), int(robust), C.byref(st), out.ctypes.data)
    return out, why


def landmarks(kps, poses, cam, start, obs, st=None, n_obs=None):
    """(world [n][4], reason [n]) of a CSR table: kps [blocks][cap] KP_DTYPE, poses [blocks][12], start [n + 1], obs [..][2]."""
    kps = np.ascontiguousarray(kps)
    P = np.ascontiguousarray(poses, np.float64).reshape(-1, 12)
    start = np.ascontiguousarray(start, np.uint32)
    obs = np.ascontiguousarray(obs, np.uint32).reshape(-1, 2)
    n = len(start) - 1
    world = np.empty((n, 4), np.float64)
    reason = np.empty(n, np.uint8)
    st = st or settings()
    lib().tri_landmarks(kps.ctypes.data, kps.shape[1], kps.shape[0], P.ctypes.data, C.byref(cam), start.ctypes.data, obs.ctypes.data,
                        len(obs) if n_obs is None else n_obs, n, C.byref(st), world.ctypes.data, reason.ctypes.data)
    return world, reason


def merged(kps, poses, cam, start, obs, best, decision, merge_ok, n_world, world, st=None, n_obs=None):
    """Writes the merge candidates' rows into `world` (in place); returns reason [frames][cap] (255 = row not written).
    n_obs: the length of the observation array as the call states it (len(obs) where not given)."""
    kps = np.ascontiguousarray(kps)
    P = np.ascontiguousarray(poses, np.float64).reshape(-1, 12)
    start = np.ascontiguousarray(start, np.uint32)
    obs = np.ascontiguousarray(obs, np.uint32).reshape(-1, 2)
    best = np.ascontiguousarray(best, np.uint32)
    decision = np.ascontiguousarray(decision, np.uint32)
    merge_ok = np.ascontiguousarray(merge_ok, np.uint8)
    F, cap = decision.shape
    assert best.shape == (F, cap, 3, 2) and merge_ok.shape == (F, cap) and cap == kps.shape[1] and world.flags.c_contiguous
    reason = np.full((F, cap), 255, np.uint8)
    st = st or settings()
    lib().tri_merged(kps.ctypes.data, cap, kps.shape[0], P.ctypes.data, C.byref(cam), start.ctypes.data, obs.ctypes.data,
                     len(obs) if n_obs is None else n_obs, len(start) - 1, C.byref(st), best.ctypes.data, decision.ctypes.data, merge_ok.ctypes.data, F, n_world,
                     world.ctypes.data, reason.ctypes.data)
    return reason


def pairs_scene(kps_a, kps_b, pairs, npairs, cam_a, cam_b, pose, inliers, st=None, n_inliers=None):
    """(points [n_inliers][4], reason) of one scene of a two-view consensus; kps_a / kps_b [cap] KP_DTYPE, pairs [cap][2].
    n_inliers: the count as the call states it (len(inliers) where not given); one above the capacity is clamped to it, and
    the rows that come back are the clamped count's."""
    kps_a, kps_b = np.ascontiguousarray(kps_a), np.ascontiguousarray(kps_b)
    pairs = np.ascontiguousarray(pairs, np.uint32)
    pose = np.ascontiguousarray(pose, np.float64).reshape(12)
    inliers = np.ascontiguousarray(inliers, np.uint32)
    stated = len(inliers) if n_inliers is None else int(n_inliers)
    n = min(stated, len(kps_a))
    assert len(inliers) >= n
    pts = np.empty((max(n, 1), 4), np.float64)
    reason = np.empty(max(n, 1), np.uint8)
    st = st or settings()
    lib().tri_pairs_scene(kps_a.ctypes.data, kps_b.ctypes.data, len(kps_a), pairs.ctypes.data, int(npairs), C.byref(cam_a),
                          C.byref(cam_b), pose.ctypes.data, inliers.ctypes.data, stated, C.byref(st), pts.ctypes.data,
                          reason.ctypes.data)
    return pts[:n], reason[:n]


def solve(a, eps=1e-12, max_sweeps=1000):
    a = np.ascontiguousarray(a, np.float64).reshape(16)
    out = np.empty(4, np.float64)
    why = lib().tri_solve(a.ctypes.data, eps, max_sweeps, out.ctypes.data)
    return out, why


def from_homogeneous(p):
    p = np.array(p, np.float64)
    lib().tri_from_homogeneous(p.ctypes.data)
    return p


# ---- synthetic geometry --------------------------------------------------------------------------------------------
def rodrigues(v):
    """Rotation3::new(v): the rotation of the scaled axis v."""
    v = np.asarray(v, np.float64)
    th = np.linalg.norm(v)
    if th == 0.0:
        return np.eye(3)
    k = v / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def random_poses(rng, n, min_gap=0.1, rot=0.05):
    """n WorldToCamera poses [n][3][4]: camera centres uniform in [-1, 1] x [-1, 1] x [-0.3, 0.3], every two at least
    min_gap apart, rotations of about `rot` rad."""
    centres = []
    while len(centres) < n:
        c = rng.uniform([-1, -1, -0.3], [1, 1, 0.3])
        if all(np.linalg.norm(c - d) >= min_gap for d in centres):
            centres.append(c)
    out = np.empty((n, 3, 4))
    for i, c in enumerate(centres):
        R = rodrigues(rng.normal(0, rot, 3))
        out[i, :, :3] = R
        out[i, :, 3] = -R @ c
    return out


def project(pose, X, f, cx, cy):
    q = pose[:, :3] @ X + pose[:, 3]
    return f * q[0] / q[2] + cx, f * q[1] / q[2] + cy


def synthetic_map(rng, n_blocks, cap, n_landmarks, f=1000.0, cx=960.0, cy=540.0, noise=0.5, max_len=32, long_lists=0):
    """A map for the landmark-table tests: n_blocks cameras (poses), n_landmarks points 2-10 units deep, each observed by
    0..max_len blocks (list lengths mixed at random, so every wave holds all of them; `long_lists` of them longer than 32),
    every observation a keypoint slot of its block holding the projection + pixel noise.  Returns (kps [blocks][cap], poses
    [blocks][12], start, obs, points).  The slots of a block are handed out in order; a block that is full is skipped."""
    poses = random_poses(rng, n_blocks)
    kps = np.zeros((n_blocks, cap), KP_DTYPE)
    used = np.zeros(n_blocks, np.int64)
    pts = np.stack([rng.uniform(-2, 2, n_landmarks), rng.uniform(-1.5, 1.5, n_landmarks), rng.uniform(2, 10, n_landmarks)], 1)
    lens = rng.integers(0, max_len + 1, n_landmarks)
    if long_lists:
        lens[rng.choice(n_landmarks, long_lists, replace=False)] = rng.integers(33, min(n_blocks, 48) + 1, long_lists)
    lens = np.minimum(lens, n_blocks)
    start, obs = [0], []
    for l in range(n_landmarks):
        blocks = rng.permutation(n_blocks)[:lens[l]]
        for b in blocks:
            if used[b] >= cap:
                continue
            x, y = project(poses[b], pts[l], f, cx, cy)
            j = used[b]
            used[b] += 1
            kps[b, j]["x"] = x + rng.uniform(-noise, noise)
            kps[b, j]["y"] = y + rng.uniform(-noise, noise)
            obs.append((b, j))
        start.append(len(obs))
    return kps, poses.reshape(n_blocks, 12), np.array(start, np.uint32), np.array(obs, np.uint32).reshape(-1, 2), pts
