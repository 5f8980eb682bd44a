"""The CPU checker of the three-view constraint kernel for the tests: tests/cpp/three_view_constraint_host.c (thin wrappers
around include/akz_three_view_constraint_math.h) as host_build.load compiles it — the host compiler, no contraction to FMA,
as the kernel — loaded with ctypes; plus the synthetic scenes both test files use."""
import ctypes as C

import numpy as np

import host_build
import three_view_checker as K
import three_view_constraint_statement as S
from triangulate_checker import KP_DTYPE, Camera

STATS = 8
S_LANDMARKS, S_USED, S_PAIRS, S_ORIGINAL_SCALE, S_FINAL_SCALE, S_STAGE = 0, 1, 2, 3, 5, 7
OK, FEW_LANDMARKS, FEW_BEARING_PAIRS, BAD_INDEX = range(4)
PAIR_MARGIN = 1e-9   # a scene in which the statement puts a pair this near the 1e-2 threshold is not used


class Settings(C.Structure):
    """akz_tvc_settings (include/akz_three_view_constraint_math.h)."""
    _fields_ = [("robust_view_bearing_pair_minimum_cosine_distance", C.c_double), ("optimization_minimum_landmarks", C.c_uint),
                ("optimization_maximum_landmarks", C.c_uint), ("constraint_patience", C.c_uint),
                ("robust_view_num_robust_bearing_pair", C.c_uint)]


def settings(**kw):
    """The reference's defaults (cv-sfm/src/settings.rs:332-338, 465-483) with `kw` on top."""
    st = Settings(1e-2, 24, 64, 4096, 3)
    for k, v in kw.items():
        assert hasattr(st, k), k
        setattr(st, k, v)
    return st


def settings_dict(st):
    return {n: getattr(st, n) for n, _ in Settings._fields_}


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    L = host_build.load("three_view_constraint_host.c")
    vp, u32, dbl = C.c_void_p, C.c_uint32, C.c_double
    sp = C.POINTER(Settings)
    L.tvc_pose_mul.argtypes = [vp, vp, vp]
    L.tvc_pose_mul.restype = None
    L.tvc_relative_poses.argtypes = [vp, vp]
    L.tvc_relative_poses.restype = None
    L.tvc_rate.argtypes = [dbl, dbl]
    L.tvc_rate.restype = dbl
    L.tvc_adaptive_step.argtypes = [vp, dbl, vp]
    L.tvc_adaptive_step.restype = None
    L.tvc_sums.argtypes = [vp, vp, u32, C.c_int, vp]
    L.tvc_adaptive_optimize.argtypes = [vp, u32, vp, u32, C.c_int]
    L.tvc_constraint.argtypes = [vp, vp, u32, sp, C.c_int, vp, vp]
    L.tvc_constraint_scene.argtypes = [vp, u32, u32, vp, C.POINTER(Camera), vp, vp, vp, u32, u32, sp, vp, vp]
    _lib = L
    return L


def _a(x, dt=np.float64):
    return np.ascontiguousarray(x, dt)


def pose_mul(a, b):
    a, b, out = _a(a).reshape(12), _a(b).reshape(12), np.empty(12)
    lib().tvc_pose_mul(a.ctypes.data, b.ctypes.data, out.ctypes.data)
    return out.reshape(3, 4)


def relative_poses(world):
    w, out = _a(world).reshape(36), np.empty(24)
    lib().tvc_relative_poses(w.ctypes.data, out.ctypes.data)
    return out.reshape(2, 3, 4)


def rate(norm, std):
    return lib().tvc_rate(norm, std)


def adaptive_step(nets16, inv_len, inv):
    n, p = _a(nets16).reshape(16), _a(inv).reshape(24).copy()
    lib().tvc_adaptive_step(n.ctypes.data, inv_len, p.ctypes.data)
    return p.reshape(2, 3, 4)


def sums(inv, landmarks, sequential=False):
    """the 16 sums of one iteration: 12 gradient components, then the four norms"""
    inv, lm = _a(inv).reshape(24), _a(landmarks).reshape(-1, 9)
    out = np.empty(16)
    assert lib().tvc_sums(inv.ctypes.data, lm.ctypes.data, len(lm), int(sequential), out.ctypes.data) == 0
    return out


def adaptive_optimize(poses, iterations, landmarks, sequential=False):
    """-> poses [2][3][4]; landmarks [n][3][3] = (c, f, s)"""
    p, lm = _a(poses).reshape(24).copy(), _a(landmarks).reshape(-1, 9)
    assert lib().tvc_adaptive_optimize(p.ctypes.data, iterations, lm.ctypes.data, len(lm), int(sequential)) == 0
    return p.reshape(2, 3, 4)


def stat_f64(stats, at):
    return float(np.asarray(stats[at:at + 2], np.uint32).copy().view(np.float64)[0])


def constraint(world, landmarks, st, sequential=False):
    """the host build on bearings: world [3][3][4], landmarks [n][3][3] in the caller's order"""
    w, lm = _a(world).reshape(36), _a(landmarks).reshape(-1, 9)
    pose_out, stats = np.full(24, np.nan), np.zeros(STATS, np.uint32)
    v = lib().tvc_constraint(w.ctypes.data, lm.ctypes.data, len(lm), C.byref(st), int(sequential), pose_out.ctypes.data, stats.ctypes.data)
    assert v >= 0
    return dict(verdict=v, poses=pose_out.reshape(2, 3, 4), stats=stats, landmarks=int(stats[S_LANDMARKS]), used=int(stats[S_USED]),
                pairs=int(stats[S_PAIRS]), original_scale=stat_f64(stats, S_ORIGINAL_SCALE), final_scale=stat_f64(stats, S_FINAL_SCALE))


def constraint_scene(kps, poses, cam, views, lm_start, lm, s, st, prior=None):
    """the host build on constraint s of the device call's inputs; `prior` [24]: what pose_out held before"""
    kps, poses = _a(kps, KP_DTYPE), _a(poses).reshape(-1, 12)
    views, lm_start, lm = _a(views, np.uint32).reshape(-1, 3), _a(lm_start, np.uint32), _a(lm, np.uint32).reshape(-1, 3)
    pose_out = np.zeros(24) if prior is None else np.array(prior, copy=True)
    stats = np.zeros(STATS, np.uint32)
    v = lib().tvc_constraint_scene(kps.ctypes.data, kps.shape[1], kps.shape[0], poses.ctypes.data, C.byref(cam), views.ctypes.data,
                                   lm_start.ctypes.data, lm.ctypes.data if len(lm) else None, len(lm), s, C.byref(st), pose_out.ctypes.data,
                                   stats.ctypes.data)
    assert v >= 0
    return dict(verdict=v, pose_out=pose_out, stats=stats)


# ---- synthetic scenes ----
class Scene:
    """Three views of an existing reconstruction looking at n landmarks 3 - 9 units deep: WorldToCamera poses `world`
    [3][3][4] (the first view anywhere in the world, the two others a rigid rig around it, each turned by `perturb` rad from
    the truth — what a registration leaves), pixel noise `noise` px at f = 1000.  `spread` scales the field the landmarks
    cover (a small one leaves no robust bearing pair)."""

    def __init__(self, seed, n, noise=0.5, perturb=2e-3, spread=1.0):
        rng = np.random.default_rng(seed)
        w0 = K.camera_to_camera(rng.uniform(-2.0, 2.0, 3), 0.3 * K.unit_vec(rng))
        rel = [K.camera_to_camera([1.0, 0.1, 0.05] + 0.1 * rng.standard_normal(3), [0.02, -0.12, 0.01]),
               K.camera_to_camera([-0.7, 0.25, -0.1] + 0.1 * rng.standard_normal(3), [-0.03, 0.10, 0.02])]
        z = rng.uniform(3.0, 9.0, n)
        pts = np.stack([spread * rng.uniform(-0.35, 0.35, n) * z, spread * rng.uniform(-0.2, 0.2, n) * z, z], 1)
        ident = np.hstack([np.eye(3), np.zeros((3, 1))])
        self.px = [np.asarray(K.project(p, pts) + noise * rng.standard_normal((n, 2)), np.float32) for p in (ident, rel[0], rel[1])]
        self.landmarks = np.stack([K.bearings_of(p) for p in self.px], 1)          # [n][3][3]
        world = [w0]
        for p in rel:
            q = p.copy()
            if perturb:
                q[:, :3] = K.rodrigues(perturb * K.unit_vec(rng)) @ q[:, :3]
            world.append(S.compose(q, w0))
        self.world = np.stack(world)
        self.n = n

    def closest_pair(self, maximum, threshold=1e-2):
        d = S.pair_distances(self.landmarks[:maximum])
        return float(np.min(np.abs(d - threshold))) if d.size else np.inf


def scene(seed, n, maximum=256, **kw):
    """The first of the scenes seed, seed + 1000, ... whose statement keeps every bearing pair of its first `maximum` landmarks
    PAIR_MARGIN away from the 1e-2 threshold (a count that may differ by rounding is no test of the count)."""
    for attempt in range(8):
        sc = Scene(seed + 1000 * attempt, n, **kw)
        if sc.closest_pair(maximum) > PAIR_MARGIN:
            return sc
    raise AssertionError(f"no usable scene for seed {seed}")


def device_arrays(scenes, cap, constraints=None):
    """The device call's inputs: scene k owns keypoint blocks and pose rows 3k .. 3k + 2; `constraints` is a list of (scene
    number, landmark numbers in list order or None for all) — default one constraint per scene with all its landmarks.
    -> kps [3K][cap], poses [3K][12], views [n][3], lm_start [n + 1], lm [n_lm][3]."""
    kps = np.zeros((3 * len(scenes), cap), KP_DTYPE)
    poses = np.zeros((3 * len(scenes), 12))
    for k, sc in enumerate(scenes):
        assert sc.n <= cap
        for v in range(3):
            kps["x"][3 * k + v, :sc.n], kps["y"][3 * k + v, :sc.n] = sc.px[v][:, 0], sc.px[v][:, 1]
            poses[3 * k + v] = sc.world[v].reshape(12)
    if constraints is None:
        constraints = [(k, None) for k in range(len(scenes))]
    views = np.array([[3 * k, 3 * k + 1, 3 * k + 2] for k, _ in constraints], np.uint32).reshape(-1, 3)
    lists = [np.repeat(np.asarray(np.arange(scenes[k].n) if order is None else order, np.uint32)[:, None], 3, axis=1) for k, order in constraints]
    lm_start = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint32)
    lm = np.concatenate(lists + [np.zeros((0, 3), np.uint32)])
    return kps, poses, views, lm_start, lm
