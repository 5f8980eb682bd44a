"""The CPU checker of the three-view kernel for the tests: tests/cpp/three_view_host.c (thin wrappers around
include/akz_three_view_math.h) as host_build.load compiles it — the host compiler, no contraction to FMA, as the kernel —
loaded with ctypes; plus the synthetic rigs both test files use."""
import ctypes as C

import numpy as np

import host_build
from triangulate_checker import KP_DTYPE, Camera, camera
from triangulate_checker import Settings as TriSettings

STATS = 24
S_SCALES, S_MEDIAN, S_PAIRS, S_RUN_MATCHES, S_RUN_STOP, S_ROBUST, S_STAGE = 0, 1, 3, 4, 13, 22, 23
FOCAL = 1000.0


class Settings(C.Structure):
    """akz_tv_settings (include/akz_three_view_math.h)."""
    _fields_ = [("maximum_cosine_distance", C.c_double), ("maximum_sine_distance", C.c_double),
                ("robust_observation_incidence_minimum_cosine_distance", C.c_double),
                ("robust_view_bearing_pair_minimum_cosine_distance", C.c_double), ("optimization_rate", C.c_double),
                ("robust_view_num_robust_bearing_pair", C.c_uint), ("three_view_minimum_relative_scales", C.c_uint),
                ("three_view_filter_loop_iterations", C.c_uint), ("three_view_optimization_landmarks", C.c_uint),
                ("three_view_patience", C.c_uint), ("three_view_minimum_robust_matches", C.c_uint),
                ("hard_minimum_matches", C.c_uint), ("tri", TriSettings)]


def settings(**kw):
    """The reference's defaults (cv-sfm/src/settings.rs:320-427) with `kw` on top."""
    st = Settings(1e-5, 1e-1, 1e-3, 1e-2, 0.001, 3, 16, 8, 1024, 65536, 32, 32, TriSettings(1e-12, 1000, 3, 0xFFFFFFFF, 1e-3))
    for k, v in kw.items():
        assert hasattr(st, k), k
        setattr(st, k, v)
    return st


def settings_dict(st):
    return {n: getattr(st, n) for n, _ in Settings._fields_ if n != "tri"}


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    L = host_build.load("three_view_host.c")
    vp, u32, dbl = C.c_void_p, C.c_uint32, C.c_double
    sp, cp = C.POINTER(Settings), C.POINTER(Camera)
    L.tv_gradients.argtypes = [vp] * 5
    L.tv_gradients.restype = None
    L.tv_three_view_gradients.argtypes = [vp] * 6
    L.tv_three_view_gradients.restype = None
    L.tv_sine_l1.argtypes = [vp] * 4
    L.tv_from_scaled_axis.argtypes = [vp, vp]
    L.tv_from_scaled_axis.restype = None
    L.tv_loss.argtypes = [vp] * 3
    L.tv_loss.restype = dbl
    L.tv_tri_robust.argtypes = [vp] * 5 + [dbl, dbl, sp]
    L.tv_bi_robust.argtypes = [vp, vp, vp, dbl]
    L.tv_relative_scale.argtypes = [vp] * 5 + [sp, vp]
    L.tv_sum.argtypes = [vp, vp, u32, C.c_int, vp]
    L.tv_optimize.argtypes = [vp, dbl, u32, vp, u32, C.c_int]
    L.tv_optimize.restype = u32
    L.tv_init_triple.argtypes = [vp, vp, vp, vp, u32, vp, vp, u32, vp, vp, u32, sp, C.c_int, vp, vp, vp, vp, vp]
    L.tv_init_scene.argtypes = [vp, u32, u32, u32, u32, u32, cp, vp, vp, u32, vp, u32, vp, u32, sp, vp, vp, vp, vp, vp]
    _lib = L
    return L


def _a(x, dt=np.float64):
    return np.ascontiguousarray(x, dt)


def gradients(inv, c, f, s):
    """the 12 gradient components of one landmark under the inverted poses inv [2][3][4]"""
    inv, c, f, s = _a(inv), _a(c), _a(f), _a(s)
    g = np.empty(12)
    lib().tv_gradients(inv.ctypes.data, c.ctypes.data, f.ctypes.data, s.ctypes.data, g.ctypes.data)
    return g


def gradient_sum(inv, landmarks, sequential=False):
    """the summed gradients [12] of landmarks [n][3][3] = (c, f, s) under the inverted poses inv [2][3][4]"""
    inv, lm, nets = _a(inv).reshape(24), _a(landmarks).reshape(-1, 9), np.empty(12)
    assert lib().tv_sum(inv.ctypes.data, lm.ctypes.data, len(lm), int(sequential), nets.ctypes.data) == 0
    return nets


def optimize(poses, rate, iterations, landmarks, sequential=False):
    """-> (poses [2][3][4], stopping iteration); landmarks [n][3][3] = (c, f, s)."""
    p = _a(poses).reshape(24).copy()
    lm = _a(landmarks).reshape(-1, 9)
    it = lib().tv_optimize(p.ctypes.data, rate, iterations, lm.ctypes.data, len(lm), int(sequential))
    assert it != 0xFFFFFFFF
    return p.reshape(2, 3, 4), it


def _result(v, n, nf, ns, pose_out, combined, first_ok, second_ok, stats):
    return dict(verdict=v, poses=pose_out.reshape(2, 3, 4), combined=combined[:n], first_ok=first_ok[:nf], second_ok=second_ok[:ns], stats=stats,
                scales=int(stats[S_SCALES]), median=float(stats[S_MEDIAN:S_MEDIAN + 2].copy().view(np.float64)[0]), pairs=int(stats[S_PAIRS]),
                robust=int(stats[S_ROBUST]))


def init_triple(pose_in, common, first_only, second_only, st, sequential=False):
    """the host build on bearings: common [n][3][3], first_only / second_only [m][2][3]"""
    cm, fo, so = _a(common).reshape(-1, 3, 3), _a(first_only).reshape(-1, 2, 3), _a(second_only).reshape(-1, 2, 3)
    col = lambda a, k: _a(a[:, k])
    c, f, s = col(cm, 0), col(cm, 1), col(cm, 2)
    fc, ff, sc, ss = col(fo, 0), col(fo, 1), col(so, 0), col(so, 1)
    pose_out = np.full(24, np.nan)
    combined, first_ok, second_ok = (np.full(max(1, len(x)), 255, np.uint8) for x in (cm, fo, so))
    stats = np.zeros(STATS, np.uint32)
    p = _a(pose_in).reshape(24)
    v = lib().tv_init_triple(p.ctypes.data, c.ctypes.data, f.ctypes.data, s.ctypes.data, len(cm), fc.ctypes.data, ff.ctypes.data, len(fo),
                             sc.ctypes.data, ss.ctypes.data, len(so), C.byref(st), int(sequential), pose_out.ctypes.data, combined.ctypes.data,
                             first_ok.ctypes.data, second_ok.ctypes.data, stats.ctypes.data)
    assert v >= 0
    return _result(v, len(cm), len(fo), len(so), pose_out, combined, first_ok, second_ok, stats)


def init_scene(kps, n_blocks, blocks, cam, pose_in, triples, n, first_only, n_first, second_only, n_second, st, prior=None):
    """the host build on one scene of the device call's inputs: kps [n_blocks][cap] KP_DTYPE, triples [cap][3] u32, ...;
    `prior` = (pose_out [24], combined, first_ok, second_ok [cap]) what the outputs held before (left as is where not written)."""
    cap = kps.shape[1]
    kps, triples, first_only, second_only = _a(kps, KP_DTYPE), _a(triples, np.uint32), _a(first_only, np.uint32), _a(second_only, np.uint32)
    if prior is None:
        prior = (np.zeros(24), np.zeros(cap, np.uint8), np.zeros(cap, np.uint8), np.zeros(cap, np.uint8))
    pose_out, combined, first_ok, second_ok = (np.array(x, copy=True) for x in prior)
    stats = np.zeros(STATS, np.uint32)
    p = _a(pose_in).reshape(24)
    v = lib().tv_init_scene(kps.ctypes.data, cap, n_blocks, blocks[0], blocks[1], blocks[2], C.byref(cam), p.ctypes.data, triples.ctypes.data, n,
                            first_only.ctypes.data, n_first, second_only.ctypes.data, n_second, C.byref(st), pose_out.ctypes.data,
                            combined.ctypes.data, first_ok.ctypes.data, second_ok.ctypes.data, stats.ctypes.data)
    assert v >= 0
    return dict(verdict=v, pose_out=pose_out, combined=combined, first_ok=first_ok, second_ok=second_ok, stats=stats)


# ---- synthetic rigs ----
def rodrigues(w):
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / th
    return np.eye(3) + np.sin(th) * k + (1 - np.cos(th)) * (k @ k)


def camera_to_camera(position, axis_angle):
    """[R | t] taking centre-camera coordinates to those of a camera at `position`, turned by `axis_angle`"""
    r = rodrigues(axis_angle).T
    return np.hstack([r, (-r @ np.asarray(position, np.float64))[:, None]])


CAM = dict(fx=FOCAL, fy=FOCAL, cx=640.0, cy=360.0)


def project(pose, pts):
    x = pts @ pose[:, :3].T + pose[:, 3]
    return np.stack([CAM["fx"] * x[:, 0] / x[:, 2] + CAM["cx"], CAM["fy"] * x[:, 1] / x[:, 2] + CAM["cy"]], 1)


def bearings_of(px):
    """CameraIntrinsics::calibrate of f32 pixel positions, in numpy"""
    px = np.asarray(px, np.float32).astype(np.float64)
    v = np.stack([(px[:, 0] - CAM["cx"]) / CAM["fx"], (px[:, 1] - CAM["cy"]) / CAM["fy"], np.ones(len(px))], 1)
    return v / np.linalg.norm(v, axis=1, keepdims=True)


class Rig:
    """A rigid three-camera rig looking at n points 3 - 9 units deep, pixel noise `noise` px at f = 1000.  pose_in: the two
    true poses, each with its translation at unit length (what a two-view consensus leaves) and turned by `perturb` rad;
    `outliers` of the common matches are 20 - 40 px off in the second view."""

    def __init__(self, seed, n, noise=0.0, perturb=0.0, n_first=0, n_second=0, outliers=0):
        rng = np.random.default_rng(seed)
        self.first = camera_to_camera([1.0, 0.1, 0.05], [0.02, -0.12, 0.01])
        self.second = camera_to_camera([-0.7, 0.25, -0.1], [-0.03, 0.10, 0.02])
        m = n + n_first + n_second
        z = rng.uniform(3.0, 9.0, m)
        self.points = np.stack([rng.uniform(-0.35, 0.35, m) * z, rng.uniform(-0.2, 0.2, m) * z, z], 1)
        ident = np.hstack([np.eye(3), np.zeros((3, 1))])
        self.px = [project(p, self.points) + noise * rng.standard_normal((m, 2)) for p in (ident, self.first, self.second)]
        for k in rng.choice(n, outliers, replace=False) if outliers else []:
            self.px[2][k] += rng.choice([-1.0, 1.0], 2) * rng.uniform(20.0, 40.0, 2)
        self.px = [np.asarray(p, np.float32) for p in self.px]
        b = [bearings_of(p) for p in self.px]
        self.common = np.stack([b[0][:n], b[1][:n], b[2][:n]], 1)
        self.first_only = np.stack([b[0][n:n + n_first], b[1][n:n + n_first]], 1)
        self.second_only = np.stack([b[0][n + n_first:], b[2][n + n_first:]], 1)
        self.n, self.n_first, self.n_second = n, n_first, n_second
        pin = []
        for p in (self.first, self.second):
            q = p.copy()
            q[:, 3] /= np.linalg.norm(q[:, 3])
            if perturb:
                q[:, :3] = rodrigues(perturb * unit_vec(rng)) @ q[:, :3]
            pin.append(q)
        self.pose_in = np.stack(pin)

    def scene_arrays(self, cap, shuffle_seed=None):
        """keypoint blocks [3][cap] and index lists for the device call: block 0 centre, 1 first, 2 second"""
        m = len(self.points)
        assert m <= cap
        kps = np.zeros((3, cap), KP_DTYPE)
        for k in range(3):
            kps["x"][k, :m], kps["y"][k, :m] = self.px[k][:, 0], self.px[k][:, 1]
        idx = np.arange(self.n, dtype=np.uint32)
        if shuffle_seed is not None:
            idx = np.random.default_rng(shuffle_seed).permutation(self.n).astype(np.uint32)
        triples = np.zeros((cap, 3), np.uint32)
        triples[:self.n] = idx[:, None]
        fo, so = np.zeros((cap, 2), np.uint32), np.zeros((cap, 2), np.uint32)
        fo[:self.n_first] = (self.n + np.arange(self.n_first, dtype=np.uint32))[:, None]
        so[:self.n_second] = (self.n + self.n_first + np.arange(self.n_second, dtype=np.uint32))[:, None]
        return kps, triples, fo, so


def unit_vec(rng):
    v = rng.standard_normal(3)
    return v / np.linalg.norm(v)


def rig_camera():
    return camera(CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"])


def rig_camera_dev():
    """the same camera as the device call's rs_camera"""
    from cv_amd import _lib
    return _lib.Camera(CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"], 0.0, 0.0, 0, 0)
