"""The CPU checker of the single-view refinement kernel for the tests: tests/cpp/single_view_host.c (thin wrappers around
include/akz_single_view_math.h) as host_build.load compiles it — the host compiler, no contraction to FMA, as the kernel —
loaded with ctypes; plus the synthetic rigs the test files use."""
import ctypes as C

import numpy as np

import host_build
from three_view_checker import CAM, bearings_of, camera_to_camera, project, rig_camera, rig_camera_dev, rodrigues, unit_vec  # noqa: F401
from triangulate_checker import KP_DTYPE, Camera
from triangulate_checker import Settings as TriSettings

STATS = 24
S_INLIERS, S_RUN_MATCHES, S_RUN_STOP, S_ROBUST, S_NO_OTHER, S_STAGE = 0, 1, 10, 19, 20, 21
OK, NO_MODEL, FEW_LANDMARKS, LOST_HALF, FEW_ROBUST, BAD_INDEX = range(6)
STAGE_INDEX, STAGE_LANDMARKS, STAGE_MODEL, STAGE_RUN0, STAGE_FINAL, STAGE_MINIMUM = 0, 1, 2, 3, 12, 13
MAX_MATCHES = 2048
NONE_ROW = np.array([0.0, 0.0, 0.0, -1.0])
NO_ID = 0xFFFFFFFF


class Settings(C.Structure):
    """akz_sv_settings (include/akz_single_view_math.h)."""
    _fields_ = [("maximum_cosine_distance", C.c_double), ("maximum_sine_distance", C.c_double),
                ("single_view_optimization_rate", C.c_double), ("single_view_optimization_num_matches", C.c_uint),
                ("single_view_filter_loop_iterations", C.c_uint), ("single_view_patience", C.c_uint),
                ("single_view_minimum_landmarks", C.c_uint), ("single_view_minimum_robust_landmarks", C.c_uint), ("tri", TriSettings)]


def settings(**kw):
    """The reference's defaults (cv-sfm/src/settings.rs:324-383) with `kw` on top."""
    st = Settings(1e-5, 1e-1, 1e-3, 2048, 5, 100000, 32, 64, TriSettings(1e-12, 1000, 3, 0xFFFFFFFF, 1e-3))
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
    L = host_build.load("single_view_host.c")
    vp, u32, dbl = C.c_void_p, C.c_uint32, C.c_double
    sp, cp = C.POINTER(Settings), C.POINTER(Camera)
    L.sv_world_pose_gradient.argtypes = [vp, vp, vp]
    L.sv_world_pose_gradient.restype = None
    L.sv_landmark_delta.argtypes = [vp] * 4
    L.sv_point.argtypes = [vp, vp]
    L.sv_point.restype = None
    L.sv_sum.argtypes = [vp, vp, u32, C.c_int, vp]
    L.sv_optimize.argtypes = [vp, dbl, u32, vp, u32, C.c_int]
    L.sv_optimize.restype = u32
    L.sv_consistent.argtypes = [u32, vp, vp, vp, vp, vp, u32, vp, sp]
    L.sv_refine.argtypes = [u32, vp, vp, vp, vp, vp, vp, C.c_int, vp, u32, sp, C.c_int, vp, vp, vp, vp]
    L.sv_refine_scene.argtypes = [vp, u32, u32, vp, cp, vp, vp, u32, u32, vp, u32, u32, u32, vp, u32, vp, vp, u32, vp, u32, sp, vp, vp, vp, vp]
    L.sv_consistency_values.argtypes = [u32, vp, vp, vp, vp, vp, u32, vp, sp, vp, u32]
    L.sv_consistency_values.restype = u32
    _lib = L
    return L


def _a(x, dt=np.float64):
    return np.ascontiguousarray(x, dt)


def _p(a):
    return a.ctypes.data


def world_pose_gradient(t, b):
    t, b, g = _a(t), _a(b), np.empty(6)
    lib().sv_world_pose_gradient(_p(t), _p(b), _p(g))
    return g


def landmark_delta(pose, b, x):
    """(1, g [6]) or (0, None): x the Euclidean world point"""
    pose, b, x, g = _a(pose).reshape(12), _a(b), _a(x), np.empty(6)
    ok = lib().sv_landmark_delta(_p(pose), _p(b), _p(x), _p(g))
    return ok, (g if ok else None)


def euclidean(world):
    w, x = _a(world).reshape(4), np.empty(3)
    lib().sv_point(_p(w), _p(x))
    return x


def gradient_sum(pose, landmarks, sequential=False):
    """the summed gradient [6] of landmarks [n][6] = (bearing, Euclidean point)"""
    pose, lm, net = _a(pose).reshape(12), _a(landmarks).reshape(-1, 6), np.empty(6)
    assert lib().sv_sum(_p(pose), _p(lm), len(lm), int(sequential), _p(net)) == 0
    return net


def optimize(pose, rate, iterations, landmarks, sequential=False):
    """-> (pose [3][4], stopping iteration); landmarks [n][6] = (bearing, Euclidean point)."""
    p = _a(pose).reshape(12).copy()
    lm = _a(landmarks).reshape(-1, 6)
    it = lib().sv_optimize(_p(p), rate, iterations, _p(lm), len(lm), int(sequential))
    assert it != 0xFFFFFFFF
    return p.reshape(3, 4), it


class Scene:
    """A scene as arrays: bearing [n][3], world [n][4] (w < 0: None), obs_start [n + 1], obs_pose [m][3][4], obs_bearing [m][3]"""

    def __init__(self, bearing, world, obs_start, obs_pose, obs_bearing):
        self.bearing, self.world = _a(bearing).reshape(-1, 3), _a(world).reshape(-1, 4)
        self.obs_start = _a(obs_start, np.uint32)
        self.obs_pose, self.obs_bearing = _a(obs_pose).reshape(-1, 12), _a(obs_bearing).reshape(-1, 3)
        self.n = len(self.bearing)
        assert len(self.world) == self.n and len(self.obs_start) == self.n + 1 and self.obs_start[-1] == len(self.obs_pose) == len(self.obs_bearing)
        if len(self.obs_pose) == 0:
            self.obs_pose, self.obs_bearing = np.zeros((1, 12)), np.zeros((1, 3))

    def args(self):
        return (self.n, _p(self.bearing), _p(self.world), _p(self.obs_start), _p(self.obs_pose), _p(self.obs_bearing))


def consistent(scene, i, pose, st):
    pose = _a(pose).reshape(12)
    return bool(lib().sv_consistent(*scene.args(), i, _p(pose), C.byref(st)))


def consistency_values(scene, i, pose, st):
    """the values is_observation_consistent compares for match i under `pose`, as the host build computes them"""
    pose, out = _a(pose).reshape(12), np.empty(64)
    m = lib().sv_consistency_values(*scene.args(), i, _p(pose), C.byref(st), _p(out), len(out))
    return out[:m].copy()


def _result(v, n, pose_out, final, n_final, stats):
    return dict(verdict=v, pose=pose_out.reshape(3, 4), final=final[:n].astype(bool), n_final=int(n_final[0]), stats=stats,
                stage=int(stats[S_STAGE]), robust=int(stats[S_ROBUST]), run_matches=stats[S_RUN_MATCHES:S_RUN_MATCHES + 9].copy(),
                run_stop=stats[S_RUN_STOP:S_RUN_STOP + 9].copy())


def refine(scene, pose_in, inliers, st, has_model=True, sequential=False):
    """the host build on a Scene"""
    pose_in, inl = _a(pose_in).reshape(12), _a(inliers, np.uint32).reshape(-1)
    pose_out, final, n_final, stats = np.full(12, np.nan), np.full(max(1, scene.n), 255, np.uint8), np.zeros(1, np.uint32), np.zeros(STATS, np.uint32)
    inl_p = _p(inl) if len(inl) else None
    v = lib().sv_refine(*scene.args(), _p(pose_in), int(has_model), inl_p, len(inl), C.byref(st), int(sequential), _p(pose_out), _p(final),
                        _p(n_final), _p(stats))
    assert v >= 0
    return _result(v, scene.n, pose_out, final, n_final, stats)


def refine_scene(b, s, st, prior):
    """the host build on scene s of a Batch (the device call's inputs); `prior` = (pose_out [12], final [cap]) what the outputs
    held before (left as is where not written) -> dict(verdict, pose_out, final, n_final, stats)"""
    pose_out, final = (np.array(x, copy=True) for x in prior)
    n_final, stats = np.zeros(1, np.uint32), np.zeros(STATS, np.uint32)
    cam = rig_camera()
    best = None if b.best is None else _p(b.best)
    v = lib().sv_refine_scene(_p(b.kps), b.cap, b.n_blocks, _p(b.poses), C.byref(cam), _p(b.obs_start), _p(b.obs), b.n_obs, b.n_landmarks,
                              _p(b.world), b.n_world, b.n_rows, int(b.ik[s]), _p(b.matches[s]), int(b.nmatches[s]), best, _p(b.pose[s]),
                              int(b.best_id[s]), _p(b.inliers[s]), int(b.n_inliers[s]), C.byref(st), _p(pose_out), _p(final), _p(n_final),
                              _p(stats))
    assert v >= 0
    return dict(verdict=v, pose_out=pose_out, final=final, n_final=int(n_final[0]), stats=stats)


# ---- synthetic rigs ----
def world_to_camera(position, axis_angle):
    return camera_to_camera(position, axis_angle)


def homogeneous(points):
    """Projective::from_point: xyz normalised, w = 1 / distance"""
    d = np.linalg.norm(points, axis=1, keepdims=True)
    return np.hstack([points / d, 1.0 / d])


class Rig:
    """n original matches of a new frame against a map of `n_views` views looking at points 4 - 10 units deep.

    obs_counts [n]: the other observations of each match's landmark (default 2 .. 5, cycling); merged: indices of matches that
    are merged matches (their observations split over two landmarks, the second with `merged_second` observations);
    none: indices whose world row says "None"; outliers: indices whose pixel in the new frame is 20 - 40 px off;
    noise: pixel noise (px at f = 1000) on every observation; perturb: the consensus' pose = the true one turned by `perturb`
    rad and moved by `perturb` units; inliers: what the consensus reports (default: every match with a world point)."""

    def __init__(self, seed, n, n_views=12, obs_counts=None, merged=(), merged_second=2, none=(), outliers=(), noise=0.0, perturb=1e-3,
                 inliers=None, has_model=True):
        rng = np.random.default_rng(seed)
        self.n, self.n_views = n, n_views
        self.view_poses = np.stack([world_to_camera([0.25 * v - 0.125 * n_views, 0.1 * np.sin(v), 0.05 * np.cos(2.0 * v)],
                                                    [0.01 * np.sin(3.0 * v), 0.02 * np.cos(v), 0.005 * v]) for v in range(n_views)])
        self.true_pose = world_to_camera([0.33, -0.21, 0.4], [0.03, -0.05, 0.02])
        z = rng.uniform(4.0, 10.0, n)
        self.points = np.stack([rng.uniform(-0.3, 0.3, n) * z, rng.uniform(-0.2, 0.2, n) * z, z], 1)
        counts = np.asarray(obs_counts if obs_counts is not None else 2 + np.arange(n) % 4, np.int64)
        assert len(counts) == n
        self.merged = np.zeros(n, bool)
        self.merged[list(merged)] = True
        self.none = np.zeros(n, bool)
        self.none[list(none)] = True
        # landmarks: match i owns landmark i; a merged match owns landmark n + (its rank among the merged) as well
        second = np.full(n, -1, np.int64)
        second[self.merged] = n + np.arange(int(self.merged.sum()))
        self.second = second
        self.n_landmarks = n + int(self.merged.sum())
        lm_point = np.concatenate([np.arange(n), np.flatnonzero(self.merged)])
        lm_count = np.concatenate([counts, np.full(int(self.merged.sum()), merged_second, np.int64)])
        # observations {view, feature}: landmark l's k-th observation is in view (l + k) mod n_views, feature = next free one
        next_feat = np.zeros(n_views, np.int64)
        self.obs_start = np.zeros(self.n_landmarks + 1, np.uint32)
        obs, px = [], []
        for l in range(self.n_landmarks):
            for k in range(int(lm_count[l])):
                v = (l + k) % n_views
                obs.append((v, next_feat[v]))
                px.append(project(self.view_poses[v], self.points[lm_point[l]][None])[0] + noise * rng.standard_normal(2))
                next_feat[v] += 1
            self.obs_start[l + 1] = len(obs)
        self.obs = np.array(obs, np.uint32).reshape(-1, 2)
        self.obs_px = np.array(px, np.float64).reshape(-1, 2)
        self.view_features = int(next_feat.max()) if n_views else 0
        new_px = project(self.true_pose, self.points) + noise * rng.standard_normal((n, 2))
        for k in outliers:
            new_px[k] += rng.choice([-1.0, 1.0], 2) * rng.uniform(20.0, 40.0, 2)
        self.new_px = np.asarray(new_px, np.float32)
        self.world = homogeneous(self.points)
        self.world[self.none] = NONE_ROW
        q = self.true_pose.copy()
        if perturb:
            dr = rodrigues(perturb * unit_vec(rng))
            q = np.hstack([dr @ q[:, :3], (dr @ q[:, 3] + perturb * unit_vec(rng))[:, None]])
        self.pose_in = q
        self.has_model = has_model
        n_rob = int((~self.none).sum())
        self.inliers = np.arange(n_rob, dtype=np.uint32) if inliers is None else np.asarray(inliers, np.uint32)

    def scene(self):
        """the Scene of arrays (bearings from the f32 pixels, as the device computes them)"""
        ob = bearings_of(np.asarray(self.obs_px, np.float32))
        op = self.view_poses[self.obs[:, 0]] if len(self.obs) else np.zeros((0, 3, 4))
        start, poses, bear = [0], [], []
        for i in range(self.n):
            for l in ([i] if not self.merged[i] else [i, int(self.second[i])]):
                s, e = int(self.obs_start[l]), int(self.obs_start[l + 1])
                poses.extend(op[s:e])
                bear.extend(ob[s:e])
            start.append(len(poses))
        return Scene(bearings_of(self.new_px), self.world, start, np.array(poses).reshape(-1, 12), np.array(bear).reshape(-1, 3))

    def pose_error(self, pose):
        """(rotation angle, translation distance) between `pose` and the true pose"""
        pose = np.asarray(pose).reshape(3, 4)
        r = pose[:, :3] @ self.true_pose[:, :3].T
        return float(np.arccos(np.clip((np.trace(r) - 1.0) / 2.0, -1.0, 1.0))), float(np.linalg.norm(pose[:, 3] - self.true_pose[:, 3]))


class Batch:
    """Rigs side by side as rs_refine_poses_batch_device takes them: rig s owns blocks [s (V + 1), (s + 1)(V + 1)) — its views,
    then its new frame —, its landmarks and its observations; the world table's rows [0, n_world) are the landmarks', the
    merged matches' rows follow at n_world + s * cap + feature."""

    def __init__(self, rigs, cap):
        self.rigs, self.cap, S = rigs, cap, len(rigs)
        self.n_blocks = sum(r.n_views + 1 for r in rigs)
        self.kps = np.zeros((self.n_blocks, cap), KP_DTYPE)
        self.poses = np.zeros((self.n_blocks, 12))
        self.n_landmarks = self.n_world = sum(r.n_landmarks for r in rigs)
        any_merged = any(r.merged.any() for r in rigs)
        self.n_rows = self.n_world + (S * cap if any_merged else 0)
        self.world = np.tile(NONE_ROW, (max(1, self.n_rows), 1))
        self.best = np.full((S, cap, 3, 2), NO_ID, np.uint32) if any_merged else None
        self.matches = np.zeros((S, cap, 2), np.uint32)
        self.nmatches = np.zeros(S, np.uint32)
        self.ik = np.zeros(S, np.uint32)
        self.pose = np.zeros((S, 12))
        self.best_id = np.zeros(S, np.uint32)
        self.inliers = np.zeros((S, cap), np.uint32)
        self.n_inliers = np.zeros(S, np.uint32)
        starts, obs = [np.zeros(1, np.uint32)], []
        b0 = l0 = o0 = 0
        for s, r in enumerate(rigs):
            assert r.n <= cap and r.view_features <= cap
            for k in range(len(r.obs)):
                v, f = r.obs[k]
                self.kps["x"][b0 + v, f], self.kps["y"][b0 + v, f] = np.float32(r.obs_px[k, 0]), np.float32(r.obs_px[k, 1])
            self.poses[b0:b0 + r.n_views] = r.view_poses.reshape(-1, 12)
            self.ik[s] = b0 + r.n_views
            self.kps["x"][self.ik[s], :r.n], self.kps["y"][self.ik[s], :r.n] = r.new_px[:, 0], r.new_px[:, 1]
            o = r.obs.copy()
            o[:, 0] += b0
            obs.append(o)
            starts.append(r.obs_start[1:] + o0)
            for i in range(r.n):
                if r.merged[i]:
                    row = self.n_world + s * cap + i
                    self.best[s, i, 0, 0], self.best[s, i, 1, 0] = l0 + i, l0 + int(r.second[i])
                else:
                    row = l0 + i
                self.world[row] = r.world[i]
                self.matches[s, i] = (i, row)
            self.nmatches[s] = r.n
            self.pose[s] = r.pose_in.reshape(12)
            self.best_id[s] = 0 if r.has_model else NO_ID
            self.inliers[s, :len(r.inliers)] = r.inliers
            self.n_inliers[s] = len(r.inliers)
            b0, l0, o0 = b0 + r.n_views + 1, l0 + r.n_landmarks, o0 + len(r.obs)
        self.obs_start = np.concatenate(starts).astype(np.uint32)
        self.obs = np.concatenate(obs).astype(np.uint32).reshape(-1, 2) if o0 else np.zeros((1, 2), np.uint32)
        self.n_obs = o0

    def host(self, st, prior_pose, prior_final):
        """the host build on every scene -> the five output buffers as the device call leaves them"""
        S = len(self.rigs)
        pose_out, final = np.array(prior_pose, copy=True), np.array(prior_final, copy=True)
        verdict, n_final, stats = np.zeros(S, np.uint32), np.zeros(S, np.uint32), np.zeros((S, STATS), np.uint32)
        for s in range(S):
            r = refine_scene(self, s, st, (pose_out[s], final[s]))
            pose_out[s], final[s], verdict[s], n_final[s], stats[s] = r["pose_out"], r["final"], r["verdict"], r["n_final"], r["stats"]
        return dict(pose_out=pose_out, verdict=verdict, final=final, n_final=n_final, stats=stats)
