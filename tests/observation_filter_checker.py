"""The CPU checker of the observation-filter kernels for the tests: tests/cpp/observation_filter_host.c (thin wrappers around
include/akz_observation_filter_math.h) as host_build.load compiles it — the host compiler, no contraction to FMA, as the
kernels — loaded with ctypes; plus the synthetic tables the test files use."""
import ctypes as C

import numpy as np

import host_build
import triangulate_checker as T

KEPT, SINGLE, PAIR_SPLIT, NO_POINT, KICKED, BAD_INDEX, SKIPPED = range(7)
OK, FEW_LANDMARKS, BAD_RANGE, RECON_SKIPPED = range(4)
STATS, NO_SOLVE = 8, 255
S_LANDMARKS, S_ROBUST_BEFORE, S_ROBUST_AFTER, S_OBS_SPLIT, S_PAIR_SPLIT, S_NO_POINT, S_KICKED = range(7)
FILL8, FILL32 = 0xA5, 0xA5A5A5A5
OR_STOPPED, OR_STAGE_RELAX, OR_STAGE_FILTER = 1 << 30, 1, 2
KP_DTYPE, Camera, camera = T.KP_DTYPE, T.Camera, T.camera


class Settings(C.Structure):
    """akz_of_settings (include/akz_observation_filter_math.h)."""
    _fields_ = [("maximum_cosine_distance", C.c_double), ("maximum_sine_distance", C.c_double),
                ("minimum_robust_landmarks", C.c_uint), ("tri", T.Settings)]


def settings(maximum_cosine_distance=1e-5, maximum_sine_distance=1e-1, minimum_robust_landmarks=32, n_views=0xFFFFFFFF, **tri):
    """The reference's defaults (cv-sfm/src/settings.rs:324-350) unless told otherwise; `tri`: triangulate_checker.settings'."""
    return Settings(maximum_cosine_distance, maximum_sine_distance, minimum_robust_landmarks, T.settings(n_views=n_views, **tri))


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    L = host_build.load("observation_filter_host.c")
    vp, u32 = C.c_void_p, C.c_uint32
    sp = C.POINTER(Settings)
    L.of_list.argtypes = [vp, vp, u32, sp, vp, vp]
    L.of_filter.argtypes = [vp, u32, u32, vp, C.POINTER(Camera), vp, vp, u32, u32, vp, vp, u32, vp, sp] + [vp] * 11
    L.of_note.argtypes = [vp, u32, u32, u32, u32, vp, vp]
    L.of_note.restype = None
    L.of_transformed_distance.argtypes = [vp, vp, vp]
    L.of_transformed_distance.restype = C.c_double
    L.of_verdict.argtypes = [u32, u32]
    L.of_triangulate.argtypes = [vp, vp, u32, C.POINTER(T.Settings), vp]
    _lib = L
    return L


def _a(x, dt=np.float64):
    return np.ascontiguousarray(x, dt)


def filter_list(poses, bearings, st=None):
    """One list through the header's function: poses [n][3][4], bearings [n][3] -> dict(state, keep, reason, robust, n_split)"""
    P, B = _a(poses).reshape(-1, 12), _a(bearings).reshape(-1, 3)
    assert len(P) == len(B)
    keep = np.full(max(len(P), 1), FILL8, np.uint8)
    out = np.zeros(3, np.uint32)
    st = st or settings()
    state = lib().of_list(P.ctypes.data, B.ctypes.data, len(P), C.byref(st), keep.ctypes.data, out.ctypes.data)
    return dict(state=state, keep=keep[:len(P)].copy(), reason=int(out[0]), robust=int(out[1]), n_split=int(out[2]))


def triangulate(poses, bearings, st=None):
    P, B = _a(poses).reshape(-1, 12), _a(bearings).reshape(-1, 3)
    out = np.empty(4)
    st = st or T.settings()
    why = lib().of_triangulate(P.ctypes.data, B.ctypes.data, len(P), C.byref(st), out.ctypes.data)
    return out, why


def transformed_distance(pose, point, b):
    p, x, b = _a(pose).reshape(12), _a(point).reshape(4), _a(b).reshape(3)
    return lib().of_transformed_distance(p.ctypes.data, x.ctypes.data, b.ctypes.data)


def filter_table(kps, poses, cam, start, obs, recon_start, view_start, st=None, skip=None, n_obs=None, distance=False):
    """rs_filter_observations_device on the host -> dict of every output array; what the call does not write keeps its fill
    (FILL8 / FILL32).  n_obs: the capacity handed to the call when it is not len(obs)."""
    kps = np.ascontiguousarray(kps)
    P = _a(poses).reshape(-1, 12)
    start, obs = _a(start, np.uint32), _a(obs, np.uint32).reshape(-1, 2)
    recon_start, view_start = _a(recon_start, np.uint32), _a(view_start, np.uint32)
    n_lm, n_rec = len(start) - 1, len(recon_start) - 1
    n_obs = len(obs) if n_obs is None else n_obs
    assert n_obs <= len(obs) or len(obs) == 0
    room = max(n_obs, 1)
    o = dict(keep=np.full(room, FILL8, np.uint8), state=np.full(max(n_lm, 1), FILL8, np.uint8), reason=np.full(max(n_lm, 1), FILL8, np.uint8),
             robust=np.full(max(n_lm, 1), FILL8, np.uint8), start_out=np.full(n_lm + 1, FILL32, np.uint32),
             obs_out=np.full((room, 2), FILL32, np.uint32), split_out=np.full((room, 2), FILL32, np.uint32),
             counts=np.full(2, FILL32, np.uint32), verdict=np.full(max(n_rec, 1), FILL32, np.uint32),
             stats=np.full((max(n_rec, 1), STATS), FILL32, np.uint32))
    dist = np.empty(room) if distance else None
    skip_a = None if skip is None else _a(skip, np.uint32)
    obs_in = obs if len(obs) else np.zeros((1, 2), np.uint32)
    st = st or settings()
    r = lib().of_filter(kps.ctypes.data, kps.shape[1], kps.shape[0], P.ctypes.data, C.byref(cam), start.ctypes.data, obs_in.ctypes.data, n_obs,
                        n_lm, recon_start.ctypes.data, view_start.ctypes.data, n_rec, None if skip_a is None else skip_a.ctypes.data,
                        C.byref(st), o["keep"].ctypes.data, o["state"].ctypes.data, o["reason"].ctypes.data, o["robust"].ctypes.data,
                        o["start_out"].ctypes.data, o["obs_out"].ctypes.data, o["split_out"].ctypes.data, o["counts"].ctypes.data,
                        o["verdict"].ctypes.data, o["stats"].ctypes.data, None if dist is None else dist.ctypes.data)
    assert r == 0
    if distance:
        o["dist"] = dist
    return o


def note(stage_verdict, ok, round_, stage, stop, verdict):
    """k_or_note on the host: stop and verdict are updated in place"""
    sv = _a(stage_verdict, np.uint32)
    lib().of_note(sv.ctypes.data, ok, round_, stage, len(sv), stop.ctypes.data, verdict.ctypes.data)


# ---- synthetic tables ---------------------------------------------------------------------------------------------
def scene(seed, n_views=12, n_landmarks=4000, lengths=(3, 8), noise=0.5, outlier_fraction=0.3, displacement=(40.0, 120.0), f=1000.0,
          cx=960.0, cy=540.0, long_lists=0):
    """n_views cameras, n_landmarks points 2 to 10 units deep, each observed by lengths[0] .. lengths[1] views chosen at random
    (list lengths mixed at random, so every wave holds all of them; `long_lists` of them 33 to 48 long), every observation the
    projection + uniform pixel noise; in outlier_fraction of the landmarks of 2 or more ONE observation is displaced by
    displacement[0] .. displacement[1] px in a random direction.  -> dict(kps, poses [n_views][12], cam, start, obs)."""
    rng = np.random.default_rng(seed)
    poses = T.random_poses(rng, n_views)
    lens = rng.integers(lengths[0], lengths[1] + 1, n_landmarks)
    if long_lists:
        lens[rng.choice(n_landmarks, long_lists, replace=False)] = rng.integers(33, min(n_views, 48) + 1, long_lists)
    lens = np.minimum(lens, n_views)
    cap = max(int(n_landmarks), 1)
    kps = np.zeros((n_views, cap), KP_DTYPE)
    used = np.zeros(n_views, np.int64)
    pts = np.stack([rng.uniform(-2, 2, n_landmarks), rng.uniform(-1.5, 1.5, n_landmarks), rng.uniform(2, 10, n_landmarks)], 1)
    start, obs = [0], []
    for l in range(n_landmarks):
        views = rng.permutation(n_views)[:lens[l]]
        bad = rng.integers(0, len(views)) if len(views) >= 2 and rng.random() < outlier_fraction else -1
        for k, b in enumerate(views):
            x, y = T.project(poses[b], pts[l], f, cx, cy)
            x, y = x + rng.uniform(-noise, noise), y + rng.uniform(-noise, noise)
            if k == bad:
                ang, d = rng.uniform(0, 2 * np.pi), rng.uniform(*displacement)
                x, y = x + d * np.cos(ang), y + d * np.sin(ang)
            j = used[b]
            used[b] += 1
            kps[b, j]["x"], kps[b, j]["y"] = x, y
            obs.append((b, j))
        start.append(len(obs))
    return dict(kps=kps, poses=poses.reshape(n_views, 12), cam=camera(f, f, cx, cy), cam5=(f, f, cx, cy, 0.0),
                start=np.array(start, np.uint32), obs=np.array(obs, np.uint32).reshape(-1, 2), points=pts)
