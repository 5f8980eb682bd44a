"""An independent float64 numpy statement of cv-sfm's VSlam::filter_non_robust_observations (cv-sfm/src/lib.rs:2657-2757) and
what it calls: are_observations_robust (2907-2934), is_bi_landmark_robust (1306-1317) with epipolar::loss
(cv-geom/src/epipolar.rs:197-233), triangulate_landmark (2874-2892) over LinearEigenTriangulator
(cv-geom/src/triangulation.rs:82-130), split_landmark (2559-2568) and split_observation (552-588).  The point comes from
numpy.linalg.eigh; nothing here is shared with include/akz_observation_filter_math.h or its host build.  A landmark's
observations are walked in list order (the reference walks a HashMap)."""
import numpy as np

KEPT, SINGLE, PAIR_SPLIT, NO_POINT, KICKED, BAD_INDEX, SKIPPED = range(7)
OK, FEW_LANDMARKS, BAD_RANGE, RECON_SKIPPED = range(4)
NO_SOLVE = 255
TRI_OK, TRI_TOO_FEW, TRI_NOT_ROBUST, TRI_EIGEN, TRI_NOT_FINITE, TRI_CHEIRALITY, TRI_BAD_INDEX = range(7)


def settings(maximum_cosine_distance=1e-5, maximum_sine_distance=1e-1, minimum_robust_landmarks=32, robust_minimum_observations=3,
             incidence_minimum_cosine_distance=1e-3):
    """the reference's defaults (cv-sfm/src/settings.rs:324-350)"""
    return dict(max_cos=maximum_cosine_distance, max_sin=maximum_sine_distance, min_landmarks=minimum_robust_landmarks,
                min_obs=robust_minimum_observations, min_inc=incidence_minimum_cosine_distance)


def calibrate(cam, x, y):
    """CameraIntrinsics::calibrate (cv-pinhole/src/lib.rs:108-117) without distortion: cam = (fx, fy, cx, cy, skew)"""
    fx, fy, cx, cy, skew = cam
    yy = (np.float64(y) - cy) / fy
    xx = (np.float64(x) - cx - skew * yy) / fx
    v = np.array([xx, yy, 1.0])
    return v / np.linalg.norm(v)


def from_homogeneous(p):
    """Projective::from_homogeneous (cv-core/src/point.rs:20-25)"""
    p = np.array(p, np.float64)
    if np.signbit(p[3]):
        p = -p
    with np.errstate(all="ignore"):
        return p / np.linalg.norm(p[:3])


def are_observations_robust(obs, st, n_views):
    if len(obs) < min(st["min_obs"], n_views):
        return False
    world = [pose[:, :3].T @ b for pose, b in obs]
    return any(1.0 - float(world[i] @ world[j]) > st["min_inc"] for i in range(len(world)) for j in range(i + 1, len(world)))


def triangulate(obs):
    """(point [4] or None, reason)"""
    if len(obs) < 2:
        return None, TRI_TOO_FEW
    a = np.zeros((4, 4))
    for pose, b in obs:
        term = pose - np.outer(b, b) @ pose
        a += term.T @ term
    if not np.all(np.isfinite(a)):
        return None, TRI_NOT_FINITE
    w, v = np.linalg.eigh(a)
    p = from_homogeneous(v[:, int(np.argmin(w))])
    if not np.all(np.isfinite(p)):
        return None, TRI_NOT_FINITE
    for pose, b in obs:
        if np.signbit(float((pose[:, :3].T @ b) @ p[:3])):
            return None, TRI_CHEIRALITY
    return p, TRI_OK


def loss(t, a, b):
    """epipolar::loss"""
    with np.errstate(all="ignore"):
        ca, cb = np.cross(a, t), np.cross(b, t)
        can2, cbn2 = float(ca @ ca), float(cb @ cb)
        residual = abs(float(a @ (cb / np.sqrt(cbn2)))) if can2 < cbn2 else abs(float(b @ (ca / np.sqrt(can2))))
    if np.isnan(residual) or np.signbit(float(a @ b)):
        return 1.0
    return residual


def cosine_distance(pose, point, b):
    """1 - bearing(pose.transform(point)) . b (lib.rs:2721)"""
    q = np.append(pose[:, :3] @ point[:3] + pose[:, 3] * point[3], point[3])
    return 1.0 - float(from_homogeneous(q)[:3] @ b)


def filter_landmark(obs, st, n_views):
    """obs: list of (pose [3][4], bearing [3]) -> dict(keep, state, reason, before, after, dist): dist[i] the distance observation
    i was compared by (the loss at the second observation of a pair), None where none was."""
    n = len(obs)
    keep, dist = [True] * n, [None] * n
    before = are_observations_robust(obs, st, n_views)
    state, reason = KEPT, NO_SOLVE
    if n <= 1:
        state = SINGLE
    elif n == 2:
        (p0, b0), (p1, b1) = obs
        r = p1[:, :3] @ p0[:, :3].T
        t = p1[:, 3] - r @ p0[:, 3]
        dist[1] = loss(t, r @ b0, b1)
        if not dist[1] < st["max_sin"]:
            keep[1], state = False, PAIR_SPLIT
    else:
        point, reason = triangulate(obs)
        if point is None:
            keep, state = [True] + [False] * (n - 1), NO_POINT
        else:
            left = n
            for i, (pose, b) in enumerate(obs):
                dist[i] = cosine_distance(pose, point, b)
                if dist[i] > st["max_cos"] and left >= 2:        # split_observation refuses the last one
                    keep[i] = False
                    left -= 1
            state = KEPT if left == n else KICKED
    after = are_observations_robust([o for o, k in zip(obs, keep) if k], st, n_views)
    return dict(keep=keep, state=state, reason=reason, before=before, after=after, dist=dist)


def filter_table(kps, poses, cam, start, obs, recon_start, view_start, st, skip=None):
    """The whole call on a well-formed table (ascending starts, disjoint reconstructions): kps [blocks][cap] with fields x, y,
    poses [blocks][12], start / obs the CSR lists, -> dict of every output of rs_filter_observations_device plus dist [n_obs]
    (NaN where no distance was compared)."""
    n_blocks, cap = kps.shape
    n_lm, n_rec = len(start) - 1, len(recon_start) - 1
    keep = np.ones(len(obs), np.uint8)
    state = np.full(n_lm, SKIPPED, np.uint8)
    reason = np.full(n_lm, NO_SOLVE, np.uint8)
    robust = np.zeros(n_lm, np.uint8)
    dist = np.full(len(obs), np.nan)
    compared = np.zeros(len(obs), bool)
    verdict = np.zeros(n_rec, np.uint32)
    stats = np.zeros((n_rec, 8), np.uint32)
    for r in range(n_rec):
        lo, hi = int(recon_start[r]), int(recon_start[r + 1])
        stats[r, 0] = hi - lo
        if skip is not None and skip[r]:
            verdict[r] = RECON_SKIPPED
            continue
        n_views = int(view_start[r + 1]) - int(view_start[r])
        for l in range(lo, hi):
            rows = obs[int(start[l]):int(start[l + 1])]
            if any(b >= n_blocks or j >= cap for b, j in rows):
                state[l], reason[l] = BAD_INDEX, TRI_BAD_INDEX
                continue
            lst = [(poses[b].reshape(3, 4), calibrate(cam, kps[b, j]["x"], kps[b, j]["y"])) for b, j in rows]
            out = filter_landmark(lst, st, n_views)
            keep[int(start[l]):int(start[l + 1])] = out["keep"]
            for i, d in enumerate(out["dist"]):
                if d is not None:
                    dist[int(start[l]) + i], compared[int(start[l]) + i] = d, True
            state[l], reason[l] = out["state"], out["reason"]
            robust[l] = int(out["before"]) | int(out["after"]) << 1
            split = len(rows) - int(np.sum(out["keep"]))
            stats[r, 1:7] += np.array([out["before"], out["after"], split, out["state"] == PAIR_SPLIT, out["state"] == NO_POINT,
                                       out["state"] == KICKED], np.uint32)
        verdict[r] = FEW_LANDMARKS if stats[r, 2] < st["min_landmarks"] else OK
    k = keep.astype(bool)
    start_out = np.concatenate([[0], np.cumsum(k)])[np.asarray(start, np.int64)].astype(np.uint32)
    return dict(keep=keep, state=state, reason=reason, robust=robust, verdict=verdict, stats=stats, start_out=start_out,
                obs_out=obs[k], split_out=obs[~k], counts=np.array([k.sum(), (~k).sum()], np.uint32), dist=dist, compared=compared)
