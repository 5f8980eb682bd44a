"""The triangulation stage (rs_triangulate_observations, rs_triangulate_landmarks_device, rs_triangulate_merged_device,
rs_triangulate_pairs_batch_device) in plain numpy / LAPACK float64, written from the reference's definitions and from the text
of include/akz.h, and a catalogue of designed inputs on which its rules decide.

Nothing here imports the product, the C oracle or a host build, compiles a header or reads a kernel.  What is stated
(paths relative to rust-cv/cv):

  calibrate        CameraIntrinsics::calibrate and the K1 variant (cv-pinhole/src/lib.rs:108-117, 191-202): the keypoint's
                   float32 pixel widened to float64, the principal point removed, y / fy, (x - skew y) / fx, with K1 both
                   divided by 1 + k1 r^2, the unit bearing.
  triangulate      LinearEigenTriangulator::triangulate_observations (cv-geom/src/triangulation.rs:82-130): the design matrix
                   sum (P - b b^T P)^T (P - b b^T P), numpy.linalg.eigh, the eigenvector of the signed-smallest eigenvalue,
                   Projective::from_homogeneous (cv-core/src/point.rs:20-25: negated when w's sign bit is set, divided by
                   |xyz|), the finite filter, the cheirality test (R^T b) . xyz sign-positive for EVERY observation.
  robust           VSlam::are_observations_robust (cv-sfm/src/lib.rs:2895-2934): n >= min(robust_minimum_observations,
                   n_views) and SOME pair i < j with 1 - (R_i^T b_i) . (R_j^T b_j) > incidence_minimum_cosine_distance,
                   stated as the maximum over all pairs (a NaN distance passes no '>': it takes no part in the maximum).
  landmarks, merged, pairs, observations
                   the three table forms and the single list as include/akz.h documents them: row addresses, the rows left
                   untouched, the "None" row {0, 0, 0, -1}, the reason byte with the precedence 6, 1, 2, 4 / 3, 5, the merged
                   list obs(best0) ++ obs(best1), the clamps of n_inliers / npairs to cap_per_img, "a scene without a model
                   writes nothing", reason 6 for whatever names something outside the caller's arrays.

The eigen-solver is LAPACK's, so a sweep limit has no meaning here but one: akz.h counts max_sweeps in tests of the cyclic
Jacobi iteration's stopping rule (off-diagonal norm <= eps * diagonal norm), so with max_sweeps == 1 a design matrix that does
not meet the rule as it stands ends with reason 3; any limit of 30 and more is ample for a 4 x 4 problem (akz.h: "needs < 20")
and is taken as no limit.  Other limits are refused.

Every row comes with the margins of its decisions: the best pair distance, the smallest |cheirality dot product|, LAPACK's
eigenvalues.  Three conditions are asserted on EVERY case wherever a case runs (`hold`; no case is excused):
  |best pair distance - threshold| >= 1e-12 (absolute: 1 - cos carries ~1e-16 whatever the distance),
  |cheirality dot| >= 1e-9 on every row that reaches that test,
  (l2 - l1) / l4 >= 1e-6 on every row that reaches the solver.
Points are compared as unit 4-vectors: sin(angle) <= (1e-12 + 16 n 2^-53) l4 / (l2 - l1) — the solver's stopping rule
(eps = 1e-12) through Davis-Kahan, plus the rounding of an n-term accumulation.

ALTERATIONS are named wrong rules the statement can be switched to; the tests show that each is caught by the catalogue.
"""
import math
from dataclasses import dataclass, field

import numpy as np

OK, TOO_FEW, NOT_ROBUST, EIGEN, NOT_FINITE, CHEIRALITY, BAD_INDEX = range(7)
NONE_ROW = np.array([0.0, 0.0, 0.0, -1.0])
NO_ID = 0xFFFFFFFF
ALTERATIONS = ("pairs_with_first_only", "need_ignores_n_views", "camera_axes_bearing", "cheirality_first_only", "w_sign_kept",
               "k1_ignored", "skew_ignored", "merged_first_only")
THRESHOLD_GUARD, DOT_GUARD, GAP_GUARD = 1e-12, 1e-9, 1e-6


@dataclass(frozen=True)
class Settings:
    """rs_triangulate_params without its size field."""
    eps: float = 1e-12
    max_sweeps: int = 1000
    robust_minimum_observations: int = 3
    n_views: int = 0xFFFFFFFF
    min_cos: float = 1e-3


# ------------------------------------------------------------------------------------------------ the rules
def calibrate(x, y, cam, alter=()):
    """pixel(s) -> unit bearing(s) [.., 3]; cam = (fx, fy, cx, cy, skew, k1 or None)"""
    fx, fy, cx, cy, skew, k1 = cam
    x = np.asarray(x, np.float32).astype(np.float64) - cx
    y = np.asarray(y, np.float32).astype(np.float64) - cy
    yn = y / fy
    xn = (x - (0.0 if "skew_ignored" in alter else skew) * yn) / fx
    if k1 is not None and "k1_ignored" not in alter:
        d = 1.0 + k1 * (xn * xn + yn * yn)
        xn, yn = xn / d, yn / d
    v = np.stack([xn, yn, np.ones_like(xn)], -1)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def world_bearings(poses, bearings, alter=()):
    """pose.inverse().isometry() * bearing: R^T b, [n, 3]"""
    R = poses[:, :, :3]
    with np.errstate(invalid="ignore"):
        if "camera_axes_bearing" in alter:
            return np.einsum("nij,nj->ni", R, bearings)
        return np.einsum("nji,nj->ni", R, bearings)


def best_pair_distance(poses, bearings, alter=()):
    """max over the pairs i < j of 1 - (R_i^T b_i) . (R_j^T b_j); -inf where no pair has a distance that is a number"""
    n = len(poses)
    if n < 2:
        return -math.inf
    d = world_bearings(poses, bearings, alter)
    with np.errstate(invalid="ignore"):
        dist = 1.0 - d @ d.T
    vals = dist[0, 1:] if "pairs_with_first_only" in alter else dist[np.triu_indices(n, 1)]
    vals = vals[~np.isnan(vals)]
    return float(vals.max()) if len(vals) else -math.inf


def need_of(st, alter=()):
    return st.robust_minimum_observations if "need_ignores_n_views" in alter else min(st.robust_minimum_observations, st.n_views)


def robust_verdict(n, best, st, alter=()):
    """are_observations_robust from the list's length and its best pair distance"""
    return n >= need_of(st, alter) and best > st.min_cos


def robust(poses, bearings, st, alter=()):
    """are_observations_robust -> (verdict, the best pair distance)"""
    best = best_pair_distance(poses, bearings, alter)
    return robust_verdict(len(poses), best, st, alter), best


def design_matrix(poses, bearings):
    A = np.zeros((4, 4))
    for P, b in zip(poses, bearings):
        term = P - np.outer(b, b) @ P
        A = A + term.T @ term
    return A


@dataclass
class Prepared:
    """What one list decides with, whatever the settings: everything but the comparisons with them."""
    n: int
    bad: bool = False
    best: float = -math.inf
    finite: bool = False            # the design matrix
    off: float = 0.0                # squared norms of its off-diagonal (upper triangle) and its diagonal
    diag: float = 0.0
    lam: np.ndarray = None
    point: np.ndarray = None        # after from_homogeneous
    point_finite: bool = False
    dots: np.ndarray = None         # the cheirality products the rule looks at


def prepare(poses, bearings, alter=(), bad=False):
    n = len(poses)
    if bad or n < 2:
        return Prepared(n, bad)
    pre = Prepared(n, False, best_pair_distance(poses, bearings, alter))
    A = design_matrix(poses, bearings)
    pre.finite = bool(np.isfinite(A).all())
    if not pre.finite:
        return pre
    pre.off, pre.diag = float((A[np.triu_indices(4, 1)] ** 2).sum()), float((np.diag(A) ** 2).sum())
    pre.lam, vec = np.linalg.eigh(A)
    v = vec[:, 0]                                          # eigh: ascending, so the signed-smallest eigenvalue's
    if np.signbit(v[3]) and "w_sign_kept" not in alter:
        v = -v
    with np.errstate(divide="ignore", invalid="ignore"):
        pre.point = v / np.linalg.norm(v[:3])
    pre.point_finite = bool(np.isfinite(pre.point).all())
    if pre.point_finite:
        dots = world_bearings(poses, bearings, alter) @ pre.point[:3]          # xyz is a unit vector: the point's bearing
        pre.dots = dots[:1] if "cheirality_first_only" in alter else dots
    return pre


@dataclass
class Row:
    reason: int
    point: np.ndarray
    n: int
    best: float = -math.inf          # the best pair distance (-inf: none)
    min_dot: float = math.inf        # the smallest |cheirality product|, where the row reached that test
    lam: np.ndarray = None           # LAPACK's eigenvalues, where the row reached the solver
    robust_asked: bool = False

    @property
    def gap(self):
        return (self.lam[1] - self.lam[0]) / self.lam[3]

    @property
    def bound(self):
        return (1e-12 + 16.0 * self.n * 2.0 ** -53) * self.lam[3] / (self.lam[1] - self.lam[0])


def decide(pre, want_robust, st, alter=()):
    """One list -> its Row.  Precedence: 6, 1, 2, then 4 / 3 / 4 around the solver, 5."""
    assert st.max_sweeps == 1 or st.max_sweeps >= 30, "the statement knows a sweep limit of 1 and ample ones"
    row = Row(OK, NONE_ROW, pre.n, pre.best, robust_asked=want_robust)
    if pre.bad:
        row.reason = BAD_INDEX
    elif pre.n < 2:
        row.reason = TOO_FEW
    elif want_robust and not robust_verdict(pre.n, pre.best, st, alter):
        row.reason = NOT_ROBUST
    elif not pre.finite:
        row.reason = NOT_FINITE
    elif st.max_sweeps == 1 and not (pre.off <= st.eps * st.eps * pre.diag or pre.off == 0.0):
        row.reason = EIGEN
    else:
        row.lam = pre.lam
        if not pre.point_finite:
            row.reason = NOT_FINITE
        else:
            row.min_dot = float(np.abs(pre.dots).min())
            if np.signbit(pre.dots).any():
                row.reason = CHEIRALITY
            else:
                row.point = pre.point
    return row


def triangulate(poses, bearings, st=Settings(), alter=(), want_robust=False):
    """LinearEigenTriangulator::triangulate_observations on poses [n, 3, 4] and unit bearings [n, 3] -> the Row: reason, point
    ("None": {0, 0, 0, -1}) and margins; want_robust: are_observations_robust first, as the table forms ask"""
    poses = np.asarray(poses, np.float64).reshape(-1, 3, 4)
    bearings = np.asarray(bearings, np.float64).reshape(-1, 3)
    return decide(prepare(poses, bearings, alter), want_robust, st, alter)


observations = triangulate       # rs_triangulate_observations: one list, the robustness test not applied


# ------------------------------------------------------------------------------------------------ the table forms
@dataclass
class Table:
    """The arguments of rs_triangulate_landmarks_device.  xy [n_blocks, cap, 2] float32: the keypoints' pixels; n_obs: the
    length of the observation array the CALL states (obs itself may be longer: what lies behind n_obs is never read)."""
    cap: int
    cam: tuple
    xy: np.ndarray
    poses: np.ndarray                # [n_blocks, 12]
    start: np.ndarray                # [n_landmarks + 1] uint32
    obs: np.ndarray                  # [.., 2] uint32 {block, feature}
    n_obs: int
    tags: dict = field(default_factory=dict)     # name -> landmarks designed for it

    @property
    def n_landmarks(self):
        return len(self.start) - 1

    @property
    def n_blocks(self):
        return len(self.poses)


def _range(t, l):
    """landmark l's rows of obs, or None where the range does not lie inside [0, n_obs]"""
    a, b = int(t.start[l]), int(t.start[l + 1])
    return t.obs[a:b] if a <= b <= t.n_obs else None


def _fetch(t, rows, alter=()):
    """{block, feature} rows -> (bad, poses [n, 3, 4], bearings [n, 3])"""
    rows = np.asarray(rows, np.int64).reshape(-1, 2)
    if len(rows) and ((rows[:, 0] >= t.n_blocks).any() or (rows[:, 1] >= t.cap).any()):
        return True, None, None
    px = t.xy[rows[:, 0], rows[:, 1]]
    return False, t.poses[rows[:, 0]].reshape(-1, 3, 4), calibrate(px[:, 0], px[:, 1], t.cam, alter).reshape(-1, 3)


def _prepare_rows(t, rows, alter):
    if rows is None:
        return Prepared(0, True)
    bad, P, B = _fetch(t, rows, alter)
    return Prepared(len(rows), True) if bad else prepare(P, B, alter)


def prepare_landmarks(t, alter=()):
    return [_prepare_rows(t, _range(t, l), alter) for l in range(t.n_landmarks)]


def landmarks(t, st=Settings(), alter=(), n_landmarks=None, prepared=None):
    """Row l of the world table for l < n_landmarks (a prefix of the table where given); no other row is written."""
    prepared = prepared if prepared is not None else prepare_landmarks(t, alter)
    n = t.n_landmarks if n_landmarks is None else n_landmarks
    return [decide(prepared[l], True, st, alter) for l in range(n)]


@dataclass
class MergeCase:
    table: Table
    best: np.ndarray                 # [F, cap, 3, 2] uint32 {landmark, distance}
    decision: np.ndarray             # [F, cap] uint32
    merge_ok: np.ndarray             # [F, cap] uint8
    n_world: int
    tags: dict = field(default_factory=dict)     # name -> (f, j)

    def row_of(self, f, j):
        return self.n_world + f * self.table.cap + j


def prepare_merged(mc, alter=()):
    """(f, j) -> Prepared for the slots that get a row: decision == 2 and merge_ok != 0"""
    t, out = mc.table, {}
    for f, j in np.argwhere((mc.decision == 2) & (mc.merge_ok != 0)):
        l0, l1 = int(mc.best[f, j, 0, 0]), int(mc.best[f, j, 1, 0])
        rows = None
        if l0 < t.n_landmarks and l1 < t.n_landmarks:
            r0, r1 = _range(t, l0), _range(t, l1)
            if r0 is not None and r1 is not None:
                rows = r0 if "merged_first_only" in alter else np.concatenate([r0, r1])
        out[(int(f), int(j))] = _prepare_rows(t, rows, alter)
    return out


def merged(mc, st=Settings(), alter=(), prepared=None):
    """(f, j) -> Row, for row n_world + f * cap + j of the world table; every other row is left as it was"""
    prepared = prepared if prepared is not None else prepare_merged(mc, alter)
    return {k: decide(p, True, st, alter) for k, p in prepared.items()}


@dataclass
class PairCase:
    """The arguments of rs_triangulate_pairs_batch_device; the consensus' outputs are the caller's own here."""
    cap: int
    cam_a: tuple
    cam_b: tuple
    xy_a: np.ndarray                 # [blocks, cap, 2] float32
    xy_b: np.ndarray
    ia: list
    ib: list
    pairs: np.ndarray                # [S, cap, 2] uint32
    npairs: np.ndarray               # [S] uint32
    pose: np.ndarray                 # [S, 12]
    best_id: np.ndarray              # [S] uint32
    inliers: np.ndarray              # [S, cap] uint32
    n_inliers: np.ndarray            # [S] uint32


def pairs(pc, st=Settings(), alter=()):
    """(scene, i) -> Row for every inlier i < min(n_inliers, cap) of a scene with a model: triangulate_relative(pose, a, b) =
    the list (identity, a), (pose, b), no robustness test; every other row is left as it was"""
    out = {}
    ident = np.hstack([np.eye(3), np.zeros((3, 1))])
    for s in range(len(pc.npairs)):
        if int(pc.best_id[s]) == NO_ID:
            continue
        ni, npr = min(int(pc.n_inliers[s]), pc.cap), min(int(pc.npairs[s]), pc.cap)
        P = np.stack([ident, pc.pose[s].reshape(3, 4)])
        for i in range(ni):
            m = int(pc.inliers[s, i])
            bad = m >= npr or int(pc.pairs[s, m, 0]) >= pc.cap or int(pc.pairs[s, m, 1]) >= pc.cap
            if bad:
                out[(s, i)] = decide(Prepared(2, True), False, st, alter)
                continue
            pa, pb = pc.xy_a[pc.ia[s], pc.pairs[s, m, 0]], pc.xy_b[pc.ib[s], pc.pairs[s, m, 1]]
            B = np.stack([calibrate(pa[0], pa[1], pc.cam_a, alter), calibrate(pb[0], pb[1], pc.cam_b, alter)])
            out[(s, i)] = decide(prepare(P, B, alter), False, st, alter)
    return out


# ------------------------------------------------------------------------------------------------ holding a build to it
def sin_angle(a, b):
    a, b = a / np.linalg.norm(a), b / np.linalg.norm(b)
    return float(np.linalg.norm(a - (a @ b) * b))


def conditions(row, st):
    """the three conditions of a designed case, on one row"""
    if row.robust_asked and math.isfinite(row.best):
        assert abs(row.best - st.min_cos) >= THRESHOLD_GUARD, ("a pair distance at the threshold", row.best, st.min_cos)
    if row.lam is not None:
        assert row.gap >= GAP_GUARD, ("the two smallest eigenvalues are not told apart", row.lam)
    if math.isfinite(row.min_dot):
        assert row.min_dot >= DOT_GUARD, ("a cheirality product at zero", row.min_dot)


def disagreements(names, points, reasons, rows):
    """The entries where a build's (point [4], reason byte) differs from the statement's row: another reason, a "None" row that
    is not {0, 0, 0, -1}, a point with w's sign bit set, a point further from the statement's than the bound.
    -> ([(name, what)], the worst sin(angle) / bound seen on the rows that agree)"""
    out, worst = [], 0.0
    for name, p, r, row in zip(names, points, reasons, rows):
        if int(r) != row.reason:
            out.append((name, f"reason {int(r)}, the statement says {row.reason}"))
        elif row.reason != OK:
            if np.asarray(p).tobytes() != NONE_ROW.tobytes():
                out.append((name, f"reason {row.reason} but the row is {p}"))
        else:
            ratio = sin_angle(p, row.point) / row.bound
            if np.signbit(p[3]) or not ratio <= 1.0 or abs(np.linalg.norm(p[:3]) - 1.0) > 1e-14:
                out.append((name, f"point {p}, the statement says {row.point}: {ratio:.3g} of the bound"))
            else:
                worst = max(worst, ratio)
    return out, worst


def hold(names, points, reasons, rows, st):
    """Asserts the three conditions on every row, then that the build agrees on every row.  -> worst sin(angle) / bound"""
    for row in rows:
        conditions(row, st)
    bad, worst = disagreements(names, points, reasons, rows)
    assert not bad, (len(bad), bad[:5])
    return worst


# ------------------------------------------------------------------------------------------------ the catalogue
CAM = (950.0, 955.0, 640.0, 250.0, 0.5, -0.05)
CAM_NO_K1 = (984.2439, 980.8141, 690.0, 233.1966, -0.3, None)
CAP, N_BLOCKS, NAN_BLOCK, BACK_BLOCK = 300, 12, 10, 11
LIST_LENGTHS = (0, 1, 2, 3, 5, 8, 33, 64)
SETTINGS_GRID = ((3, 0xFFFFFFFF), (3, 2), (2, 0xFFFFFFFF), (5, 0xFFFFFFFF))      # (robust_minimum_observations, n_views)
N_DESIGNED = 32


def rodrigues(v):
    v = np.asarray(v, np.float64)
    th = np.linalg.norm(v)
    if th == 0.0:
        return np.eye(3)
    k = v / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def project(cam, q):
    """A point in camera axes -> its pixel under the camera model calibrate inverts: the distorted normalised point is the
    fixed point of x_d = x (1 + k1 r_d^2)."""
    fx, fy, cx, cy, skew, k1 = cam
    x, y = q[0] / q[2], q[1] / q[2]
    xd, yd = x, y
    if k1 is not None:
        for _ in range(100):
            d = 1.0 + k1 * (xd * xd + yd * yd)
            xd, yd = x * d, y * d
    return fx * xd + skew * yd + cx, fy * yd + cy


def _pose(R, c):
    return np.hstack([R, (-R @ np.asarray(c, np.float64)).reshape(3, 1)])


def _blocks(rng):
    """The twelve poses.  0, 1, 2: centres on one line, 0 in the middle (a list 0, 1, 2 has its widest pair in (1, 2)); 3, 4: 0.03
    apart; 5..9: anywhere in the box; 10: block 5's pose with a NaN in its rotation; 11: a camera at (0, 0, 1) that looks down
    -z, away from every point.  No centre is the origin."""
    c0 = np.array([0.1, -0.2, 0.05])
    centres = [c0, c0 - [0.3, 0, 0], c0 + [0.3, 0, 0], np.array([-0.7, 0.6, -0.2])]
    centres.append(centres[3] + 0.03 * np.array([0.6, 0.8, 0.0]))
    while len(centres) < 10:
        c = rng.uniform([-1, -1, -0.3], [1, 1, 0.3])
        if all(np.linalg.norm(c - d) >= 0.1 for d in centres):
            centres.append(c)
    poses = [_pose(rodrigues(rng.normal(0, 0.15, 3)), c) for c in centres]
    nan = poses[5].copy()
    nan[1, 2] = np.nan
    poses.append(nan)
    poses.append(_pose(np.diag([-1.0, 1.0, -1.0]), [0.0, 0.0, 1.0]))
    return np.stack(poses)


class _Builder:
    def __init__(self, rng, cam, noise=0.5):
        self.rng, self.cam, self.noise = rng, cam, noise
        self.poses = _blocks(rng)
        self.xy = np.zeros((N_BLOCKS, CAP, 2), np.float32)
        self.used = np.zeros(N_BLOCKS, np.int64)
        self.lists, self.tags = [], {}

    def see(self, block, X):
        """a new keypoint of `block`: the projection of world point X plus pixel noise -> {block, feature}"""
        j = int(self.used[block])
        assert j < CAP, "a keypoint block of the catalogue is full"
        self.used[block] += 1
        P = self.poses[NAN_BLOCK - 5] if block == NAN_BLOCK else self.poses[block]
        px = project(self.cam, P[:, :3] @ X + P[:, 3])
        self.xy[block, j] = np.array(px) + self.rng.uniform(-self.noise, self.noise, 2)
        return [block, j]

    def point(self, depth):
        return np.array([self.rng.uniform(-0.5, 0.5) * depth, self.rng.uniform(-0.35, 0.35) * depth, depth])

    def add(self, tag, X, blocks):
        self.tags.setdefault(tag, []).append(len(self.lists))
        self.lists.append([self.see(b, X) for b in blocks])
        return self.lists[-1]

    def ordinary(self, n):
        """n observations of one point 2 .. 3 000 units deep (log-uniform); a list longer than the ten ordinary blocks sees
        them again, each time in another keypoint"""
        perm = self.rng.permutation(10)
        self.add(f"len_{n}", self.point(float(np.exp(self.rng.uniform(np.log(2.0), np.log(3000.0))))), [int(perm[k % 10]) for k in range(n)])


def table(n_landmarks, seed=0x7AB1E):
    """The landmark table of the catalogue: 12 blocks of 300 keypoints, the K1 + skew camera, pixel noise +- 0.5.  Landmarks
    0 .. 31 are designed (tags), the others have the list lengths 0, 1, 2, 3, 5, 8, 33, 64 mixed inside every wave of 64.  The
    last landmark's range leaves the observation array the call states (n_obs is two rows short)."""
    rng = np.random.default_rng(seed)
    b = _Builder(rng, CAM)
    b.add("first", b.point(4.0), [6, 2, 9, 0, 7])
    c0 = np.array([0.1, -0.2, 0.05])
    for _ in range(8):          # 0 in the middle of 1 and 2, the point 10 units ahead: d01, d02 ~ 4.5e-4 < 1e-3 < d12 ~ 1.8e-3
        b.add("only_pair_1_2", c0 + [rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05), 10.0], [0, 1, 2])
    for k in range(4):          # a NaN pose among robust observations, at every place of the list
        blocks = [6, 1, 8, 2]
        blocks.insert(k, NAN_BLOCK)
        b.add("nan_pose", b.point(3.0 + k), blocks)
    b.add("nan_in_every_wide_pair", b.point(6.0), [3, NAN_BLOCK, 4])      # the only pair of numbers is the narrow (3, 4)
    for k in range(4):          # the camera that looks away, behind the first observation
        blocks = [7, 0, 9]
        blocks.insert(1 + k % 3, BACK_BLOCK)
        b.add("behind", b.point(4.0 + k), blocks)
    b.add("behind_first", b.point(5.0), [BACK_BLOCK, 2, 8, 5])
    for k, (blk, feat) in enumerate(((N_BLOCKS, 0), (NO_ID, 3), (0, CAP), (4, NO_ID))):
        lst = b.add("bad_index", b.point(3.0), [5, 1, 9, 6][:1 if k == 3 else 4])
        lst[k % len(lst)] = [blk, feat]
    P = b.point(6.0)
    b.add("narrow_side", P, [3, 4])                   # 23: d ~ 1.2e-5
    b.add("one_block_twice", P, [1, 1])               # 24: the same point from block 1 in two keypoints
    Q = b.point(5.0)
    b.add("single_of_block_5", Q, [5])                # 25, 26: one observation each, the same block
    b.add("single_of_block_5", Q, [5])
    S = b.point(3.0)
    b.add("single_wide", S, [0])                      # 27, 28: one observation each, blocks 0 and 7
    b.add("single_wide", S, [7])
    b.add("empty", S, [])                             # 29
    b.add("robust_three", b.point(3.0), [2, 8, 5])    # 30
    b.add("narrowest", b.point(1500.0), [3, 4])       # 31: d ~ 1e-10
    assert len(b.lists) == N_DESIGNED
    total = max(n_landmarks, N_DESIGNED)
    for w0 in range(0, total, 64):
        free = [l for l in range(w0, min(w0 + 64, total)) if l >= N_DESIGNED]
        base = ([64, 33] + [LIST_LENGTHS[k % 6] for k in range(len(free))])[:len(free)]
        lens = [base[k] for k in rng.permutation(len(free))]
        for l, n in zip(free, lens):
            b.ordinary(5 if l == total - 1 else int(n))
    lists = b.lists[:n_landmarks]
    start = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.uint32)
    obs = np.array([o for l in lists for o in l], np.int64).reshape(-1, 2).astype(np.uint32)
    n_obs = len(obs) - 2 if n_landmarks > N_DESIGNED else len(obs)
    tags = {k: [l for l in v if l < n_landmarks] for k, v in b.tags.items()}
    return Table(CAP, CAM, b.xy, b.poses.reshape(N_BLOCKS, 12), start, obs, n_obs, tags)


def around(d):
    """(the largest number t with d - t >= 1e-12, the smallest with t - d >= 1e-12): d -+ 1e-12 rounded away from d, so that
    the guard holds in floating point too"""
    lo, hi = d - THRESHOLD_GUARD, d + THRESHOLD_GUARD
    while d - lo < THRESHOLD_GUARD:
        lo = np.nextafter(lo, -math.inf)
    while hi - d < THRESHOLD_GUARD:
        hi = np.nextafter(hi, math.inf)
    return float(lo), float(hi)


def thresholds(t, prepared=None):
    """-> (16 chosen landmarks, the 33 thresholds: d - 1e-12 and d + 1e-12 for each, d its best pair distance, and the
    default 1e-3).  Chosen: two of the landmarks whose only robust pair is (1, 2), and fourteen spread evenly by rank of d over
    the landmarks of three and more observations that reach the solver — above the distance under which some list's two
    smallest eigenvalues come within 1e-5 l4 of each other (every launch is judged over all rows, and a threshold below that
    distance would send such a list to the solver: the gap condition, with a factor of ten to spare)."""
    prepared = prepared if prepared is not None else prepare_landmarks(t)
    solved = [l for l, p in enumerate(prepared) if p.lam is not None and math.isfinite(p.best)]
    narrow = [prepared[l].best for l in solved if (prepared[l].lam[1] - prepared[l].lam[0]) / prepared[l].lam[3] < 10 * GAP_GUARD]
    floor = 2.0 * max(narrow, default=0.0)
    pool = sorted((l for l in solved if prepared[l].n >= 3 and prepared[l].best > floor and l not in t.tags["only_pair_1_2"]),
                  key=lambda l: prepared[l].best)
    assert len(pool) >= 14
    chosen = t.tags["only_pair_1_2"][:2] + [pool[round(k * (len(pool) - 1) / 13)] for k in range(14)]
    assert len(set(chosen)) == 16
    values = sorted({v for l in chosen for v in around(prepared[l].best)} | {1e-3})
    assert len(values) == 33
    return chosen, values


def merge_case(seed=0x3E6E):
    """rs_triangulate_merged_device over table(257): F = 3 frame slots of 300 features (a ragged second block of lanes), every
    combination of decision 0 / 1 / 2 and merge_ok 0 / 1 at random, keys outside the table, and the designed slots (tags)."""
    t = table(257)
    rng = np.random.default_rng(seed)
    F, nl = 3, t.n_landmarks
    best = rng.integers(0, nl, (F, CAP, 3, 2)).astype(np.uint32)
    best[rng.random((F, CAP)) < 0.04, 1, 0] = NO_ID
    best[rng.random((F, CAP)) < 0.03, 0, 0] = nl
    best[rng.random((F, CAP)) < 0.02, 1, 0] = nl
    best[rng.random((F, CAP)) < 0.02, 0, 0] = NO_ID
    dec = rng.integers(0, 3, (F, CAP)).astype(np.uint32)
    ok = (rng.random((F, CAP)) < 0.6).astype(np.uint8)
    tag = lambda name: t.tags[name]
    designed = {
        "cross_pair_only": ((0, 299), tag("narrow_side")[0], tag("one_block_twice")[0]),      # robust through a pair across the lists
        "cross_pair_only_swapped": ((1, 256), tag("one_block_twice")[0], tag("narrow_side")[0]),
        "same_block_singles": ((2, 5), *tag("single_of_block_5")),                            # two observations, one centre
        "wide_singles": ((0, 7), *tag("single_wide")),                                        # robust where two observations are enough
        "empty_then_robust": ((1, 8), tag("empty")[0], tag("robust_three")[0]),
        "robust_then_empty": ((2, 280), tag("robust_three")[0], tag("empty")[0]),
        "robust_then_behind": ((0, 9), tag("robust_three")[0], tag("behind")[0]),
        "robust_then_bad_index": ((1, 10), tag("robust_three")[0], tag("bad_index")[0]),
        "robust_then_nan": ((2, 11), tag("robust_three")[0], tag("nan_pose")[0]),
        "first_key_is_n_landmarks": ((0, 12), nl, tag("robust_three")[0]),
        "second_key_is_none": ((1, 13), tag("robust_three")[0], NO_ID),
        "narrow_then_narrowest": ((2, 14), tag("narrow_side")[0], tag("narrowest")[0]),
        "last_landmark_leaves_the_array": ((0, 257), tag("robust_three")[0], nl - 1),
    }
    tags = {}
    for name, ((f, j), l0, l1) in designed.items():
        best[f, j, 0, 0], best[f, j, 1, 0], dec[f, j], ok[f, j] = l0, l1, 2, 1
        tags[name] = (f, j)
    best[0, 15, :2, 0], dec[0, 15], ok[0, 15] = (tag("robust_three")[0], tag("first")[0]), 2, 0       # not admitted
    best[0, 16, :2, 0], dec[0, 16], ok[0, 16] = (tag("robust_three")[0], tag("first")[0]), 1, 1       # not a merge candidate
    tags["not_admitted"], tags["not_a_candidate"] = (0, 15), (0, 16)
    return MergeCase(t, best, dec, ok, nl + 5, tags)


def pair_case(seed=0x9A12):
    """rs_triangulate_pairs_batch_device: 5 scenes over 300 features, K1 + skew on side a only, the keypoint blocks in permuted
    order.  n_inliers 0, 1, 256, 300 and 0xFFFF; scene 2 states more pairs than the capacity and lists inliers between the two,
    scene 4 has 280 pairs and an inlier between that and the capacity, scene 3 has no model (and 300 inliers that must not be touched); inlier indices >= npairs and features >= cap; depths of 2
    to 150 units seen over baselines of 1, 0.3, 0.03 and 0.01 units: the parallax falls under the pixel noise (points land
    behind a camera: reason 5) and the eigenvalue gap to within two orders of its guard (there is no robustness test on this
    path to keep such pairs out)."""
    rng = np.random.default_rng(seed)
    S = 5
    BASELINES = (1.0, 0.3, 0.03, 1.0, 0.01)
    cam_a, cam_b = CAM, CAM_NO_K1
    ia, ib = [4, 3, 2, 1, 0], [1, 3, 0, 2, 4]
    xy_a = np.zeros((S, CAP, 2), np.float32); xy_b = np.zeros((S, CAP, 2), np.float32)
    pr = np.zeros((S, CAP, 2), np.uint32)
    pose = np.zeros((S, 12))
    npairs = np.array([300, 200, 511, 300, 280], np.uint32)
    n_inl = np.array([0, 1, 256, 300, 0xFFFF], np.uint32)
    best_id = np.array([7, 0, 3, NO_ID, 12], np.uint32)
    inl = np.zeros((S, CAP), np.uint32)
    for s in range(S):
        R = rodrigues(rng.normal(0, 0.1, 3))
        tr = rng.normal(0, 1, 3)
        tr *= BASELINES[s] / np.linalg.norm(tr)          # (l2 - l1) / l4 falls with the square of the baseline
        pose[s] = np.hstack([R, tr.reshape(3, 1)]).reshape(12)
        fa, fb = rng.permutation(CAP), rng.permutation(CAP)
        pr[s, :, 0], pr[s, :, 1] = fa, fb
        for m in range(CAP):
            depth = float(np.exp(rng.uniform(np.log(2.0), np.log(150.0))))
            X = np.array([rng.uniform(-0.4, 0.4) * depth, rng.uniform(-0.3, 0.3) * depth, depth])
            xy_a[ia[s], fa[m]] = np.array(project(cam_a, X)) + rng.uniform(-0.5, 0.5, 2)
            xy_b[ib[s], fb[m]] = np.array(project(cam_b, R @ X + tr)) + rng.uniform(-0.5, 0.5, 2)
        n_eff = min(int(npairs[s]), CAP)
        inl[s] = rng.integers(0, n_eff, CAP)
    inl[1, 0] = 17
    inl[2, [3, 100, 255]] = (300, 305, 510)            # below the stated count, at and above the capacity
    inl[2, [4, 200]] = (NO_ID, 299)
    inl[4, [0, 150, 299]] = (290, NO_ID, 7)             # 290: inside the capacity, outside the scene's 280 pairs
    pr[2, inl[2, 10]] = (CAP, 3)                       # features outside the block
    pr[4, inl[4, 11]] = (2, NO_ID)
    pr[4, inl[4, 298]] = (NO_ID, CAP)
    return PairCase(CAP, cam_a, cam_b, xy_a, xy_b, ia, ib, pr, npairs, pose, best_id, inl, n_inl)


def list_case(n, seed=0x115):
    """rs_triangulate_observations: n observations of one point 5 units deep, bearings given directly (noise 1e-4 rad)"""
    rng = np.random.default_rng([seed, n])
    poses = _blocks(rng)[:10]
    X = np.array([0.4, -0.3, 5.0])
    P = poses[np.arange(n) % 10]
    B = np.zeros((n, 3))
    for k in range(n):
        q = P[k, :, :3] @ X + P[k, :, 3] + rng.normal(0, 1e-4, 3) * 5.0
        B[k] = q / np.linalg.norm(q)
    return P, B
