"""One synthetic world, the metric that compares a reconstruction with it, the invariants of a landmark table and the chain of
the existing statements that carries the world through a reconstruction's life: start -> grow -> bridge -> merge -> export.

numpy and the standard library only; the stages are the *_statement.py modules, the consensus' poses come from a numpy
eight-point and the two-conic P3P of test_gpu_independent_geometry.py.  Nothing here imports the product, a host build or ctypes.
What this module adds is the GLUE: one plain function per stage boundary that says what one stage's output means to the next.
Each glue function takes `alter`, a set of names of deliberately wrong conventions (ALTERATIONS); tests/test_reconstruction_life.py
shows that every one of them is caught by the invariants, by aligned_errors or by the export's colour check.

Poses are WorldToCamera [R | t] unless a name says camera-to-camera; a table is a list of rows, row = list of (block, feature).
"""
import math
from types import SimpleNamespace

import numpy as np

import bootstrap_table_statement as BT
import consensus_statement as CS
import covisibility_statement as CV
import landmark_table_statement as LT
import matching_statement as MS
import observation_filter_statement as OF
import export_statement as EX
import pose_graph_statement as PG
import reconstruction_merge_statement as RM
import single_view_statement as SV
import three_view_constraint_statement as TC
import three_view_statement as TV
import triangulate_statement as TS
from test_gpu_independent_geometry import p3p_conics

NONE = 0xFFFFFFFF
CAP = 256
N_VIEWS = 13
CAM = (1000.0, 1000.0, 640.0, 360.0, 0.0)            # three_view_checker.rig_camera()
CAM6 = CAM + (None,)
A_VIEWS, B_VIEWS, BRIDGE = (0, 6), (6, 12), 12       # block ranges of the two reconstructions; the bridging frame's view
A_START, B_START = (0, 1, 2), (6, 7, 8)              # (centre, first, second) of the two bootstraps
A_GROW, B_GROW = (3, 4, 5), (9, 10, 11)
ALTERATIONS = ("pose_inverted_into_table", "first_second_exchanged", "view_base_one_high", "src_pose_from_a", "merge_transform_inverted",
               "colour_of_last_observation")

# One set of settings for every phase and both sides; the device tests build the product's parameter structs from these.
SETTINGS = dict(
    arrsac=dict(threshold=1e-5, n_hypotheses=256, seed=7, block_size=64, init_blocks=1, max_candidates=64, halve=True),
    p3p=dict(threshold=1e-5, n_hypotheses=512, seed=0, block_size=64, init_blocks=1, max_candidates=64, halve=True, sprt=True,
             estimations_per_block=0),
    join_minimum=64, join_seed=0xABCDEF12345,
    three_view=dict(three_view_patience=64, three_view_filter_loop_iterations=2),
    single_view=dict(single_view_optimization_rate=0.02, single_view_patience=100, single_view_filter_loop_iterations=2),
    filter=dict(minimum_robust_landmarks=8),
    covisibility=dict(optimization_robust_covisibility_minimum_landmarks=4, optimization_minimum_landmarks=4),
    constraint=dict(constraint_patience=64),
    pose_graph=dict(optimization_iterations=64),
)


# ------------------------------------------------------------------------------------------------------------ the world
def _rodrigues(w):
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / th
    return np.eye(3) + np.sin(th) * k + (1 - np.cos(th)) * (k @ k)


def _look_at(centre, target, roll):
    z = (target - centre) / np.linalg.norm(target - centre)
    x = np.cross([0.0, 1.0, 0.0], z)
    x /= np.linalg.norm(x)
    r = np.stack([x, np.cross(z, x), z])                 # rows: the camera's axes in the world
    r = _rodrigues(np.array([0.0, 0.0, roll])) @ r
    return np.hstack([r, (-r @ centre)[:, None]])


def world(seed, noise, wrong_share):
    """13 views on an arc around 216 points 4 - 10 units deep.  Reconstruction A is views 0-5, B views 6-11 (closer together and walking the arc the
    other way, so the two bootstraps fix different scales, origins and orientations), view 12 stands between them.  -> SimpleNamespace; the designed matcher outputs come
    from pair_lists() and frame_hits()."""
    rng = np.random.default_rng(seed)
    target = np.array([0.0, 0.0, 7.0])
    ang = np.concatenate([-0.47 + 0.19 * np.arange(6), 0.40 - 0.16 * np.arange(6), [0.03]]) + rng.uniform(-0.008, 0.008, N_VIEWS)
    radius = 6.5 + rng.uniform(-0.25, 0.25, N_VIEWS)
    centres = np.stack([target[0] + radius * np.sin(ang), rng.uniform(-0.25, 0.25, N_VIEWS), target[2] - radius * np.cos(ang)], 1)
    poses = np.stack([_look_at(c, target + rng.uniform(-0.3, 0.3, 3), r) for c, r in zip(centres, rng.uniform(-0.05, 0.05, N_VIEWS))])
    kinds = ["a"] * 80 + ["b"] * 80 + ["both"] * 48 + ["rare"] * 8
    n = len(kinds)
    points = np.stack([rng.uniform(-2.0, 2.0, n), rng.uniform(-1.2, 1.2, n), rng.uniform(5.2, 8.8, n)], 1)
    seen = []
    for p, kind in enumerate(kinds):
        side = lambda lo: [lo, lo + 1, lo + 2] + [v for v in range(lo + 3, lo + 6) if rng.random() < 0.9]
        if kind == "a":
            s = side(0) + ([BRIDGE] if rng.random() < 0.6 else [])
        elif kind == "b":
            s = side(6) + ([BRIDGE] if rng.random() < 0.6 else [])
        elif kind == "both":                             # four views of each side and the bridging frame: nine
            s = [BRIDGE]
            for lo in (0, 6):
                drop = rng.permutation(6)[:2]
                s += [lo + v for v in range(6) if v not in drop]
        else:                                            # two or three views of one side
            lo = 0 if p % 2 == 0 else 6
            s = [lo + int(v) for v in rng.permutation(6)[:2 + p % 4 // 2]]
        seen.append(sorted(s))
    px = np.zeros((N_VIEWS, CAP, 2), np.float32)
    px[:] = -1000.0                                      # unused entries lie far outside the frame
    feature = np.full((N_VIEWS, n), -1, np.int64)
    point_of = np.full((N_VIEWS, CAP), -1, np.int64)
    counts = np.zeros(N_VIEWS, np.uint32)
    for v in range(N_VIEWS):
        mine = [p for p in range(n) if v in seen[p]]
        order = rng.permutation(len(mine))
        x = points[mine] @ poses[v][:, :3].T + poses[v][:, 3]
        assert x[:, 2].min() > 3.0
        uv = np.stack([CAM[0] * x[:, 0] / x[:, 2] + CAM[2], CAM[1] * x[:, 1] / x[:, 2] + CAM[3]], 1) + noise * rng.standard_normal((len(mine), 2))
        assert uv.min() > 0 and uv[:, 0].max() < 1280 and uv[:, 1].max() < 720
        for j, k in enumerate(order):
            px[v, j], feature[v, mine[k]], point_of[v, j] = uv[k], j, mine[k]
        counts[v] = len(mine)
    colours = rng.integers(0, 256, (N_VIEWS, CAP, 3), dtype=np.uint8)
    n_obs = np.array([len(s) for s in seen])
    assert n_obs.min() == 2 and n_obs.max() == 9 and kinds.count("both") >= 40
    return SimpleNamespace(seed=seed, noise=noise, wrong_share=wrong_share, poses=poses, points=points, seen=seen, px=px, feature=feature,
                           point_of=point_of, counts=counts, colours=colours, kinds=kinds, n_points=n)


def kps_of(w):
    """the keypoint blocks [13][cap] as the stages that calibrate read them: fields x, y"""
    kps = np.zeros((N_VIEWS, CAP), np.dtype([("x", np.float32), ("y", np.float32)]))
    kps["x"], kps["y"] = w.px[..., 0], w.px[..., 1]
    return kps


def bearings_of(w):
    """[13][cap][3] float64 unit bearings of the f32 pixels"""
    return TS.calibrate(w.px[..., 0], w.px[..., 1], CAM6)


def pair_lists(w, triple):
    """the matcher's lists (centre, first) and (centre, second) of a bootstrap: the common points in a seeded order, wrong_share
    of the entries naming another entry's feature (tests/test_gpu_bootstrap.synthetic_views) -> pairs [2][cap][2] u32, npairs [2]"""
    rng = np.random.default_rng([w.seed, 11] + list(triple))
    c = triple[0]
    pairs, npairs = np.zeros((2, CAP, 2), np.uint32), np.zeros(2, np.uint32)
    for k, other in enumerate(triple[1:]):
        common = [p for p in range(w.n_points) if c in w.seen[p] and other in w.seen[p]]
        theirs = w.feature[other][common].copy()
        wrong = rng.permutation(len(common))[:int(round(len(common) * w.wrong_share))]
        theirs[wrong] = theirs[np.roll(wrong, 1)]
        order = rng.permutation(len(common))
        pairs[k, :len(common)] = np.stack([w.feature[c][common][order], theirs[order]], 1)
        npairs[k] = len(common)
    return pairs, npairs


def frame_hits(w, frame, stored):
    """what the k = 3 searches of frame view `frame` against the views `stored` find: per feature the (view, feature) it is
    nearest to in every stored view that sees its point; wrong_share of the features find another feature's hits instead"""
    rng = np.random.default_rng([w.seed, 13, frame] + list(stored))
    n = int(w.counts[frame])
    hits = [[(u, int(w.feature[u][p])) for u in stored if u in w.seen[p]] for p in w.point_of[frame][:n]]
    wrong = rng.permutation(n)[:int(round(n * w.wrong_share))]
    moved = [hits[j] for j in np.roll(wrong, 1)]
    for j, h in zip(wrong, moved):
        hits[j] = h
    return hits


def matcher_tables(w, frames, stored, landmark_map):
    """best [F][cap][3][2] / decision [F][cap] as hm_best_of_views_batch_device leaves them for the designed hits, given the
    per-feature landmark map of the reconstruction the frames are matched against: the landmarks the hits name in hit order,
    decision 1 (a unique match on the first) where there is one, 0 where there is none.  The matcher itself is not part of this."""
    best = np.full((len(frames), CAP, 3, 2), NONE, np.uint32)
    decision = np.zeros((len(frames), CAP), np.uint32)
    for f, frame in enumerate(frames):
        for j, hits in enumerate(frame_hits(w, frame, stored)):
            lms = []
            for u, i in hits:
                l = int(landmark_map[u][i])
                if l != NONE and l not in lms:
                    lms.append(l)
            for r, l in enumerate(lms[:3]):
                best[f, j, r] = (l, (10, 50, 90)[r])
            decision[f, j] = min(len(lms), 1)
    return best, decision


# ------------------------------------------------------------------------------------------------------------ the metric
def umeyama(src, dst):
    """the similarity (s, R, t) with dst ~ s R src + t in the least-squares sense (Umeyama 1991, closed form)"""
    ms, md = src.mean(0), dst.mean(0)
    a, b = src - ms, dst - md
    u, d, vt = np.linalg.svd(b.T @ a / len(src))
    sgn = np.array([1.0, 1.0, np.sign(np.linalg.det(u) * np.linalg.det(vt))])
    r = u @ np.diag(sgn) @ vt
    s = float((d * sgn).sum() / (a ** 2).sum() * len(src))
    return s, r, md - s * r @ ms


def truth_of(w, rows, views):
    """what aligned_errors compares with: the views of the reconstruction, and for every row of its table the point most of its
    observations show (-1: none, or no majority)"""
    row_point = []
    for row in rows:
        pts = [int(w.point_of[b][f]) for b, f in row if b < N_VIEWS and f < CAP]
        best = max(set(pts), key=pts.count) if pts else -1
        row_point.append(best if pts and 2 * pts.count(best) > len(pts) else -1)
    return SimpleNamespace(w=w, views=list(views), row_point=row_point)


def aligned_errors(poses, world_rows, reasons, truth, similarity=None):
    """poses [blocks][12] (or [3][4] each), world_rows [n][4] homogeneous, reasons [n] (0: TRI_OK) of one reconstruction ->
    dict(rotation, centre, point, left_out, similarity): one similarity fitted to the camera centres and the TRI_OK points
    together; the worst rotation angle (rad) over the views, the worst centre distance over the longest true baseline, the worst
    point distance over the point's true distance from the middle of the true centres, and the share of the truth points with at
    least three observations in these views that no TRI_OK row was compared for."""
    w, views = truth.w, truth.views
    if not views:
        return dict(rotation=math.inf, centre=math.inf, point=math.inf, left_out=1.0, similarity=(1.0, np.eye(3), np.zeros(3)), n_points=0)
    est = [np.asarray(poses[v], np.float64).reshape(3, 4) for v in views]
    c_est = np.stack([-p[:, :3].T @ p[:, 3] for p in est])
    c_true = np.stack([-w.poses[v][:, :3].T @ w.poses[v][:, 3] for v in views])
    rows = [l for l in range(min(len(world_rows), len(truth.row_point))) if reasons[l] == 0 and truth.row_point[l] >= 0 and world_rows[l][3] > 0]
    x_est = np.array([np.asarray(world_rows[l][:3], np.float64) / world_rows[l][3] for l in rows]).reshape(-1, 3)
    x_true = w.points[[truth.row_point[l] for l in rows]].reshape(-1, 3)
    s, r, t = similarity or umeyama(np.concatenate([c_est, x_est]), np.concatenate([c_true, x_true]))
    rot = 0.0
    for p, v in zip(est, views):
        d = p[:, :3] @ (w.poses[v][:, :3] @ r).T
        rot = max(rot, float(np.arccos(np.clip((np.trace(d) - 1.0) / 2.0, -1.0, 1.0))))
    baseline = max(float(np.linalg.norm(a - b)) for a in c_true for b in c_true)
    centre = float(np.linalg.norm(c_est @ r.T * s + t - c_true, axis=1).max()) / baseline
    depth = np.linalg.norm(x_true - c_true.mean(0), axis=1)
    point = float((np.linalg.norm(x_est @ r.T * s + t - x_true, axis=1) / depth).max()) if len(rows) else math.inf
    wanted = {p for p in range(w.n_points) if sum(1 for v in w.seen[p] if v in views) >= 3}
    left_out = 1.0 - len(wanted & {truth.row_point[l] for l in rows}) / max(len(wanted), 1)
    return dict(rotation=rot, centre=centre, point=point, left_out=left_out, similarity=(s, r, t), n_points=len(rows))


# ------------------------------------------------------------------------------------------------------------ the invariants
def rows_of(start, obs, n_rows=None):
    """the CSR arrays of a table -> its rows"""
    start = np.asarray(start, np.int64)
    n = len(start) - 1 if n_rows is None else n_rows
    return [[(int(b), int(f)) for b, f in obs[start[l]:start[l + 1]]] for l in range(n)]


def invariants(rows, view_range, landmark_map=None, tombstones=()):
    """Every (block, feature) at most once, no landmark with two observations in one view, every block inside the
    reconstruction's range, the tombstones empty and, where a per-feature map is given, the map the inverse of the table.
    -> list of what is broken (empty: all hold)"""
    broken, where = [], {}
    lo, hi = view_range
    for l, row in enumerate(rows):
        if len({b for b, _ in row}) != len(row):
            broken.append(("two observations in one view", l))
        for o in row:
            if o in where:
                broken.append(("observation twice", o, where[o], l))
            where[o] = l
            if not lo <= o[0] < hi:
                broken.append(("block outside the range", l, o))
    broken += [("tombstone not empty", l) for l in tombstones if rows[l]]
    if landmark_map is not None:
        named = {(b, f): int(landmark_map[b][f]) for b in range(len(landmark_map)) for f in range(len(landmark_map[b]))
                 if int(landmark_map[b][f]) != NONE}
        if named != where:
            diff = set(named.items()) ^ set(where.items())
            broken.append(("the map is not the inverse of the table", len(diff), sorted(diff)[:4]))
    return broken


# ------------------------------------------------------------------------------------------------------------ the providers
def eight_point_provider(first, second):
    """samples [h][8] -> the four poses of each sample's essential matrix, by numpy's SVD: b^T E a = 0 over the sample, E's null
    vector, its nearest U diag(1, 1, 0) V^T, R = U W V^T or U W^T V^T, t = +-u3 (Hartley & Zisserman, 9.6.2)"""
    wm = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])

    def provider(smp):
        smp = np.asarray(smp, np.int64)
        poses, ok = np.zeros((len(smp), 4, 3, 4)), np.ones((len(smp), 4), bool)
        for h, idx in enumerate(smp):
            a, b = first[idx], second[idx]
            e = np.linalg.svd(np.einsum("ni,nj->nij", b, a).reshape(len(idx), 9))[2][-1].reshape(3, 3)
            u, _, vt = np.linalg.svd(e)
            u, vt = u * np.sign(np.linalg.det(u)), vt * np.sign(np.linalg.det(vt))
            for k, (r, t) in enumerate(((u @ wm @ vt, u[:, 2]), (u @ wm.T @ vt, u[:, 2]), (u @ wm @ vt, -u[:, 2]), (u @ wm.T @ vt, -u[:, 2]))):
                poses[h, k] = np.hstack([r, t[:, None]])
        return poses, ok
    return provider


def p3p_provider(bearings, points):
    """samples [h][3] -> up to four poses of each, by the two-conic P3P"""
    def provider(smp):
        smp = np.asarray(smp, np.int64)
        poses, ok = np.zeros((len(smp), 4, 3, 4)), np.zeros((len(smp), 4), bool)
        for h, idx in enumerate(smp):
            x = points[idx]
            if np.any(x[:, 3] <= 0):
                continue
            try:
                found = p3p_conics(bearings[idx], x[:, :3] / x[:, 3:4])
            except np.linalg.LinAlgError:
                found = []
            for k, (r, t) in enumerate(found[:4]):
                poses[h, k], ok[h, k] = np.hstack([r, t[:, None]]), True
        return poses, ok
    return provider


def _consensus(family, scene, first, second, provider, prm_kw, shuffle):
    prm_kw = dict(prm_kw)
    n_hyp, thr = prm_kw.pop("n_hypotheses"), prm_kw.pop("threshold")
    prm = CS.Params(threshold=thr, bound=True, **dict(dict(sprt=True), **prm_kw))
    batch = SimpleNamespace(family=family, prm=prm, n_hyp=n_hyp, shuffle=shuffle)
    return CS.batch_scene(batch, scene, first, second, provider)[0]


# ------------------------------------------------------------------------------------------------------------ phase 1: start
def _refused(stage):
    """what a refusal leaves: no view, no row, the pool's poses as they were"""
    return SimpleNamespace(poses=np.zeros((N_VIEWS, 12)), rows=[], split=[], world=np.zeros((0, 4)), reason=np.zeros(0, np.uint8), table_rows=[],
                           table_map=np.full((N_VIEWS, CAP), NONE, np.uint32), views=[], refused=stage)


def start(w, triple, view_base, alter=(), lists=None):
    """What reconstruction.start_reconstructions does for one scene: the two-view consensus of (centre, first) and (centre,
    second; the designed pair_lists, or `lists` = (pairs, npairs) where a matcher made them) -> the join -> the three-view
    bootstrap -> add_reconstruction at view_base -> the pose graph over the first constraint -> the observation filter -> the
    world table of the filtered rows.
    -> SimpleNamespace(poses [13][12], rows, split, landmark_map, world [rows][4], reason [rows], views, ...)"""
    bear = bearings_of(w)
    pairs, npairs = lists or pair_lists(w, triple)
    c, f, s = triple
    # consensus: slot k is the pair list k; its pose takes the centre's camera frame to the other's, translation of unit length
    slots = []
    for k, other in enumerate((f, s)):
        pr = pairs[k, :npairs[k]].astype(np.int64)
        a, b = bear[c][pr[:, 0]], bear[other][pr[:, 1]]
        slots.append(_consensus("two_view", k, a, b, eight_point_provider(a, b), SETTINGS["arrsac"], True))
    # consensus -> join: the inlier POSITIONS of a slot index its pair list; the slot's pose goes with its list
    jin = dict(cap=CAP, flags=1, n_scenes=1, slot_first=[0], slot_second=[1], minimum=SETTINGS["join_minimum"], seed=SETTINGS["join_seed"],
               pose=np.stack([r.pose.reshape(12) for r in slots]), pairs=pairs, npairs=npairs,
               inliers=[r.inliers for r in slots], n_inliers=[len(r.inliers) for r in slots], best_id=[r.best_id for r in slots])
    jout = dict(pose_first=np.zeros((1, 12)), pose_second=np.zeros((1, 12)), verdict=np.zeros(1, np.uint32), ntriples=np.zeros(1, np.uint32),
                nfirst=np.zeros(1, np.uint32), nsecond=np.zeros(1, np.uint32), triples=np.zeros((1, CAP, 3), np.uint32),
                first_only=np.zeros((1, CAP, 2), np.uint32), second_only=np.zeros((1, CAP, 2), np.uint32))
    BT.join(jin, jout)
    if alter and jout["verdict"][0] != BT.JP_OK:
        return _refused("join")
    assert jout["verdict"][0] == BT.JP_OK, ("join", int(jout["verdict"][0]), jin["n_inliers"])
    nt, nf, ns = int(jout["ntriples"][0]), int(jout["nfirst"][0]), int(jout["nsecond"][0])
    triples, first_only, second_only = jout["triples"][0, :nt].astype(np.int64), jout["first_only"][0, :nf].astype(np.int64), jout["second_only"][0, :ns].astype(np.int64)
    if "first_second_exchanged" in alter:                # the join's columns: a triple is (centre, first, second)
        triples = triples[:, [0, 2, 1]]
    # join -> bootstrap: a triple's features index the centre's, the first's and the second's keypoint block
    common = [(bear[c][i], bear[f][j], bear[s][k]) for i, j, k in triples]
    tv = TV.init_triple([jout["pose_first"][0].reshape(3, 4), jout["pose_second"][0].reshape(3, 4)], common,
                        [(bear[c][i], bear[f][j]) for i, j in first_only], [(bear[c][i], bear[s][k]) for i, k in second_only], SETTINGS["three_view"])
    if alter and tv["verdict"] != TV.VERDICTS["ok"]:
        return _refused("bootstrap")
    assert tv["verdict"] == TV.VERDICTS["ok"], ("bootstrap", tv["verdict"], tv.get("run_matches"))
    # bootstrap -> table: the centre's camera frame is the world; the two poses are the views' WorldToCamera poses as they are
    first, second = tv["poses"]
    if "pose_inverted_into_table" in alter:
        first, second = TV.invert(first), TV.invert(second)
    base = view_base + (1 if "view_base_one_high" in alter else 0)
    room = 3 * CAP
    ain = dict(cap=CAP, n_scenes=1, view_base=base, n_landmarks=0, n_obs=0, n_recons=0, obs_start=None, obs=None, recon_start=None,
               view_start=None, n_blocks=N_VIEWS, ic=[c], i_first=[f], i_second=[s], counts=w.counts, ntriples=[nt], nfirst=[nf], nsecond=[ns],
               tv_verdict=[tv["verdict"]], skip=None, triples=jout["triples"] if "first_second_exchanged" not in alter else triples[None],
               combined=[tv["combined"]], first_only=jout["first_only"], first_ok=[tv["first_ok"]], second_only=jout["second_only"],
               second_ok=[tv["second_ok"]], kps=np.arange(N_VIEWS), pose_out=[np.concatenate([first.reshape(12), second.reshape(12)])], lm_room=room)
    aout = dict(views_out=np.zeros((1, 3), np.uint32), frame_verdict=np.zeros(1, np.uint32), constraint_verdict_out=np.zeros(1, np.uint32),
                stats=np.zeros((1, 4), np.uint32), kps_dst=np.full(N_VIEWS, -1), counts_dst=np.zeros(N_VIEWS, np.uint32), poses=np.zeros((N_VIEWS, 12)),
                constraint_poses_out=np.zeros((1, 24)), obs_start_out=np.zeros(room + 1, np.uint32), obs_counts_out=np.zeros(room, np.uint32),
                obs_out=np.zeros((room, 2), np.uint32), landmarks_out=np.zeros((N_VIEWS, CAP), np.uint32), recon_start_out=np.zeros(2, np.uint32),
                view_start_out=np.zeros(2, np.uint32), counts_out=np.zeros(4, np.uint32), call_verdict=np.zeros(1, np.uint32))
    BT.add_reconstruction(ain, aout)
    if alter and aout["frame_verdict"][0] != BT.AR_OK:
        return _refused("add_reconstruction")
    assert aout["frame_verdict"][0] == BT.AR_OK, ("add_reconstruction", int(aout["frame_verdict"][0]))
    n_rows = int(aout["counts_out"][0])
    rows = rows_of(aout["obs_start_out"], aout["obs_out"], n_rows)
    views = [int(v) for v in aout["views_out"][0]]
    # (the destination pool holds view v's keypoints in block v: add_reconstruction copies source block `triple[k]` to block
    #  views[k], and the world's blocks are its views — under view_base_one_high the keypoints move with the views)
    kps, px = kps_of(w), w.px.copy()
    for k in range(3):
        kps[views[k]], px[views[k]] = kps_of(w)[triple[k]], w.px[triple[k]]
    poses = aout["poses"].copy()
    out = _optimize(px, kps, poses, rows, [(views, aout["constraint_poses_out"][0][:12].reshape(3, 4), aout["constraint_poses_out"][0][12:].reshape(3, 4))],
                    (int(aout["view_start_out"][0]), int(aout["view_start_out"][1])), strict=not alter)
    out.table_rows, out.table_map, out.views, out.px = rows, aout["landmarks_out"].copy(), views, px
    out.table_counts = aout["obs_counts_out"][:n_rows].copy()
    return out


def _optimize(px, kps, poses, rows, constraints, view_range, strict=True):
    """optimize_reconstruction with one round: the pose graph relaxed over the recorded constraints (views, first, second), the
    observation filter under the relaxed poses, the robust triangulation of the filtered rows"""
    lo, hi = view_range
    graph = PG.flatten(constraints)
    relaxed, _, bad = PG.relax({v: poses[v].reshape(3, 4) for v in range(lo, hi)}, graph, SETTINGS["pose_graph"]["optimization_iterations"])
    assert not bad or not strict, ("pose graph", bad)
    poses = poses.copy()
    for v, p in relaxed.items():
        poses[v] = p.reshape(12)
    start = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint32)
    obs = np.array([o for r in rows for o in r], np.uint32).reshape(-1, 2)
    flt = OF.filter_table(kps, poses, CAM, start, obs, [0, len(rows)], [lo, hi], OF.settings(**SETTINGS["filter"]))
    assert flt["verdict"][0] == OF.OK or not strict, ("filter", int(flt["verdict"][0]), flt["stats"][0])
    kept = rows_of(flt["start_out"], flt["obs_out"])
    split = [(int(b), int(f)) for b, f in flt["split_out"]]
    world, reason = triangulate_rows(px, poses, kept, hi - lo)
    return SimpleNamespace(poses=poses, rows=kept, split=split, world=world, reason=reason, view_range=(lo, hi), filter=flt)


def triangulate_rows(px, poses, rows, n_views=0xFFFFFFFF):
    """the world table of a list of rows: triangulate_landmark_robust of every row -> (world [n][4], reason [n])"""
    start = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint32)
    obs = np.array([o for r in rows for o in r], np.uint32).reshape(-1, 2)
    t = TS.Table(CAP, CAM6, px, np.asarray(poses, np.float64).reshape(-1, 12), start, obs, len(obs))
    got = TS.landmarks(t, TS.Settings())
    return np.array([r.point for r in got]).reshape(-1, 4), np.array([r.reason for r in got], np.uint8)


def map_of(rows):
    """the per-feature landmark map of a table"""
    m = np.full((N_VIEWS, CAP), NONE, np.uint32)
    for l, row in enumerate(rows):
        for b, f in row:
            m[b, f] = min(int(m[b, f]), l)
    return m


# ------------------------------------------------------------------------------------------------------------ phase 2: grow
def register(w, state, frames, stored, view_range, regenerated=True):
    """What Registration.sharing_view -> consensus -> refine -> landmark_table.add_views_and_regenerate do for one batch of
    frames against the reconstruction `state` (what start() or an earlier register() returned) -> the next state"""
    bear = bearings_of(w)
    px = state.px
    rows, poses, world = state.rows, state.poses, state.world
    n_world = len(rows)
    # the matcher's tables over the reconstruction's per-feature landmark map; no feature names two landmarks, so the mask of
    # the merge candidates is empty
    best, decision = matcher_tables(w, frames, stored, map_of(rows))
    mask = LT.sharing_mask(rows, best, decision, n_world)
    assert not np.any(mask)
    F = len(frames)
    matches, nmatches = np.zeros((F, CAP, 2), np.uint32), np.zeros(F, np.uint32)
    final, verdict, pose_out = np.zeros((F, CAP), np.uint8), np.zeros(F, np.uint32), np.zeros((F, 12))
    for f, frame in enumerate(frames):
        # matcher -> consensus: a pair is (the frame's feature, a row of the world table); rows without a robust point drop out
        pairs = MS.landmark_pairs(best[f], decision[f], None, world, n_world, n_world + f * CAP)
        original = MS.landmark_pairs(best[f], decision[f], None, None, n_world, n_world + f * CAP)
        b, x = bear[frame][pairs[:, 0]], world[pairs[:, 1]]
        res = _consensus("p3p", f, b, x, p3p_provider(b, x), SETTINGS["p3p"], True)
        # consensus -> refinement: the inliers index the pairs WITH a world point; the pose is the frame's WorldToCamera pose;
        # the other observations of a match are its landmark's row under the views' current poses
        others = [[(poses[v].reshape(3, 4), bear[v][j]) for v, j in rows[l]] for _, l in original]
        wpts = np.array([world[l] for _, l in original]).reshape(-1, 4)
        out = SV.refine(bear[frame][original[:, 0]], wpts, others, res.pose, res.inliers, SV.settings(**SETTINGS["single_view"]),
                        has_model=res.best_id != NONE)
        verdict[f] = out["verdict"]
        nmatches[f] = len(original)
        matches[f, :len(original)] = original
        if out["final"] is not None:
            final[f, :len(original)] = out["final"]
        if out["pose"] is not None:
            pose_out[f] = out["pose"].reshape(12)
    assert list(verdict) == [SV.OK] * F, ("registration", list(verdict))
    # refinement -> add_views: the final matches name rows of the table the refinement read; the split list is the filter's
    start = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint32)
    obs = np.array([o for r in rows for o in r], np.uint32).reshape(-1, 2)
    split = np.array(state.split, np.uint32).reshape(-1, 2)
    inp = dict(start=start, obs=obs, n_obs=len(obs), n_landmarks=n_world, n_world=n_world, split=split if len(split) else None,
               split_count=[len(split)], split_room=len(split), cap=CAP, n_blocks=N_VIEWS, ik=np.array(frames, np.uint32), n_frames=F,
               counts=w.counts, matches=matches, nmatches=nmatches, final=final, verdict=verdict, pose_out=pose_out, best=best, skip=None)
    added = LT.add_views(inp)
    assert added["frame_verdict"] == [LT.OK] * F and added["call_verdict"] == LT.OK, added["frame_verdict"]
    poses = poses.copy()
    for blk, slot in added["poses"].items():
        poses[blk] = pose_out[slot]
    new_rows = [list(r) for r in added["rows"]]
    if not regenerated:                                  # add_views alone: the destination's side of a bridging frame
        return SimpleNamespace(poses=poses, rows=new_rows, table_rows=new_rows, table_map=map_of(new_rows), px=px, split=[], n_world=n_world,
                               matches=matches, nmatches=nmatches, final=final, best=best, tombstones=[l for l in range(n_world) if rows[l] and not new_rows[l]])
    out = regenerate(w, px, poses, new_rows, list(range(*view_range)), view_range)
    out.table_rows, out.table_map, out.px = new_rows, map_of(new_rows), px
    out.tombstones = [l for l in range(n_world) if rows[l] and not new_rows[l]]
    out.views = sorted({b for r in out.rows for b, _ in r})
    return out


def regenerate(w, px, poses, rows, targets, view_range, strict=True):
    """reconstruction.regenerate: the robust triangulation of the table -> the covisibility candidates of the targets -> their
    three-view constraints -> the record -> the pose graph, the filter and the world table (_optimize)"""
    bear = TS.calibrate(px[..., 0], px[..., 1], CAM6)
    _, reason = triangulate_rows(px, poses, rows)
    start = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint32)
    obs = np.array([o for r in rows for o in r], np.uint32).reshape(-1, 2)
    cvs = SETTINGS["covisibility"]
    p = CV.settings(min_cov=cvs["optimization_robust_covisibility_minimum_landmarks"], min_lm=cvs["optimization_minimum_landmarks"])
    cand = CV.candidates(start, obs, reason, targets, N_VIEWS, CAP, p)
    # candidates -> constraints: slot k is the triple views[k] (ascending blocks) with the features lm[lm_start[k] : lm_start[k + 1]],
    # one column per view of the triple; the constraint's poses take the FIRST view's camera frame to the second's and third's
    tcs = dict(SETTINGS["constraint"], optimization_minimum_landmarks=cvs["optimization_minimum_landmarks"])
    results = []
    for k, tv in enumerate(cand["views"]):
        feats = cand["lm"][cand["lm_start"][k]:cand["lm_start"][k + 1]]
        lms = [[bear[tv[i]][row[i]] for i in range(3)] for row in feats]
        results.append(TC.constraint([poses[v].reshape(3, 4) for v in tv], lms, tcs))
    verdicts = [r["verdict"] for r in results]
    recorded, target_verdict, _ = CV.record(verdicts, targets, cand["verdict"], list(view_range), p)
    constraints = [(cand["views"][k], results[k]["poses"][0], results[k]["poses"][1]) for k in range(len(results)) if recorded[k] == 0]
    kps = np.zeros((N_VIEWS, CAP), np.dtype([("x", np.float32), ("y", np.float32)]))
    kps["x"], kps["y"] = px[..., 0], px[..., 1]
    out = _optimize(px, kps, poses, rows, constraints, view_range, strict)
    out.n_constraints, out.target_verdict = len(constraints), target_verdict
    return out


# ------------------------------------------------------------------------------------------------------------ phase 3: merge
MERGED_VIEWS = (0, 13)                                   # B's range takes the bridging frame's block behind its own: [6, 13)
B_WITH_BRIDGE = (6, 13)


def normalize(w, state, view_range):
    """normalize_reconstruction: the reconstruction's first view becomes the origin and the mean distance of its robust
    landmarks 1; the world table is that of the same rows under the new poses"""
    views = list(range(*view_range))
    got = RM.normalize(views, w.counts, map_of(state.rows), state.world, state.poses, np.zeros((0, 2, 12)), CAP, N_VIEWS)
    assert got["verdict"] == RM.NR_OK
    world, reason = triangulate_rows(state.px, got["poses"], state.rows)
    out = SimpleNamespace(**vars(state))
    out.poses, out.world, out.reason = got["poses"], world, reason
    return out


NORMALIZE = True


def merge(w, grown_a, grown_b, alter=(), register_with=None):
    """The bridging frame is registered in B (add_views_and_regenerate over [6, 13)) and in A (add_views alone) — by register(),
    or by `register_with` where a caller brings its own form of it —, then what
    reconstruction.merge_reconstructions does: the landmark map of the frame's final matches -> incorporate B into A under
    inverse(src_pose) * dst_pose -> regenerate over [0, 13) with B's views as targets.
    -> (B with the frame, A with the frame, the merged state)"""
    reg = register_with or register
    if NORMALIZE:
        grown_a, grown_b = normalize(w, grown_a, A_VIEWS), normalize(w, grown_b, B_VIEWS)
    b = reg(w, grown_b, [BRIDGE], list(range(*B_VIEWS)), B_WITH_BRIDGE)
    # B -> merge: the frame's pose IN B, taken before A's add_views overwrites the block's row; B's per-feature landmark map
    src_pose, src_map, src_rows = b.poses[BRIDGE].copy(), b.table_map, b.table_rows
    a = reg(w, grown_a, [BRIDGE], list(range(*A_VIEWS)), A_VIEWS, regenerated=False)
    if "src_pose_from_a" in alter:
        src_pose = a.poses[BRIDGE].copy()
    # A's refinement -> the map: a final match of the frame's feature j on A's row l, where B's map knows j, pairs B's row with l
    n = int(a.nmatches[0])
    # (a merged match, row >= n_world, stands for its two landmarks: the map takes the first, which add_views kept)
    named = {int(j): [int(l) if l < a.n_world else int(a.best[0, j, 0, 0])] for (j, l), ok in zip(a.matches[0, :n], a.final[0, :n]) if ok}
    view_lms = [None if int(l) == NONE else int(l) for l in src_map[BRIDGE]]
    pairs = RM.merge_map(named, view_lms)
    poses = b.poses.copy()                               # one pool: B's rows as B left them, A's rows and the frame's as A left them
    poses[list(range(*A_VIEWS)) + [BRIDGE]] = a.poses[list(range(*A_VIEWS)) + [BRIDGE]]
    if "merge_transform_inverted" in alter:              # T = inverse(src) * dst; the exchange of the two is its inverse
        src_pose, poses[BRIDGE] = poses[BRIDGE].copy(), src_pose
    src_blocks = list(range(*B_VIEWS))
    inc = RM.incorporate(a.table_rows, src_rows, pairs, src_blocks, BRIDGE, src_pose, poses, CAP, N_VIEWS)
    assert inc["verdict"] == RM.OK, ("incorporate", inc["verdict"])
    merged_poses = inc["poses"].copy()
    if "merge_transform_inverted" in alter:
        merged_poses[BRIDGE] = a.poses[BRIDGE]
    rows = [list(r) for r in inc["rows"]]
    out = regenerate(w, a.px, merged_poses, rows, src_blocks, MERGED_VIEWS, strict=not alter)
    out.table_rows, out.table_map, out.px, out.tombstones = rows, map_of(rows), a.px, []
    out.views = sorted({v for r in out.rows for v, _ in r})
    out.applied, out.pairs = inc["counts"][2], pairs
    return b, a, out


def relative_scale(state, w):
    """the scale of the similarity fitted to the merged map's B views over that fitted to its A views: the truth's is 1"""
    scales = []
    for lo, hi in (A_VIEWS, B_VIEWS):
        views = list(range(lo, hi))
        c_est = np.stack([-state.poses[v].reshape(3, 4)[:, :3].T @ state.poses[v].reshape(3, 4)[:, 3] for v in views])
        c_true = np.stack([-w.poses[v][:, :3].T @ w.poses[v][:, 3] for v in views])
        scales.append(umeyama(c_est, c_true)[0])
    return scales[1] / scales[0]


def shared_points_are_one_landmark(w, state):
    """every point seen from both sides: the live rows that hold its observations -> (merged into one row, left as two or more
    rows — a documented non-merge: the frame did not match it —, pairs of live rows of one point that SHARE A VIEW: never)"""
    one = many = sharing = 0
    for p, kind in enumerate(w.kinds):
        if kind != "both":
            continue
        rows = [r for r in state.rows if len(r) > 1 and any(w.point_of[b][f] == p for b, f in r)]
        one, many = one + (len(rows) == 1), many + (len(rows) > 1)
        sharing += sum(1 for i in range(len(rows)) for j in range(i) if {b for b, _ in rows[i]} & {b for b, _ in rows[j]})
    return one, many, sharing


# ------------------------------------------------------------------------------------------------------------ phase 4: export
def export(w, merged, alter=()):
    """export_reconstruction on the merged, filtered table -> export_statement's dict: the cameras' vertices, then the points
    with the colour of their row's first observation"""
    rows = merged.rows
    if "colour_of_last_observation" in alter:
        rows = [r[::-1] for r in rows]
    return EX.export(merged.world, rows, w.colours, list(range(N_VIEWS)), w.counts, merged.table_map, merged.poses, CAP, N_VIEWS, len(merged.world))


def exported_errors(w, merged, xyz, rgb, keys, similarity):
    """the file's vertices against the truth under the merged phase's similarity: the worst camera-centre distance over the
    longest baseline, the worst point distance over depth, and the points whose colour is not their first observation's"""
    s, r, t = similarity
    centres = xyz[0:5 * N_VIEWS:5]
    c_true = np.stack([-p[:, :3].T @ p[:, 3] for p in w.poses])
    baseline = max(float(np.linalg.norm(a - b)) for a in c_true for b in c_true)
    centre = float(np.linalg.norm(centres @ r.T * s + t - c_true, axis=1).max()) / baseline
    truth = truth_of(w, merged.rows, merged.views)
    pts, worst, wrong = xyz[5 * N_VIEWS:], 0.0, 0
    for k, key in enumerate(keys):
        key = int(key)
        b, f = merged.rows[key][0]
        wrong += tuple(int(c) for c in rgb[5 * N_VIEWS + k]) != tuple(int(c) for c in w.colours[b][f])
        p = truth.row_point[key]
        if p >= 0 and merged.reason[key] == 0:
            worst = max(worst, float(np.linalg.norm(s * r @ pts[k] + t - w.points[p]) / np.linalg.norm(w.points[p] - c_true.mean(0))))
    return dict(centre=centre, point=worst, wrong_colours=wrong)


# ------------------------------------------------------------------------------------------------------------ the life
SCENES = dict(exact=(0.0, 0.0), noisy=(0.5, 0.1))        # (pixel noise, the share of every designed list that is wrong)
SEEDS = dict(exact=(1, 2, 3), noisy=(9, 10, 11))          # worlds the chain of statements carries through inside the caps
LEFT_OUT_CAP = dict(exact=0.20, noisy=0.35)              # truth points with at least three observations a comparison may leave out
VIEWS_AFTER = dict(start=3, grow=6, bridge=7, merge=13)  # no view may be left out
PHASES = ("start", "grow", "bridge", "merge", "export")
SHARED_MERGED_AT_LEAST = dict(exact=40, noisy=30)        # of the 48 points seen from both sides: the rest are documented non-merges
# The worst error of the chain of statements (this module, on the CPU) against the ground truth over the scene's three seeds and
# both reconstructions, per phase and error kind, as measure() printed it, rounded up.  A BOUND is four times the entry: the
# factor covers equally valid discrete choices (inlier sets, filter kicks) and summation orders in optimisers that stop on
# patience; a convention mistake moves a pose by the size of the scene.  rotation: radians; centre: over the longest baseline;
# point: over the point's distance from the middle of the views; scale: |ln| of the B views' fitted scale over the A views'.
BOUNDS = dict(
    exact=dict(
        start=dict(rotation=3.101e-05, centre=1.064e-04, point=1.730e-05),
        grow=dict(rotation=8.687e-05, centre=1.107e-04, point=2.818e-05),
        bridge=dict(rotation=8.550e-05, centre=1.077e-04, point=2.770e-05),
        merge=dict(rotation=4.401e-03, centre=1.337e-02, point=2.235e-02, scale=4.464e-02),
        export=dict(centre=1.337e-02, point=2.235e-02),
    ),
    noisy=dict(
        start=dict(rotation=3.422e-02, centre=1.163e-01, point=3.869e-02),
        grow=dict(rotation=5.895e-02, centre=7.429e-02, point=4.469e-02),
        bridge=dict(rotation=1.966e-02, centre=2.618e-02, point=1.466e-02),
        merge=dict(rotation=6.653e-02, centre=6.638e-02, point=4.870e-02, scale=9.649e-02),
        export=dict(centre=6.638e-02, point=4.870e-02),
    ),
)


def life(w, alter=()):
    """both reconstructions of a world through the phases -> {(side, phase): state}"""
    out = {}
    for side, triple, frames, view_range in (("A", A_START, A_GROW, A_VIEWS), ("B", B_START, B_GROW, B_VIEWS)):
        out[side, "start"] = start(w, triple, view_range[0], alter)
        out[side, "grow"] = register(w, out[side, "start"], frames, out[side, "start"].views, view_range)
    out["B", "bridge"], _, out["AB", "merge"] = merge(w, out["A", "grow"], out["B", "grow"], alter)
    return out


RANGES = dict(A=A_VIEWS, B=B_VIEWS, AB=MERGED_VIEWS)


def errors_of(w, states):
    """{(side, phase): aligned_errors and the broken invariants}; the export's errors under the merge's similarity"""
    got = {}
    for (side, phase), st in states.items():
        view_range = B_WITH_BRIDGE if phase == "bridge" else RANGES[side]
        e = aligned_errors(st.poses, st.world, st.reason, truth_of(w, st.rows, st.views))
        e["broken"] = invariants(st.table_rows, view_range, st.table_map, getattr(st, "tombstones", ())) + invariants(st.rows, view_range)
        e["views"] = len(st.views)
        got[side, phase] = e
    m = states["AB", "merge"]
    ex = export(w, m)
    e = exported_errors(w, m, ex["vertices"], np.array(ex["colors"]), ex["keys"], got["AB", "merge"]["similarity"])
    got["AB", "export"] = dict(e, rotation=0.0, left_out=got["AB", "merge"]["left_out"], broken=[], views=N_VIEWS, similarity=got["AB", "merge"]["similarity"])
    got["AB", "merge"]["scale"] = abs(math.log(relative_scale(m, w)))
    got["AB", "merge"]["shared"] = shared_points_are_one_landmark(w, m)
    return got


def measure(scene):
    """the worst error of the chain of statements over the scene's seeds and both reconstructions, per phase and error kind:
    what BOUNDS holds (a bound is four times it)"""
    worst = {p: dict(rotation=0.0, centre=0.0, point=0.0, left_out=0.0) for p in PHASES}
    worst["merge"]["scale"] = 0.0
    for seed in SEEDS[scene]:
        w = world(seed, *SCENES[scene])
        for (side, phase), e in errors_of(w, life(w)).items():
            assert not e["broken"], (seed, side, phase, e["broken"])
            for k in worst[phase]:
                worst[phase][k] = max(worst[phase][k], e[k])
            if phase == "merge":
                print(scene, seed, "shared points (one row, several rows, rows sharing a view)", e["shared"], "scale", e["scale"])
    return worst


if __name__ == "__main__":
    import sys
    import time
    for scene in sys.argv[1:] or SCENES:
        t = time.time()
        print(scene, {p: {k: float("%.3e" % v) for k, v in m.items()} for p, m in measure(scene).items()}, "%.0f s" % (time.time() - t), flush=True)
