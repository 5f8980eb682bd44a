"""The host build of include/akz_triangulate_math.h (tests/triangulate_checker.py) held to the independent float64 statement of
the triangulation stage (tests/triangulate_statement.py) on the whole catalogue: reason bytes and the set of rows written
equal, points within the statement's bound; every alteration of the statement shown to be caught; the statement's calibrate
held to a projection written out by hand.  tests/test_gpu_triangulate_statement.py holds the device to the same statement."""
import functools
import itertools

import numpy as np

import triangulate_checker as tc
import triangulate_statement as S

POISON = 7.25


def kps_of(xy):
    """[.., 2] float32 pixels -> akz_keypoint records"""
    k = np.zeros(xy.shape[:-1], tc.KP_DTYPE)
    k["x"], k["y"] = xy[..., 0], xy[..., 1]
    return k


def host_settings(st):
    return tc.settings(st.eps, st.max_sweeps, st.robust_minimum_observations, st.n_views, st.min_cos)


def grid_settings(rmo_views, min_cos=1e-3, **kw):
    return S.Settings(robust_minimum_observations=rmo_views[0], n_views=rmo_views[1], min_cos=min_cos, **kw)


@functools.lru_cache(maxsize=None)
def catalogue():
    """everything the two test files share, made once: the tables, what the statement prepares of them, the thresholds"""
    t = S.table(513)
    pre = S.prepare_landmarks(t)
    chosen, values = S.thresholds(t, pre)
    mc = S.merge_case()
    return dict(table=t, prepared=pre, chosen=chosen, thresholds=values, merge=mc, merge_prepared=S.prepare_merged(mc),
                pairs=S.pair_case(), lists={n: S.list_case(n) for n in (0, 1, 2, 3, 48)})


def landmark_names(n, what):
    return [f"landmarks/{what}/l={l}" for l in range(n)]


def host_landmarks(t, st, n=None):
    n = t.n_landmarks if n is None else n
    return tc.landmarks(kps_of(t.xy), t.poses, tc.camera(*t.cam), t.start[:n + 1], t.obs, st=host_settings(st), n_obs=t.n_obs)


def host_merged(mc, st):
    """-> (world, reason [F, cap]) of a poisoned table"""
    t = mc.table
    world = np.full((mc.n_world + mc.decision.size, 4), POISON)
    reason = tc.merged(kps_of(t.xy), t.poses, tc.camera(*t.cam), t.start, t.obs, mc.best, mc.decision, mc.merge_ok, mc.n_world, world,
                       st=host_settings(st), n_obs=t.n_obs)
    return world, reason


def judge_merged(mc, world, reason, rows, what):
    """the rows written are the statement's and no others; -> (names, points, reasons) in the statement's order"""
    keys = sorted(rows)
    written = {(int(f), int(j)) for f, j in np.argwhere(reason != 255)}
    assert written == set(keys), (what, sorted(written ^ set(keys))[:5])
    at = np.array([mc.row_of(f, j) for f, j in keys], np.int64)
    rest = np.ones(len(world), bool)
    rest[at] = False
    assert (world[rest] == POISON).all(), what
    names = [f"merged/{what}/f={f},j={j}" for f, j in keys]
    return names, world[at], np.array([reason[k] for k in keys]), [rows[k] for k in keys]


def host_pairs(pc, st):
    """(scene, i) -> (point, reason) for the rows the host build writes"""
    ka, kb = kps_of(pc.xy_a), kps_of(pc.xy_b)
    out = {}
    for s in range(len(pc.npairs)):
        if int(pc.best_id[s]) == S.NO_ID:
            continue
        pts, why = tc.pairs_scene(ka[pc.ia[s]], kb[pc.ib[s]], pc.pairs[s], pc.npairs[s], tc.camera(*pc.cam_a), tc.camera(*pc.cam_b),
                                  pc.pose[s], pc.inliers[s], st=host_settings(st), n_inliers=pc.n_inliers[s])
        for i in range(len(pts)):
            out[(s, i)] = (pts[i], why[i])
    return out


def judge_pairs(got, rows, what):
    assert set(got) == set(rows), (what, sorted(set(got) ^ set(rows))[:5])
    keys = sorted(rows)
    return [f"pairs/{what}/s={s},i={i}" for s, i in keys], [got[k][0] for k in keys], [got[k][1] for k in keys], [rows[k] for k in keys]


def landmark_runs(cat):
    """(name, Settings) of every launch of the landmark sweep: settings_grid x thresholds"""
    return [(f"need={rv[0]},views={rv[1]:#x},thr={thr!r}", grid_settings(rv, thr)) for rv in S.SETTINGS_GRID for thr in cat["thresholds"]]


def test_host_build_agrees_on_the_landmark_table():
    """tc.landmarks == the statement on table(513) under every element of settings_grid x thresholds (132 runs, every run
    judged over all 513 rows), on the prefixes 1, 255, 256, 257, and under a sweep limit of 1.  Reasons 0, 1, 2, 4, 5, 6 all
    occur, 3 under the sweep limit; each of the 16 chosen landmarks flips between its two thresholds; at least eight landmarks
    are robust only through a pair without observation 0.
    Worst sin(angle) / bound of the host build, measured: 3.3e-4 (the bound is not tightened to it)."""
    cat = catalogue()
    t, pre = cat["table"], cat["prepared"]
    n = t.n_landmarks
    worst, hist = 0.0, np.zeros(7, np.int64)
    reasons_at = {}
    for what, st in landmark_runs(cat):
        rows = S.landmarks(t, st, prepared=pre)
        world, reason = host_landmarks(t, st)
        worst = max(worst, S.hold(landmark_names(n, what), world, reason, rows, st))
        hist += np.bincount(reason, minlength=7)
        reasons_at[(st.robust_minimum_observations, st.n_views, st.min_cos)] = reason
    print("reasons 0..6 over the sweep:", hist.tolist())
    assert (hist[[0, 1, 2, 4, 5, 6]] > 0).all() and hist[3] == 0
    for l in cat["chosen"]:
        lo, hi = S.around(pre[l].best)
        assert reasons_at[(3, 0xFFFFFFFF, lo)][l] != 2 and reasons_at[(3, 0xFFFFFFFF, hi)][l] == 2, l
    print("threshold flips:", len(cat["chosen"]), "of", len(cat["chosen"]))
    bests = [p.best for p in pre if np.isfinite(p.best)]
    print(f"best pair distances {min(bests):.3g} .. {max(bests):.3g}")
    assert min(bests) < 1e-9 and max(b for b in bests if b < 1.0) > 1e-2
    first_only = S.landmarks(t, S.Settings(), alter=("pairs_with_first_only",))
    default = reasons_at[(3, 0xFFFFFFFF, 1e-3)]
    only_later = [l for l in range(n) if default[l] == 0 and first_only[l].reason == 2]
    print("robust only through a pair without observation 0:", only_later)
    assert len(only_later) >= 8 and set(t.tags["only_pair_1_2"]) <= set(only_later)
    lens = np.diff(t.start.astype(np.int64))
    for w0 in range(0, n - 63, 64):
        assert set(S.LIST_LENGTHS) <= set(lens[w0:w0 + 64].tolist()), w0
    for k in (1, 255, 256, 257):
        world, reason = host_landmarks(t, S.Settings(), n=k)
        S.hold(landmark_names(k, f"prefix {k}"), world, reason, S.landmarks(t, S.Settings(), n_landmarks=k, prepared=pre), S.Settings())
    st1 = S.Settings(max_sweeps=1)
    world, reason = host_landmarks(t, st1)
    S.hold(landmark_names(n, "one sweep"), world, reason, S.landmarks(t, st1, prepared=pre), st1)
    assert (reason == 3).sum() == (default == 0).sum() + (default == 5).sum() > 0
    print(f"worst sin(angle) / bound of the host build: {worst:.3g}")


MERGE_SETTINGS = (("default", S.Settings()), ("need=3,views=2", grid_settings((3, 2))))


def test_host_build_agrees_on_the_merge_candidates():
    """tc.merged == the statement on merge_case() under the default settings and under (3, 2): the rows written, their reasons
    and points; the designed slots decide as designed.  Worst sin(angle) / bound of the host build, measured: 3.4e-4."""
    cat = catalogue()
    mc, pre = cat["merge"], cat["merge_prepared"]
    worst = 0.0
    seen = {}
    for what, st in MERGE_SETTINGS:
        rows = S.merged(mc, st, prepared=pre)
        world, reason = host_merged(mc, st)
        names, pts, why, rws = judge_merged(mc, world, reason, rows, what)
        worst = max(worst, S.hold(names, pts, why, rws, st))
        seen[what] = {k: r.reason for k, r in rows.items()}
        print(what, "rows", len(rows), "reasons 0..6:", np.bincount(why, minlength=7).tolist())
    d, v2 = seen["default"], seen["need=3,views=2"]
    tag = mc.tags
    assert any(j >= 256 for _, j in d) and len({f for f, _ in d}) == 3
    assert d[tag["cross_pair_only"]] == 0 and d[tag["cross_pair_only_swapped"]] == 0          # neither side alone is robust
    lm = S.landmarks(mc.table, S.Settings())
    assert all(lm[l].reason == 2 for l in mc.table.tags["narrow_side"] + mc.table.tags["one_block_twice"])
    assert d[tag["same_block_singles"]] == 2 and v2[tag["same_block_singles"]] == 2
    assert d[tag["wide_singles"]] == 2 and v2[tag["wide_singles"]] == 0
    assert d[tag["empty_then_robust"]] == 0 and d[tag["robust_then_empty"]] == 0
    # (the rule is monotone — a robust side makes the concatenation robust — so a merge with a robust side fails only later)
    assert d[tag["robust_then_behind"]] == 5 and d[tag["robust_then_bad_index"]] == 6 and d[tag["robust_then_nan"]] == 4
    assert d[tag["first_key_is_n_landmarks"]] == 6 and d[tag["second_key_is_none"]] == 6
    # two narrow lists of DIFFERENT points: the pairs across them are wide, the merge is robust and goes to the solver
    assert d[tag["narrow_then_narrowest"]] in (0, 5) and d[tag["last_landmark_leaves_the_array"]] == 6
    assert tag["not_admitted"] not in d and tag["not_a_candidate"] not in d
    print(f"worst sin(angle) / bound of the host build: {worst:.3g}")


def test_host_build_agrees_on_the_two_view_inliers_and_the_single_lists():
    """tc.pairs_scene == the statement on pair_case() (the rows written: the clamps of n_inliers and npairs, the scene without
    a model; reason 6 for an inlier index or a feature outside), tc.observations on list_case(n), n = 0, 1, 2, 3, 48.
    Worst sin(angle) / bound of the host build, measured: 2.3e-4 on the two-view inliers, 1.7e-4 on the single lists.
    Reason 5 occurs on 90 of the inliers (baselines of 0.03 and 0.01 units under half a pixel of noise); smallest
    (l2 - l1) / l4 2.1e-5."""
    cat = catalogue()
    pc = cat["pairs"]
    st = S.Settings()
    rows = S.pairs(pc, st)
    names, pts, why, rws = judge_pairs(host_pairs(pc, st), rows, "default")
    worst = S.hold(names, pts, why, rws, st)
    hist = np.bincount(why, minlength=7)
    per_scene = [sum(1 for s, _ in rows if s == k) for k in range(5)]
    print("rows per scene", per_scene, "reasons 0..6:", hist.tolist(), "smallest gap %.3g" % min(r.gap for r in rws if r.lam is not None))
    assert per_scene == [0, 1, 256, 0, 300] and hist[0] > 400 and hist[5] > 0 and hist[6] >= 8 and hist[[1, 2, 3]].sum() == 0
    assert rows[(1, 0)].reason == 0 and rows[(2, 3)].reason == 6 and rows[(4, 0)].reason == 6
    for n, (P, B) in cat["lists"].items():
        row = S.observations(P, B, st)
        p, r = tc.observations(P, B, st=host_settings(st))
        worst = max(worst, S.hold([f"list/n={n}"], [p], [r], [row], st))
        assert row.reason == (1 if n < 2 else 0), n
    print(f"worst sin(angle) / bound of the host build: {worst:.3g}")


@functools.lru_cache(maxsize=None)
def host_answers():
    """What the host build says on the runs the alterations are tried on: name of the run -> (names, points, reasons)"""
    cat = catalogue()
    t, mc, pc = cat["table"], cat["merge"], cat["pairs"]
    out = {}
    runs = [(f"need={rv[0]},views={rv[1]:#x}", grid_settings(rv)) for rv in S.SETTINGS_GRID]
    runs += [(f"thr={thr!r}", S.Settings(min_cos=thr)) for thr in cat["thresholds"]]
    for what, st in runs:
        out[("landmarks", what)] = (st, host_landmarks(t, st))
    for what, st in MERGE_SETTINGS:
        out[("merged", what)] = (st, host_merged(mc, st))
    out[("pairs", "default")] = (S.Settings(), host_pairs(pc, S.Settings()))
    return out


def first_disagreement(alter):
    """the first named case on which the host build and the statement switched to `alter` disagree, or None"""
    cat = catalogue()
    t, mc, pc = cat["table"], cat["merge"], cat["pairs"]
    pre, mpre = S.prepare_landmarks(t, alter), S.prepare_merged(mc, alter)
    for (kind, what), (st, got) in host_answers().items():
        if kind == "landmarks":
            bad, _ = S.disagreements(landmark_names(t.n_landmarks, what), got[0], got[1], S.landmarks(t, st, alter, prepared=pre))
        elif kind == "merged":
            rows = S.merged(mc, st, alter, prepared=mpre)
            keys = sorted(rows)
            at = [mc.row_of(f, j) for f, j in keys]
            bad, _ = S.disagreements([f"merged/{what}/f={f},j={j}" for f, j in keys], got[0][at], [got[1][k] for k in keys],
                                     [rows[k] for k in keys])
        else:
            rows = S.pairs(pc, st, alter)
            keys = sorted(rows)
            bad, _ = S.disagreements([f"pairs/{what}/s={s},i={i}" for s, i in keys], [got[k][0] for k in keys],
                                     [got[k][1] for k in keys], [rows[k] for k in keys])
        if bad:
            return bad[0]
    return None


def test_every_alteration_is_caught():
    """With the statement switched to each of its named wrong rules, the host build disagrees with it on at least one named
    case of the catalogue; unswitched, on none (the tests above)."""
    assert first_disagreement(()) is None
    for alter in S.ALTERATIONS:
        found = first_disagreement((alter,))
        print(f"{alter}: caught at {found}")
        assert found is not None, alter


def project_by_hand(cam, x, y):
    """normalised image point -> pixel: the distorted point is the fixed point of x_d = x (1 + k1 r_d^2), the pixel
    (fx x_d + skew y_d + cx, fy y_d + cy)"""
    fx, fy, cx, cy, skew, k1 = cam
    xd, yd = x, y
    if k1 is not None:
        for _ in range(200):
            g = 1.0 + k1 * (xd * xd + yd * yd)
            xd, yd = x * g, y * g
    return fx * xd + skew * yd + cx, fy * yd + cy


def test_calibrate_round_trip_by_hand():
    """pixel (an exact float32) -> calibrate -> normalised point -> the projection by hand -> the pixel again, within 1e-12
    in normalised coordinates; with and without K1 and skew."""
    rng = np.random.default_rng(0xCA1)
    worst = 0.0
    for cam in (S.CAM, S.CAM_NO_K1, (1000.0, 1000.0, 960.0, 540.0, 0.0, None), (950.0, 955.0, 640.0, 250.0, 0.0, -0.05)):
        for px, py in itertools.chain([(cam[2], cam[3]), (0.0, 0.0)], rng.uniform(0, 1300, (500, 2))):
            px, py = np.float32(px), np.float32(py)
            b = S.calibrate(px, py, cam)
            assert abs(np.linalg.norm(b) - 1.0) < 1e-15
            qx, qy = project_by_hand(cam, b[0] / b[2], b[1] / b[2])
            worst = max(worst, abs(qx - float(px)) / cam[0], abs(qy - float(py)) / cam[1])
    print("worst round trip, normalised:", worst)
    assert worst <= 1e-12
