"""The life of tests/reconstruction_life_statement.py with the matcher in the loop: the world gets descriptors, and every matcher
output the designed life set by hand is SEARCHED for — the bootstrap's pair lists by the symmetric better-by-24 match, a
frame's best / decision tables by the k = 3 searches and best-of-views over the landmark map the phase before WROTE
(add_reconstruction's landmarks_out, then add_views'), the merge candidates by the share test, their rows by the merged
triangulation, the consensus' order by the observation counts the phase before wrote.  Each side grows in two calls: one frame
against the three start views (a single frame's merges are applied, as add_view does), then two frames against four stored
views, the one just added among them (two frames that name one landmark pair: the demotion rule).

numpy and the statement modules only, as the designed life.  What is new here is again GLUE, and SEARCH_ALTERATIONS names four
deliberately wrong forms of it; tests/test_searched_life.py shows what catches each.

HANDOVER names which landmark map and observation counts a call reads: "documented" — the ones add_views / add_reconstruction
wrote BEFORE the observation filter ran, which is what the device chain has (a feature the filter split off still maps to
its old landmark) — or "filtered", the map and lengths of the filtered rows (what the reference has: split_observation gives
the feature a new landmark at once).  measure(scene, handover) runs either (`python searched_life_statement.py filtered noisy`);
DESIGN.md section 7 has the figures.
"""
from types import SimpleNamespace

import numpy as np

import landmark_table_statement as LT
import matching_statement as M
import reconstruction_life_statement as L
import single_view_statement as SV
import triangulate_statement as TS

NONE, CAP, N_VIEWS = L.NONE, L.CAP, L.N_VIEWS
BETTER_BY = 24
LATE = 16                                                # appended points per side
SEARCH_ALTERATIONS = ("map_one_generation_old", "view_sel_permuted", "merged_row_transposed", "mask_of_the_other_frame")


# ------------------------------------------------------------------------------------------------------------ the world
def searched_world(seed, noise, wrong_share):
    """world() — unchanged, its random stream untouched — and behind its 216 points LATE more per side that the first and second
    view of the side's triple and its grow frames see but the centre does not: add_reconstruction gives such a point one
    single-observation landmark per view, which a grow frame's search then finds as a merge candidate.  Every fourth of them is
    not seen by the first grow frame but by the bridging frame: the two frames of the second call both name its pair, the
    merge is demoted, and the bridging frame finds a candidate of four observations — the only kind whose merged row holds a
    point (a robust triangulation takes three observations; two single-observation landmarks have two).  descs [13][CAP][64]
    uint8: one random row per point with the pad bits 486..511 clear, every observation that row with 0 - 12 of the first 486
    bits flipped; wrong_share of a view's features carry ANOTHER feature's point row.  The additions draw from a stream of
    their own."""
    w = L.world(seed, noise, wrong_share)
    rng = np.random.default_rng([seed, 0x5EA2C4])
    n0, n = w.n_points, w.n_points + 2 * LATE
    late = np.stack([rng.uniform(-2.0, 2.0, 2 * LATE), rng.uniform(-1.2, 1.2, 2 * LATE), rng.uniform(5.2, 8.8, 2 * LATE)], 1)
    w.points = np.concatenate([w.points, late])
    w.feature = np.concatenate([w.feature, np.full((N_VIEWS, 2 * LATE), -1, np.int64)], 1)
    for k in range(2 * LATE):
        p, lo = n0 + k, (0 if k < LATE else 6)
        seen = [lo + 1, lo + 2] + ([lo + 3] if k % 4 != 3 else []) + [lo + 4, lo + 5] + ([L.BRIDGE] if k % 4 == 3 else [])
        w.seen.append(seen)
        w.kinds.append("late")
        for v in seen:
            x = w.poses[v][:, :3] @ w.points[p] + w.poses[v][:, 3]
            uv = np.array([L.CAM[0] * x[0] / x[2] + L.CAM[2], L.CAM[1] * x[1] / x[2] + L.CAM[3]]) + noise * rng.standard_normal(2)
            assert x[2] > 3.0 and uv.min() > 0 and uv[0] < 1280 and uv[1] < 720
            j = int(w.counts[v])
            w.px[v, j], w.feature[v, p], w.point_of[v, j] = uv, j, p
            w.counts[v] += 1
    w.n_points = n
    assert w.counts.max() <= CAP
    base = rng.integers(0, 256, (n, 64), dtype=np.uint8)
    base[:, 60] &= 0x3F                                  # bits 486..511: the upper two of byte 60 and bytes 61..63
    base[:, 61:] = 0
    w.descs = np.zeros((N_VIEWS, CAP, 64), np.uint8)
    w.desc_point = np.full((N_VIEWS, CAP), -1, np.int64)   # the point whose row a feature carries
    for v in range(N_VIEWS):
        c = int(w.counts[v])
        carried = w.point_of[v, :c].copy()
        wrong = rng.permutation(c)[:int(round(c * wrong_share))]
        carried[wrong] = carried[np.roll(wrong, 1)]
        w.desc_point[v, :c] = carried
        for j in range(c):
            w.descs[v, j] = M.flip(base[carried[j]], rng.permutation(486)[:int(rng.integers(0, 13))])
    return w


# ------------------------------------------------------------------------------------------------------------ the matcher
def searched_pair_lists(w, triple):
    """the lists (centre, first) and (centre, second) as hm_match_batch_device leaves them: symmetric, better-by 24, ascending
    centre feature -> pairs [2][cap][2] u32, npairs [2]"""
    c = triple[0]
    pairs, npairs = np.zeros((2, CAP, 2), np.uint32), np.zeros(2, np.uint32)
    for k, other in enumerate(triple[1:]):
        got = M.match(w.descs[c, :w.counts[c]], w.descs[other, :w.counts[other]], M.RULE_BETTER_BY, BETTER_BY, 0.0, True)
        pairs[k, :len(got)], npairs[k] = got, len(got)
    return pairs, npairs


def wrong_pairs(w, triple, pairs, npairs):
    """-> (entries that pair two different points, common points of a pair that its list lacks)"""
    c, wrong, missing = triple[0], 0, 0
    for k, other in enumerate(triple[1:]):
        got = {(int(i), int(j)) for i, j in pairs[k, :npairs[k]]}
        common = {(int(w.feature[c][p]), int(w.feature[other][p])) for p in range(w.n_points) if c in w.seen[p] and other in w.seen[p]}
        wrong, missing = wrong + len(got - common), missing + len(common - got)
    return wrong, missing


def searched_tables(w, frames, stored, landmark_map, alter=()):
    """best [F][cap][3][2] / decision [F][cap] as Registration.match_views leaves them: per frame the k = 3 neighbours of every
    feature in every stored view, in the order of `stored`, then best-of-views over the landmark map in the SAME order"""
    best = np.full((len(frames), CAP, 3, 2), NONE, np.uint32)
    decision = np.zeros((len(frames), CAP), np.uint32)
    view_sel = np.roll(stored, 1) if "view_sel_permuted" in alter else np.asarray(stored)
    for f, frame in enumerate(frames):
        nq = int(w.counts[frame])
        nb = np.zeros((len(stored), CAP, 3), M.NB)
        for k, v in enumerate(stored):                    # problem f * V + k of the knn call is (frame, stored[k])
            nb[k, :nq] = M.as_neighbors(*M.knn(w.descs[frame, :nq], w.descs[v, :w.counts[v]], 3), M.ABI_ABSENT)
        best[f, :nq], decision[f, :nq] = M.best_of_views(nb, nq, landmark_map, view_sel, w.counts, BETTER_BY)
    return best, decision


def csr(rows):
    start = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint32)
    return start, np.array([o for r in rows for o in r], np.uint32).reshape(-1, 2)


def merged_rows(px, poses, rows, best, decision, mask, world, n_world, alter=()):
    """the world table with the merge candidates' rows behind it: row n_world + f * cap + j = the robust triangulation of both
    landmarks' observations for slot f, feature j with decision 2 and the mask set; every other row behind n_world "None" """
    F = len(decision)
    transposed = "merged_row_transposed" in alter
    ext = np.zeros(((CAP if transposed else F) * CAP, 4))
    ext[:, 3] = -1.0
    start, obs = csr(rows)
    mc = TS.MergeCase(TS.Table(CAP, L.CAM6, px, np.asarray(poses, np.float64).reshape(-1, 12), start, obs, len(obs)), best, decision,
                      np.asarray(mask, np.uint8), n_world)
    for (f, j), row in TS.merged(mc).items():
        ext[j * CAP + f if transposed else f * CAP + j] = row.point
    return np.concatenate([np.asarray(world, np.float64).reshape(-1, 4)[:n_world], ext])


# ------------------------------------------------------------------------------------------------------------ what is handed over
def handed_over(state, handover):
    """(the per-feature landmark map, the observation count of every key) the next call reads"""
    if handover == "documented":
        return state.table_map, np.asarray(state.table_counts, np.uint32)
    assert handover == "filtered"
    return L.map_of(state.rows), np.array([len(r) for r in state.rows], np.uint32)


def start(w, triple, view_base, alter=()):
    lists = searched_pair_lists(w, triple)
    st = L.start(w, triple, view_base, alter, lists=lists)
    st.lists = lists
    return st


# ------------------------------------------------------------------------------------------------------------ one call
def register(w, state, frames, stored, view_range, regenerated=True, alter=(), handover="documented"):
    """Registration.match_views -> sharing_view -> triangulate_merged -> consensus(d_merge_ok, d_obs_counts) -> refine ->
    landmark_table.add_views_and_regenerate for one batch of frames against the reconstruction `state` -> the next state.  With
    an alteration a frame may be refused: it is then left out, as add_views leaves it out."""
    bear = L.bearings_of(w)
    px, rows, poses, world = state.px, state.rows, state.poses, state.world
    n_world, F, strict = len(rows), len(frames), not alter
    landmark_map, obs_counts = handed_over(state, handover)
    if "map_one_generation_old" in alter and getattr(state, "older", None) is not None:
        landmark_map, obs_counts = state.older
        obs_counts = np.concatenate([obs_counts, np.zeros(n_world, np.uint32)])[:n_world]
    best, decision = searched_tables(w, frames, stored, landmark_map, alter)
    share = np.array(LT.sharing_mask(rows, best, decision, n_world), np.uint8)
    mask = share[::-1].copy() if "mask_of_the_other_frame" in alter and F == 2 else share
    ext = merged_rows(px, poses, rows, best, decision, mask, world, n_world, alter)
    matches, nmatches = np.zeros((F, CAP, 2), np.uint32), np.zeros(F, np.uint32)
    final, verdict, pose_out = np.zeros((F, CAP), np.uint8), np.zeros(F, np.uint32), np.zeros((F, 12))
    pairs_of = []
    for f, frame in enumerate(frames):
        # matcher -> consensus: a pair is (the frame's feature, a row of the world table); a merged match's row is the slot's
        # own, n_world + f * cap + feature; the lists leave in the order of the counts the call before wrote, no shuffle
        pairs = M.landmark_pairs(best[f], decision[f], mask[f], ext, n_world, n_world + f * CAP, obs_counts)
        original = M.landmark_pairs(best[f], decision[f], mask[f], None, n_world, n_world + f * CAP, obs_counts)
        pairs_of.append(pairs)
        nmatches[f] = len(original)
        matches[f, :len(original)] = original
        if len(pairs) < 3:
            verdict[f] = SV.FEW_LANDMARKS
            continue
        b, x = bear[frame][pairs[:, 0]], ext[pairs[:, 1]]
        res = L._consensus("p3p", f, b, x, L.p3p_provider(b, x), L.SETTINGS["p3p"], False)
        # consensus -> refinement: a merged match brings BOTH landmarks' observations, the first's first
        lms = [[int(l)] if l < n_world else [int(best[f, j, 0, 0]), int(best[f, j, 1, 0])] for j, l in original]
        others = [[(poses[v].reshape(3, 4), bear[v][i]) for l in ls for v, i in rows[l]] for ls in lms]
        out = SV.refine(bear[frame][original[:, 0]], ext[original[:, 1]].reshape(-1, 4), others, res.pose, res.inliers,
                        SV.settings(**L.SETTINGS["single_view"]), has_model=res.best_id != NONE)
        verdict[f] = out["verdict"]
        if out["final"] is not None:
            final[f, :len(original)] = out["final"]
        if out["pose"] is not None:
            pose_out[f] = out["pose"].reshape(12)
    assert not strict or list(verdict) == [SV.OK] * F, ("registration", list(verdict))
    start, obs = csr(rows)
    split = np.array(state.split, np.uint32).reshape(-1, 2)
    inp = dict(start=start, obs=obs, n_obs=len(obs), n_landmarks=n_world, n_world=n_world, split=split if len(split) else None,
               split_count=[len(split)], split_room=len(split), cap=CAP, n_blocks=N_VIEWS, ik=np.array(frames, np.uint32), n_frames=F,
               counts=w.counts, matches=matches, nmatches=nmatches, final=final, verdict=verdict, pose_out=pose_out, best=best, skip=None)
    added = LT.add_views(inp)
    assert added["call_verdict"] == LT.OK and (not strict or added["frame_verdict"] == [LT.OK] * F), added["frame_verdict"]
    poses = poses.copy()
    for blk, slot in added["poses"].items():
        poses[blk] = pose_out[slot]
    new_rows = [list(r) for r in added["rows"]]
    table_map = np.full((N_VIEWS, CAP), NONE, np.uint32)
    for (b, j), key in added["landmarks"].items():
        table_map[b, j] = key
    call = SimpleNamespace(frames=list(frames), stored=list(stored), rows_before=rows, best=best, decision=decision, share=share, mask=mask,
                           pairs=pairs_of, matches=matches, nmatches=nmatches, final=final, verdict=verdict, stats=added["stats"],
                           counts=added["counts"], rows_after=new_rows, read_map=landmark_map, read_counts=obs_counts)
    common = dict(table_rows=new_rows, table_map=table_map, table_counts=np.array([len(r) for r in new_rows], np.uint32), px=px,
                  tombstones=[l for l in range(n_world) if rows[l] and not new_rows[l]], older=(landmark_map, obs_counts), call=call)
    if not regenerated:                                  # add_views alone: the destination's side of a bridging frame
        return SimpleNamespace(poses=poses, rows=new_rows, split=[], n_world=n_world, matches=matches, nmatches=nmatches, final=final, best=best,
                               **common)
    out = L.regenerate(w, px, poses, new_rows, list(range(*view_range)), view_range, strict)
    for k, v in common.items():
        setattr(out, k, v)
    out.views = sorted({b for r in out.rows for b, _ in r})
    return out


# ------------------------------------------------------------------------------------------------------------ the exact conditions
def conditions(w, call):
    """What an exact world's tables must satisfy, on the arrays of one call (the statement's or the device's): -> dict of
    counts and of lists that must be empty.
      wrong_decision1  a decision-1 feature whose landmark holds no observation of the feature's own point
      wrong_merges     an applied merge (both landmarks named once over the call's final matches) whose two rows and the feature
                       are not one point
      two_live         an applied merge after which both rows are alive
      stray_mask       a mask entry set where the decision is not 2: a mask that belongs to other features
    merged_pairs counts the consensus' pairs whose row is a merge candidate's (>= n_world), i.e. whose merged row holds a point.
    demoted: final merged matches whose pair another final match of the call names too (landmark_table_statement.add_views)."""
    n_world = len(call.rows_before)
    points = lambda l: {int(w.point_of[b][j]) for b, j in call.rows_before[l]}
    live = np.arange(CAP)[None, :] < np.asarray(w.counts)[call.frames][:, None]      # what lies behind a frame's count is nobody's
    mask = (np.asarray(call.mask) != 0) & live
    out = dict(decision1=0, candidates=0, admitted=int(mask.sum()), final_merges=0, applied=0, demoted=0, wrong_decision1=[],
               wrong_merges=[], two_live=[], merged_pairs=sum(int((np.asarray(p).reshape(-1, 2)[:, 1] >= n_world).sum()) for p in call.pairs),
               stray_mask=[(int(f), int(j)) for f, j in np.argwhere(mask & (np.asarray(call.decision) != 2))])
    refs, merges = {}, []
    for f, frame in enumerate(call.frames):
        if call.verdict[f] != 0:
            continue
        for j in range(int(w.counts[frame])):
            l0 = int(call.best[f, j, 0, 0])
            if call.decision[f, j] == 1:
                out["decision1"] += 1
                if l0 >= n_world or int(w.point_of[frame][j]) not in points(l0):
                    out["wrong_decision1"].append((frame, j, l0))
            out["candidates"] += int(call.decision[f, j] == 2)
        for (j, row), ok in zip(call.matches[f, :call.nmatches[f]], call.final[f, :call.nmatches[f]]):
            if not ok:
                continue
            names = [int(row)] if row < n_world else [int(call.best[f, j, 0, 0]), int(call.best[f, j, 1, 0])]
            for l in names:
                refs[l] = refs.get(l, 0) + 1
            if len(names) == 2:
                merges.append((frame, int(j), names))
    out["final_merges"] = len(merges)
    for frame, j, (a, b) in merges:
        if refs[a] != 1 or refs[b] != 1:
            out["demoted"] += 1
            continue
        out["applied"] += 1
        if len(points(a) | points(b) | {int(w.point_of[frame][j])}) != 1:
            out["wrong_merges"].append((frame, j, a, b))
        if call.rows_after[a] and call.rows_after[b]:
            out["two_live"].append((frame, j, a, b))
    return out


# ------------------------------------------------------------------------------------------------------------ the life
# (pixel noise, the share of a VIEW's features that carry another feature's point row).  The designed life's noisy scene makes a
# tenth of every designed LIST wrong; a searched list entry is right only when both of its features carry their own row, and the
# chain of statements — the reference's own thresholds: 64 common inliers for the join, 64 robust matches for a registration —
# refuses such worlds.  With a tenth of every view one world in 96 (seeds 30 - 125) carried both sides through the two grow
# calls (refused by the three-view bootstrap 37, by a registration 44, by the join 14); with 1 - sqrt(0.9) = 0.0513 of a view (a
# tenth of a list) 9 of seeds 9 - 32 did, and none of the four tried registered the bridging frame (50 - 60 robust matches of
# the 64; these scans were made before the bridging frame saw its eight late points).  Of the shares tried below that (0.035, 0.02, 0) this is the largest at which two of seeds 9 - 16 go through to the file.
SCENES = dict(exact=(0.0, 0.0), noisy=(0.5, 0.02))
SEEDS = dict(exact=(1, 2), noisy=(15, 16))               # worlds the chain of statements carries through inside the caps
VIEWS_AFTER = dict(L.VIEWS_AFTER, grow1=4)
PHASES = ("start", "grow1", "grow", "bridge", "merge", "export")
CANDIDATES_AT_LEAST, MERGES_AT_LEAST = 12, 8             # per side of an exact world: the first call's admitted candidates; merges applied
MUST_BE_EMPTY = ("wrong_decision1", "wrong_merges", "two_live", "stray_mask")


def exact_side(first, second, bridge):
    """what conditions() of a side's two grow calls and of the bridging frame's call must show in an EXACT world -> list of what
    does not hold.  The bridging frame sees LATE / 4 points of the side whose merge was demoted: each is a candidate of four
    observations from four views, so its merged row holds a point and the consensus has the pair."""
    if bridge is None:
        return [("the bridging frame was not reached",)]
    failed = [(k, c[k][:3]) for c in (first, second, bridge) for k in MUST_BE_EMPTY if c[k]]
    if first["admitted"] < CANDIDATES_AT_LEAST:
        failed.append(("candidates admitted in the first call", first["admitted"]))
    if first["applied"] + second["applied"] < MERGES_AT_LEAST:
        failed.append(("merges applied", first["applied"] + second["applied"]))
    if first["demoted"] + second["demoted"] < 1:
        failed.append(("merges demoted", 0))
    if bridge["merged_pairs"] < LATE // 4 or bridge["applied"] < LATE // 4:
        failed.append(("merged pairs in the bridging frame's consensus, merges it applied", bridge["merged_pairs"], bridge["applied"]))
    return failed


def life(w, alter=(), handover="documented"):
    """both reconstructions of a world through the phases -> {(side, phase): state}"""
    out = {}
    reg = lambda *a, **k: register(*a, alter=alter, handover=handover, **k)
    for side, triple, frames, view_range in (("A", L.A_START, L.A_GROW, L.A_VIEWS), ("B", L.B_START, L.B_GROW, L.B_VIEWS)):
        out[side, "start"] = start(w, triple, view_range[0], alter)
        # (the graph of a call is the views that exist behind it: four after the first, blocks [lo, lo + 4))
        out[side, "grow1"] = reg(w, out[side, "start"], frames[:1], out[side, "start"].views, (view_range[0], view_range[0] + 4))
        out[side, "grow"] = reg(w, out[side, "grow1"], frames[1:], out[side, "start"].views + list(frames[:1]), view_range)
    out["B", "bridge"], out["A", "bridge"], out["AB", "merge"] = L.merge(w, out["A", "grow"], out["B", "grow"], alter, register_with=reg)
    return out


def errors_of(w, states):
    """reconstruction_life_statement.errors_of; A's side of the bridging frame is add_views alone and has no world table of its own"""
    return L.errors_of(w, {k: v for k, v in states.items() if k != ("A", "bridge")})


def handover_difference(state):
    """the features of the stored views whose landmark differs between the documented and the filtered map"""
    return int((handed_over(state, "documented")[0] != handed_over(state, "filtered")[0]).sum())


# The worst error of this chain of statements (on the CPU, handover "documented") against the ground truth over the scene's two
# seeds and both reconstructions, as measure() printed it, rounded up; a bound is four times the entry, as in the designed life.
BOUNDS = dict(
    exact=dict(
        start=dict(rotation=8.799e-06, centre=7.435e-05, point=4.211e-06),
        grow1=dict(rotation=9.234e-06, centre=4.998e-05, point=3.181e-05),
        grow=dict(rotation=4.028e-05, centre=5.182e-05, point=2.679e-05),
        bridge=dict(rotation=4.113e-05, centre=5.266e-05, point=2.602e-05),
        merge=dict(rotation=1.373e-03, centre=5.077e-03, point=9.570e-03, scale=1.805e-02),
        export=dict(centre=5.077e-03, point=9.570e-03),
    ),
    noisy=dict(
        start=dict(rotation=2.814e-02, centre=9.532e-02, point=3.017e-02),
        grow1=dict(rotation=3.389e-02, centre=7.462e-02, point=2.969e-02),
        grow=dict(rotation=3.396e-02, centre=4.592e-02, point=2.799e-02),
        bridge=dict(rotation=3.262e-02, centre=4.460e-02, point=2.862e-02),
        merge=dict(rotation=2.352e-02, centre=4.027e-02, point=3.539e-02, scale=8.936e-03),
        export=dict(centre=4.027e-02, point=3.539e-02),
    ),
)


def measure(scene, handover="documented"):
    worst = {p: dict(rotation=0.0, centre=0.0, point=0.0, left_out=0.0) for p in PHASES}
    worst["merge"]["scale"] = 0.0
    for seed in SEEDS[scene]:
        w = searched_world(seed, *SCENES[scene])
        states = life(w, handover=handover)
        for (side, phase), e in errors_of(w, states).items():
            assert not e["broken"], (seed, side, phase, e["broken"])
            assert e["views"] == VIEWS_AFTER.get(phase, N_VIEWS), (seed, side, phase, e["views"])
            for k in worst[phase]:
                worst[phase][k] = max(worst[phase][k], e[k])
            if phase == "merge":
                print(scene, seed, "shared points (one row, several rows, rows sharing a view)", e["shared"], "scale", e["scale"])
        for (side, phase), st in states.items():
            if hasattr(st, "call"):
                c = conditions(w, st.call)
                print(scene, seed, side, phase, "differing map entries read", int((st.call.read_map != L.map_of(st.call.rows_before)).sum()),
                      {k: (v if isinstance(v, int) else len(v)) for k, v in c.items()}, flush=True)
    return worst


if __name__ == "__main__":
    import sys
    import time
    handover = sys.argv[1] if len(sys.argv) > 1 else "documented"
    for scene in sys.argv[2:] or SCENES:
        t = time.time()
        print(handover, scene, {p: {k: float("%.3e" % v) for k, v in m.items()} for p, m in measure(scene, handover).items()},
              "%.0f s" % (time.time() - t), flush=True)
