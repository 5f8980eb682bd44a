"""An independent statement of the landmark bookkeeping in dicts, sets and lists — no arrays, no scan, no code shared with
include/akz_landmark_table_math.h.

`Reconstruction` is the reference's text, applied frame by frame: a landmark is {view: feature} (a dict keeps the order of
insertion, which is the order the device's lists are specified in), a view is the list of the landmark each feature observes.

  VSlamData::add_view                 cv-sfm/src/lib.rs:432-483
  VSlamData::add_landmark             cv-sfm/src/lib.rs:487-500
  VSlamData::merge_landmarks          cv-sfm/src/lib.rs:699-721
  VSlam::are_landmarks_sharing_view   cv-sfm/src/lib.rs:1435-1449

`add_views` layers the rule for several frames against one table on top (a merge is applied only when nothing else in the call
names either landmark; otherwise the observation goes to the first landmark alone), and keeps keys stable: a merged-away
landmark stays as an empty row.  Both take the call as landmark_table_checker.inputs describes it.
"""

NONE = 0xFFFFFFFF
OK, NOT_ACCEPTED, BAD_INDEX, BAD_TABLE = range(4)


class Reconstruction:
    def __init__(self, lists):
        """lists: per landmark key, the (view, feature) observations in order"""
        self.landmarks = {}
        self.views = {}
        self.next_key = 0
        for l in lists:
            key = self._insert({})
            for view, feature in l:
                self.landmarks[key][view] = feature
                self.views.setdefault(view, {})[feature] = key

    def _insert(self, observations):
        key = self.next_key
        self.next_key += 1
        self.landmarks[key] = observations
        return key

    def add_landmark(self, view, feature):
        return self._insert({view: feature})

    def merge_landmarks(self, a, b):
        old = self.landmarks.pop(b)                       # "landmark_b didnt exist" otherwise
        for view, feature in old.items():
            self.views[view][feature] = a
            assert view not in self.landmarks[a]
            self.landmarks[a][view] = feature
        return a

    def add_view(self, view, n_features, existing_landmark):
        assert view not in self.views
        self.views[view] = {}
        merged = 0
        for feature in range(n_features):
            found = existing_landmark(feature)
            if found is not None:
                if len(found) == 1:
                    landmark = found[0]
                else:
                    a, b = found
                    merged += 1
                    landmark = self.merge_landmarks(a, b)
                self.landmarks[landmark][view] = feature
            else:
                landmark = self.add_landmark(view, feature)
            self.views[view][feature] = landmark
        return merged

    def are_landmarks_sharing_view(self, a, b):
        first = [view for view in self.landmarks[a]]
        return any(view in first for view in self.landmarks[b])

    def rows(self, n_rows):
        """row per key below n_rows: the observations in order; a removed landmark is an empty row"""
        return [[(v, f) for v, f in self.landmarks.get(k, {}).items()] for k in range(n_rows)]


def input_lists(inp):
    """the per-landmark lists of the input table, or None when its starts do not ascend inside [0, n_obs]"""
    start = [int(s) for s in inp["start"]]
    if any(a > b for a, b in zip(start, start[1:])) or start[-1] > inp["n_obs"]:
        return None
    return [[(int(b), int(f)) for b, f in inp["obs"][start[l]:start[l + 1]]] for l in range(inp["n_landmarks"])]


def split_list(inp):
    if inp["split"] is None:
        return []
    n = min(int(inp["split_count"][0]), inp["split_room"])
    return [(int(b), int(f)) for b, f in inp["split"][:n]]


def final_matches(inp, f):
    """slot f's final matches as (feature, [landmarks]) in list order, or None when the slot is invalid"""
    cap, n_lm, n_world = inp["cap"], inp["n_landmarks"], inp["n_world"]
    count, nm = int(inp["counts"][inp["ik"][f]]), int(inp["nmatches"][f])
    if count > cap or nm > cap:
        return None
    out, seen = [], set()
    for i in range(nm):
        if not inp["final"][f, i]:
            continue
        feature, row = int(inp["matches"][f, i, 0]), int(inp["matches"][f, i, 1])
        if feature >= count or feature in seen:
            return None
        seen.add(feature)
        if row < min(n_world, n_lm):
            out.append((feature, [row]))
        elif row == n_world + f * cap + feature and inp["best"] is not None:
            a, b = int(inp["best"][f, feature, 0, 0]), int(inp["best"][f, feature, 1, 0])
            if a == b or a >= n_lm or b >= n_lm:
                return None
            out.append((feature, [a, b]))
        else:
            return None
    return out


def verdicts(inp):
    """per slot: (verdict, final matches or None)"""
    out = []
    lists = input_lists(inp)
    for f in range(inp["n_frames"]):
        skipped = inp["skip"] is not None and inp["skip"][f] != 0
        if lists is None or inp["verdict"][f] != 0 or skipped:
            out.append((NOT_ACCEPTED, None))
            continue
        fm = final_matches(inp, f)
        out.append((OK, fm) if fm is not None else (BAD_INDEX, None))
    return out


def sequential(inp):
    """The reference, frame by frame: the split rows, then add_view for each accepted slot in order.  For one frame this is the
    expectation with no rule of ours involved.  -> (rows, Reconstruction)"""
    lists = input_lists(inp)
    rec = Reconstruction(lists)
    for view, feature in split_list(inp):
        rec.add_landmark(view, feature)
    for f, (verdict, fm) in enumerate(verdicts(inp)):
        if verdict != OK:
            continue
        named = dict(fm)
        rec.add_view(int(inp["ik"][f]), int(inp["counts"][inp["ik"][f]]), lambda feature: named.get(feature))
    return rec.rows(rec.next_key), rec


def add_views(inp):
    """The batch: every accepted slot against the one input table.  -> dict(rows, landmarks {(block, feature): key},
    frame_verdict, stats [observations, merged, demoted, new], counts [rows, observations, merged, demoted], call_verdict,
    poses {block: slot})"""
    lists = input_lists(inp)
    vs = verdicts(inp)
    if lists is None:
        return dict(rows=[], landmarks={}, frame_verdict=[v for v, _ in vs], stats=[[0, 0, 0, 0] for _ in vs], counts=[0, 0, 0, 0],
                    call_verdict=BAD_TABLE, poses={})
    refs = {}
    for verdict, fm in vs:
        if verdict == OK:
            for _, names in fm:
                for l in names:
                    refs[l] = refs.get(l, 0) + 1
    rows = [list(l) for l in lists]
    gone = set()
    new = {}                                               # landmark -> [(slot, block, feature)]
    stats = [[0, 0, 0, 0] for _ in vs]
    for f, (verdict, fm) in enumerate(vs):
        if verdict != OK:
            continue
        for feature, names in fm:
            if len(names) == 2:
                a, b = names
                if refs[a] == 1 and refs[b] == 1:
                    rows[a] = rows[a] + rows[b]
                    rows[b] = []
                    gone.add(b)
                    stats[f][1] += 1
                else:
                    stats[f][2] += 1
            new.setdefault(names[0], []).append((f, int(inp["ik"][f]), feature))
            stats[f][0] += 1
    for l, added in new.items():
        assert l not in gone
        rows[l] = rows[l] + [(blk, feature) for _, blk, feature in sorted(added)]
    rows += [[o] for o in split_list(inp)]
    poses = {}
    for f, (verdict, fm) in enumerate(vs):
        if verdict != OK:
            continue
        named = {feature for feature, _ in fm}
        blk = int(inp["ik"][f])
        poses[blk] = f
        for j in range(int(inp["counts"][blk])):
            if j not in named:
                rows.append([(blk, j)])
                stats[f][3] += 1
    landmarks = {}
    for key, row in enumerate(rows):
        for o in row:
            landmarks.setdefault(o, key)                   # the lowest key where a broken table lists a feature twice
    return dict(rows=rows, landmarks=landmarks, frame_verdict=[v for v, _ in vs], stats=stats,
                counts=[len(rows), sum(len(r) for r in rows), sum(s[1] for s in stats), sum(s[2] for s in stats)], call_verdict=OK, poses=poses)


def sharing_mask(lists, best, decision, n_landmarks):
    """the mask of the merge candidates: lists per landmark (None where its range does not lie inside the table)"""
    rec = Reconstruction([l or [] for l in lists])
    F, cap = len(decision), len(decision[0])
    mask = [[0] * cap for _ in range(F)]
    for f in range(F):
        for j in range(cap):
            a, b = int(best[f][j][0][0]), int(best[f][j][1][0])
            if decision[f][j] != 2 or a >= n_landmarks or b >= n_landmarks or lists[a] is None or lists[b] is None:
                continue
            mask[f][j] = 0 if rec.are_landmarks_sharing_view(a, b) else 1
    return mask
