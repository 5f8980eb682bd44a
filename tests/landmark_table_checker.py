"""The CPU checker of the landmark-table kernels for the tests: tests/cpp/landmark_table_host.c (the kernels' loops restated
around include/akz_landmark_table_math.h) as host_build.load compiles it, loaded with ctypes; plus the one description of a
call (`inputs`) that the checker, the device and the statement (tests/landmark_table_statement.py) all take."""
import ctypes as C

import numpy as np

import host_build

OK, NOT_ACCEPTED, BAD_INDEX, BAD_TABLE = range(4)
S_OBSERVATIONS, S_MERGED, S_DEMOTED, S_NEW_LANDMARKS = range(4)
STATS, COUNTS = 4, 4
NONE = 0xFFFFFFFF
FILL8, FILL32 = 0xA5, 0xA5A5A5A5
SV_OK, SV_FEW_ROBUST = 0, 4

_lib = None


def lib():
    global _lib
    if _lib is None:
        L = host_build.load("landmark_table_host.c")
        vp, u32 = C.c_void_p, C.c_uint32
        L.lt_sharing.argtypes = [vp, vp, u32, u32, vp, vp, u32, u32, vp]
        L.lt_sharing.restype = None
        L.lt_add_views.argtypes = [vp, vp, u32, u32, u32, vp, vp, u32, u32, u32, vp, u32] + [vp] * 8 + [u32, u32] + [vp] * 9
        L.lt_merge_applied.argtypes = [u32, u32]
        L.lt_lists_share.argtypes = [vp, u32, u32, u32, u32]
        _lib = L
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data


def table(lists, n_obs=None, pad=0):
    """CSR arrays of per-landmark lists of (block, feature): start [n + 1], obs [n_obs][2]; `pad` rows of filler behind the fill
    (n_obs = fill + pad unless given)."""
    lens = [len(l) for l in lists]
    start = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    flat = [o for l in lists for o in l]
    obs = np.array(flat, np.uint32).reshape(-1, 2)
    n_obs = len(obs) + pad if n_obs is None else n_obs
    full = np.full((max(n_obs, len(obs), 1), 2), FILL32, np.uint32)
    full[:len(obs)] = obs
    return start, full, n_obs


def slot(block, count, matches=(), final=None, verdict=SV_OK, pose=None, skip=0, nmatches=None):
    """One slot of a call: the frame in `block` with `count` features, its original matches [(feature, world row)], their
    final flags (default: all set), the refinement's verdict and pose."""
    matches = [tuple(m) for m in matches]
    return dict(block=block, count=count, matches=matches, final=[1] * len(matches) if final is None else list(final), verdict=verdict,
                pose=pose, skip=skip, nmatches=len(matches) if nmatches is None else nmatches)


def inputs(start, obs, n_obs, cap, n_blocks, slots=(), n_world=None, split=None, split_count=None, split_room=None, best=None, use_skip=None,
           counts=None, obs_room=None, lm_room=None, extra_room=0):
    """Every array of an rs_add_views_device call, contiguous, as a dict.  best: {(slot, feature): (a, b)} -> d_best with those
    two landmarks (distance 0) and none elsewhere, or None for no d_best."""
    start = np.ascontiguousarray(start, np.uint32)
    obs = np.ascontiguousarray(obs, np.uint32).reshape(-1, 2)
    n_lm, F = len(start) - 1, len(slots)
    n_world = n_lm if n_world is None else n_world
    cnt = np.zeros(n_blocks, np.uint32) if counts is None else np.ascontiguousarray(counts, np.uint32).copy()
    matches = np.full((max(F, 1), cap, 2), FILL32, np.uint32)
    final = np.full((max(F, 1), cap), FILL8, np.uint8)
    nmatches, verdict, skip = np.zeros(max(F, 1), np.uint32), np.zeros(max(F, 1), np.uint32), np.zeros(max(F, 1), np.uint32)
    pose_out = np.zeros((max(F, 1), 12))
    for f, s in enumerate(slots):
        if counts is None:
            cnt[s["block"]] = s["count"]
        m = np.array(s["matches"], np.uint32).reshape(-1, 2)[:cap]
        matches[f, :len(m)] = m
        final[f, :len(m)] = np.array(s["final"], np.uint8)[:cap]
        nmatches[f], verdict[f], skip[f] = s["nmatches"], s["verdict"], s["skip"]
        pose_out[f] = np.arange(12) / 16.0 + f + 1 if s["pose"] is None else np.asarray(s["pose"], np.float64).reshape(12)
    d_best = None
    if best is not None:
        d_best = np.full((max(F, 1), cap, 3, 2), NONE, np.uint32)
        for (f, j), (a, b) in best.items():
            d_best[f, j, 0], d_best[f, j, 1] = (a, 0), (b, 0)
    if use_skip is None:
        use_skip = bool(skip.any())
    if split is not None:
        split = np.ascontiguousarray(split, np.uint32).reshape(-1, 2)
        split_room = len(split) if split_room is None else split_room
        split_count = np.array([len(split) if split_count is None else split_count], np.uint32)
        if len(split) < max(split_room, 1):
            split = np.concatenate([split, np.full((max(split_room, 1) - len(split), 2), FILL32, np.uint32)])
    else:
        split_room, split_count = 0, None
    grow = split_room + F * cap
    return dict(start=start, obs=obs, n_obs=n_obs, n_landmarks=n_lm, n_world=n_world, split=split, split_count=split_count, split_room=split_room,
                cap=cap, n_blocks=n_blocks, ik=np.array([s["block"] for s in slots], np.uint32), n_frames=F, counts=cnt, matches=matches,
                nmatches=nmatches, final=final, verdict=verdict, pose_out=pose_out, best=d_best, skip=skip if use_skip else None,
                obs_room=n_obs + grow + extra_room if obs_room is None else obs_room,
                lm_room=n_lm + grow + extra_room if lm_room is None else lm_room, poses=np.full((n_blocks, 12), -1.0))


def outputs(inp):
    """The output buffers of a call under their fill — what neither side writes stays FILL32."""
    F = max(inp["n_frames"], 1)
    return dict(poses=inp["poses"].copy(), start_out=np.full(inp["lm_room"] + 1, FILL32, np.uint32),
                obs_out=np.full((max(inp["obs_room"], 1), 2), FILL32, np.uint32), counts_out=np.full(COUNTS, FILL32, np.uint32),
                landmarks_out=np.full((inp["n_blocks"], inp["cap"]), FILL32, np.uint32),
                obs_counts_out=np.full(max(inp["lm_room"], 1), FILL32, np.uint32), frame_verdict=np.full(F, FILL32, np.uint32),
                stats=np.full((F, STATS), FILL32, np.uint32), call_verdict=np.full(1, FILL32, np.uint32))


OUTPUT_NAMES = ("poses", "start_out", "obs_out", "counts_out", "landmarks_out", "obs_counts_out", "frame_verdict", "stats", "call_verdict")


def add_views(inp):
    """rs_add_views_device on the host -> dict of every output buffer."""
    o = outputs(inp)
    r = lib().lt_add_views(_p(inp["start"]), _p(inp["obs"]), inp["n_obs"], inp["n_landmarks"], inp["n_world"], _p(inp["split"]),
                           _p(inp["split_count"]), inp["split_room"], inp["cap"], inp["n_blocks"], _p(inp["ik"]), inp["n_frames"],
                           _p(inp["counts"]), _p(inp["matches"]), _p(inp["nmatches"]), _p(inp["final"]), _p(inp["verdict"]),
                           _p(inp["pose_out"]), _p(inp["best"]), _p(inp["skip"]), inp["obs_room"], inp["lm_room"], *[_p(o[k]) for k in OUTPUT_NAMES])
    assert r == 0
    return o


def sharing_view(start, obs, n_obs, best, decision):
    """rs_landmarks_sharing_view_device on the host: best [F][cap][3][2], decision [F][cap] -> mask [F][cap] u8."""
    start, obs = np.ascontiguousarray(start, np.uint32), np.ascontiguousarray(obs, np.uint32)
    best, decision = np.ascontiguousarray(best, np.uint32), np.ascontiguousarray(decision, np.uint32)
    F, cap = decision.shape
    mask = np.full((F, cap), FILL8, np.uint8)
    lib().lt_sharing(_p(start), _p(obs), n_obs, len(start) - 1, _p(best), _p(decision), cap, F, _p(mask))
    return mask


def rows(o, n_rows=None):
    """The filled rows of an output table as lists of (block, feature)."""
    n = int(o["counts_out"][0]) if n_rows is None else n_rows
    s = o["start_out"]
    return [[tuple(int(v) for v in ob) for ob in o["obs_out"][s[r]:s[r + 1]]] for r in range(n)]


def random_call(seed, n_landmarks=40, n_views=6, n_frames=3, cap=48, merges=2, collide=True, bad_slots=False, split=0, pad=3, extra_room=0):
    """A table of n_landmarks lists over the blocks [0, n_views) (0 to 5 observations each, a block at most once per list) and
    n_frames new frames in the blocks behind them, handed over in descending block order so that slot order is not block order.
    Every frame matches some of its features to landmarks — distinct inside the frame; with `collide` two frames may name one
    landmark — and up to `merges` of them to a pair of landmarks that share no view.  -> inputs(...)"""
    rng = np.random.default_rng(seed)
    used = np.zeros(n_views, np.int64)
    lists = []
    for _ in range(n_landmarks):
        views = rng.permutation(n_views)[:rng.integers(0, min(n_views, 5) + 1)]
        row = []
        for v in views:
            row.append((int(v), int(used[v])))
            used[v] += 1
        lists.append(row)
    sp = None
    if split:                                                    # observations a filter took out of their landmarks: features of their own
        sp = []
        for k in range(split):
            sp.append((k % n_views, int(used[k % n_views])))
            used[k % n_views] += 1
    assert used.max(initial=0) <= cap
    start, obs, n_obs = table(lists, pad=pad)
    n_blocks = n_views + n_frames
    counts = np.zeros(n_blocks, np.uint32)
    counts[:n_views] = used
    slots, best = [], {}
    free = list(rng.permutation(n_landmarks))                    # without `collide` no landmark is named twice in the call
    for f in range(n_frames):
        block = n_blocks - 1 - f
        count = int(rng.integers(0, cap + 1))
        counts[block] = count
        feats = rng.permutation(count)[:rng.integers(0, count + 1)] if count else []
        pool = list(rng.permutation(n_landmarks)) if collide else free
        matches, final, left = [], [], merges
        for j in feats:
            if len(pool) < 2:
                break
            a = int(pool.pop())
            if left and rng.random() < 0.3:
                b = next((int(x) for x in pool if not {v for v, _ in lists[a]} & {v for v, _ in lists[int(x)]}), None)
                if b is not None:
                    pool.remove(b)
                    left -= 1
                    best[(f, int(j))] = (a, b)
                    matches.append((int(j), n_landmarks + f * cap + int(j)))
                    final.append(1)
                    continue
            matches.append((int(j), a))
            final.append(int(rng.random() < 0.85))
        order = rng.permutation(len(matches))
        s = slot(block, count, [matches[k] for k in order], [final[k] for k in order],
                 verdict=SV_OK if rng.random() < 0.85 else SV_FEW_ROBUST, skip=int(rng.random() < 0.1))
        if bad_slots and f % 3 == 1 and s["matches"]:
            s["matches"][0] = (s["matches"][0][0], n_landmarks + 7 * cap * n_frames)       # names nothing
            s["final"][0] = 1
        slots.append(s)
    return inputs(start, obs, n_obs, cap, n_blocks, slots, best=best, counts=counts, split=sp, extra_room=extra_room)


def check_against_statement(inp, o, expect=None, fill=FILL32):
    """Every output buffer `o` of a call against tests/landmark_table_statement.py's result for the same inputs (`expect`: that
    result when the caller has it already; `fill`: what the observation rows held before the call) -> the result."""
    import landmark_table_statement as S
    st = S.add_views(inp) if expect is None else expect
    F = inp["n_frames"]
    assert int(o["call_verdict"][0]) == st["call_verdict"]
    assert [int(v) for v in o["frame_verdict"][:F]] == st["frame_verdict"]
    assert [[int(v) for v in row] for row in o["stats"][:F]] == st["stats"]
    assert [int(v) for v in o["counts_out"]] == st["counts"]
    n_rows, total = st["counts"][0], st["counts"][1]
    assert rows(o) == st["rows"]                                                   # as lists: the order inside a row is specified
    lens = [len(r) for r in st["rows"]]
    assert [int(v) for v in o["obs_counts_out"][:inp["lm_room"]]] == lens + [0] * (inp["lm_room"] - n_rows)
    assert np.all(o["start_out"][n_rows:] == total) and (n_rows == 0 or o["start_out"][0] == 0)
    assert np.all(o["obs_out"][total:] == fill)                                    # nothing is written behind the total
    want = np.full((inp["n_blocks"], inp["cap"]), NONE, np.uint32)
    for (blk, feat), key in st["landmarks"].items():
        if blk < inp["n_blocks"] and feat < inp["cap"]:
            want[blk, feat] = key
    assert np.array_equal(o["landmarks_out"], want)                                # the exact inverse of the table
    poses = inp["poses"].copy()
    for blk, f in st["poses"].items():
        poses[blk] = inp["pose_out"][f]
    assert np.array_equal(o["poses"], poses)
    return st


def one_observation_per_view(table_rows):
    """the invariant of a landmark: no view observes it twice"""
    return all(len({v for v, _ in r}) == len(r) for r in table_rows)


# ---- designed calls: every rule and every refusal once, small enough to read ----------------------------------------
def small_table():
    """landmarks 0..5 over the views 0..3; 4 is empty, 5 has one observation"""
    return [[(0, 0), (1, 0)], [(2, 0), (3, 0)], [(0, 1), (2, 1), (3, 1)], [(1, 1)], [], [(3, 2)]]


def designed(slots, best=None, lists=None, cap=8, n_blocks=8, **kw):
    start, obs, n_obs = table(small_table() if lists is None else lists, pad=2)
    return inputs(start, obs, n_obs, cap, n_blocks, slots, best=best, **kw)


def designed_cases():
    """name -> inputs.  Merged rows are n_world + slot * cap + feature with n_world = 6, cap = 8."""
    good = lambda block, lm: slot(block, 3, [(1, lm)])
    around = lambda s, **kw: designed([good(4, 0), s, good(6, 2)], **kw)
    start, obs, n_obs = table(small_table(), pad=1)
    empty = table([], pad=0)
    c = {
        "one frame: matches, a merge, new landmarks": designed([slot(5, 6, [(4, 3), (1, 6 + 1), (0, 2)])], best={(0, 1): (0, 1)}, n_blocks=6),
        "three frames on one landmark, ik not ascending": designed([slot(7, 2, [(1, 2)]), slot(5, 3, [(0, 2), (2, 0)]), slot(6, 1, [(0, 2)])]),
        "a merge demoted because another frame names b": designed([slot(4, 2, [(0, 6)]), slot(5, 2, [(1, 1)])], best={(0, 0): (0, 1)}),
        "a merge demoted because another frame names a": designed([slot(4, 2, [(0, 6)]), slot(5, 2, [(1, 0)])], best={(0, 0): (0, 1)}),
        "two merges chained through one landmark": designed([slot(4, 2, [(0, 6)]), slot(5, 2, [(1, 6 + 8 + 1)])],
                                                            best={(0, 0): (5, 3), (1, 1): (3, 4)}),
        "two merges that touch nothing in common": designed([slot(4, 2, [(0, 6)]), slot(5, 2, [(1, 6 + 8 + 1)])],
                                                            best={(0, 0): (5, 3), (1, 1): (1, 0)}),
        "bad: a landmark >= n_landmarks": around(slot(5, 2, [(0, 6)])),
        "bad: a feature >= count": around(slot(5, 2, [(2, 1)])),
        "bad: the merged row of another slot": around(slot(5, 2, [(0, 6 + 0)]), best={(1, 0): (0, 1), (0, 0): (0, 1)}),
        "bad: a merged row without d_best": around(slot(5, 2, [(0, 6 + 8 + 0)])),
        "bad: a merge of a landmark with itself": around(slot(5, 2, [(0, 6 + 8 + 0)]), best={(1, 0): (1, 1)}),
        "bad: a merge with an absent landmark": around(slot(5, 2, [(0, 6 + 8 + 0)]), best={(1, 0): (1, NONE)}),
        "bad: a feature in two final matches": around(slot(5, 2, [(0, 1), (0, 3)])),
        "bad: a count above the capacity": around(slot(5, 9, [(0, 1)])),
        "bad: a match count above the capacity": around(slot(5, 2, [(0, 1)], nmatches=9)),
        "a row below n_world but not below n_landmarks": around(slot(5, 2, [(0, 7)]), n_world=9),
        "a verdict that is not RS_SV_OK": around(slot(5, 2, [(0, 99)], verdict=SV_FEW_ROBUST)),
        "a skipped slot": around(slot(5, 2, [(0, 1)], skip=1)),
        "a skip array of zeros": around(slot(5, 2, [(0, 1)]), use_skip=True),
        "a match that is not final": designed([slot(4, 2, [(0, 99), (1, 2)], final=[0, 1])]),
        "no frames, a split list above its room": inputs(start, obs, n_obs, 8, 4, [], split=[(0, 5), (1, 5), (2, 5)], split_count=7, split_room=3),
        "no frames, a split list below its room": inputs(start, obs, n_obs, 8, 4, [], split=[(0, 5), (1, 5), (2, 5)], split_count=1, split_room=3),
        "frames and a split list": designed([slot(5, 3, [(1, 2)])], split=[(0, 5), (1, 5)]),
        "an empty table, nothing to add": inputs(*empty, 4, 2, []),
        "an empty table, a frame of cap features and one of none": inputs(*empty, 4, 2, [slot(1, 4), slot(0, 0)]),
        "starts that descend": inputs(np.array([0, 2, 1, 7, 8, 8, 9], np.uint32), obs, n_obs, 8, 8, [slot(4, 2, [(0, 1)])], split=[(0, 5)]),
        "a last start above n_obs": inputs(np.array([0, 2, 4, 7, 8, 8, 12], np.uint32), obs, n_obs, 8, 8, [slot(4, 2, [(0, 1)])], split=[(0, 5)]),
        "a first start above 0": inputs(np.array([1, 2, 4, 7, 8, 8, 9], np.uint32), obs, n_obs, 8, 8, []),
        "a feature listed twice": designed([], lists=[[(0, 0)], [(1, 1), (0, 0)], [(0, 0), (2, 0)]], n_blocks=3),
        "an observation outside the blocks": designed([], lists=[[(9, 0), (0, 99), (1, 1)]], n_blocks=3),
        "rooms above the least": designed([slot(5, 3, [(1, 2)])], extra_room=5),
    }
    return c


def mask_case(lists, pairs, decisions, cap=None, n_obs=None, pad=2, frames=1):
    """one merge candidate per feature of slot 0: pairs [(a, b)], decisions -> start, obs, n_obs, best [F][cap][3][2], decision"""
    start, obs, n_obs = table(lists, n_obs=n_obs, pad=pad)
    cap = cap or len(pairs)
    best = np.full((frames, cap, 3, 2), NONE, np.uint32)
    decision = np.zeros((frames, cap), np.uint32)
    for j, ((a, b), d) in enumerate(zip(pairs, decisions)):
        f, k = divmod(j, cap)
        best[f, k, 0, 0], best[f, k, 1, 0], decision[f, k] = a, b, d
        best[f, k, :, 1] = 7
    return start, obs, n_obs, best, decision


def mask_lists():
    """lists of 1, 2, 65, 66 and 70 entries; 6 and 7 share nothing with 5 but for 7's last element"""
    long_a = [(v, 0) for v in range(70)]
    long_b = [(100 + v, 0) for v in range(66)]
    return [[(0, 0), (1, 0)], [(2, 0), (3, 0)], [(4, 0), (1, 1)], [], [(5, 0)], long_a, long_b, long_b[:65] + [(69, 1)], [(69, 2)]]


MASK_PAIRS = [(0, 1), (0, 1), (0, 1), (0, 2), (0, NONE), (NONE, 1), (0, 9), (3, 0), (4, 4), (5, 6), (5, 7), (6, 7), (5, 8), (8, 5), (4, 6), (0, 3)]
MASK_DECISIONS = [2, 1, 0, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3]
#               d=2 d=1 d=0 share absent absent >=n empty same long long-share-last share(first) share share long+short d=3
MASK_WANT = [1, 0, 0, 0, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 1, 0]
