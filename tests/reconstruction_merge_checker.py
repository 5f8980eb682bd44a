"""The CPU checker of the reconstruction-merge kernels for the tests: tests/cpp/reconstruction_merge_host.c (the host's
execution of include/akz_reconstruction_merge_math.h) as host_build.load compiles it, loaded with ctypes; plus the one
description of a call (`incorporate_inputs`, `map_inputs`, `normalize_inputs`) that the checker, the device and the statement
(tests/reconstruction_merge_statement.py) all take, the designed cases and the seeded random ones."""
import ctypes as C

import numpy as np

import host_build
from landmark_table_checker import FILL8, FILL32, NONE, table

OK, BAD_TABLE, BAD_INDEX, SHARED_BLOCK = range(4)
NR_OK, NR_NOT_NORMAL, NR_BAD_INDEX = range(3)
COUNTS = 6
FILL64 = np.frombuffer(np.full(2, FILL32, np.uint32).tobytes(), np.float64)[0]

_lib = None


def lib():
    global _lib
    if _lib is None:
        L = host_build.load("reconstruction_merge_host.c")
        vp, u32 = C.c_void_p, C.c_uint32
        L.mr_merge_map.argtypes = [vp, vp, vp, vp, u32, u32, u32, u32, vp, vp, u32, u32, vp, vp]
        L.mr_incorporate.argtypes = [vp, vp, u32, u32, vp, vp, u32, u32, vp, vp, u32, u32, u32, vp, u32, u32, vp, vp, u32, u32] + [vp] * 8
        L.mr_normalize.argtypes = [vp, u32, vp, vp, u32, u32, vp, u32, vp, vp, u32, vp, vp]
        L.mr_normalize.restype = None
        L.mr_is_normal.argtypes = [C.c_double]
        L.mr_transform.argtypes = [vp, vp, vp]
        L.mr_transform.restype = None
        _lib = L
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data


def random_pose(rng, t_max=10.0):
    """a rotation from a random axis-angle, |t| <= t_max -> [12] row-major 3 x 4"""
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    angle = rng.uniform(-np.pi, np.pi)
    k = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    r = np.eye(3) + np.sin(angle) * k + (1 - np.cos(angle)) * (k @ k)
    t = rng.normal(size=3)
    t *= rng.uniform(0, t_max) / np.linalg.norm(t)
    return np.concatenate([r, t[:, None]], axis=1).reshape(12)


# ---- incorporate ----------------------------------------------------------------------------------------------------
def incorporate_inputs(dst_rows, src_rows, pairs, src_blocks, bridge_block, cap=8, n_blocks=12, skip=None, map_room=None, map_count=None,
                       extra_room=0, pad=2, seed=0, dst_start=None, src_start=None):
    """Every array of an rs_incorporate_reconstruction_device call, contiguous, as a dict.  dst_rows / src_rows: per-landmark
    lists of (block, feature); pairs [(source landmark, destination landmark)]; *_start: starts to hand over instead of the
    rows' own (the broken tables)."""
    rng = np.random.default_rng(seed)
    ds, dobs, n_dst_obs = table(dst_rows, pad=pad)
    ss, sobs, n_src_obs = table(src_rows, pad=pad)
    ds = ds if dst_start is None else np.array(dst_start, np.uint32)
    ss = ss if src_start is None else np.array(src_start, np.uint32)
    n_dst, n_src = len(ds) - 1, len(ss) - 1
    map_room = max(len(pairs), 1) if map_room is None else map_room
    m = np.full((max(map_room, len(pairs), 1), 2), FILL32, np.uint32)
    if len(pairs):
        m[:len(pairs)] = np.array(pairs, np.uint32).reshape(-1, 2)
    poses = np.stack([random_pose(rng) for _ in range(n_blocks)])
    return dict(dst_start=ds, dst_obs=dobs, n_dst_obs=n_dst_obs, n_dst=n_dst, src_start=ss, src_obs=sobs, n_src_obs=n_src_obs, n_src=n_src,
                map=m, map_count=np.array([len(pairs) if map_count is None else map_count], np.uint32), map_room=map_room, cap=cap,
                n_blocks=n_blocks, src_blocks=np.array(src_blocks, np.uint32), bridge_block=bridge_block, src_pose=random_pose(rng),
                skip=None if skip is None else np.array(skip, np.uint32), obs_room=n_dst_obs + n_src_obs + extra_room,
                lm_room=n_dst + n_src + extra_room, poses=poses, dst_rows=dst_rows, src_rows=src_rows, pairs=list(pairs))


IR_OUTPUTS = ("poses", "start_out", "obs_out", "counts_out", "landmarks_out", "obs_counts_out", "src_key_out", "call_verdict")


def incorporate_outputs(inp):
    """The output buffers of a call under their fill — what neither side writes stays FILL32."""
    w = lambda *shape: np.full(shape, FILL32, np.uint32)
    return dict(poses=inp["poses"].copy(), start_out=w(inp["lm_room"] + 1), obs_out=w(max(inp["obs_room"], 1), 2), counts_out=w(COUNTS),
                landmarks_out=w(inp["n_blocks"], inp["cap"]), obs_counts_out=w(max(inp["lm_room"], 1)), src_key_out=w(max(inp["n_src"], 1)),
                call_verdict=w(1))


def incorporate(inp):
    """rs_incorporate_reconstruction_device on the host -> dict of every output buffer."""
    o = incorporate_outputs(inp)
    r = lib().mr_incorporate(_p(inp["dst_start"]), _p(inp["dst_obs"]), inp["n_dst_obs"], inp["n_dst"], _p(inp["src_start"]), _p(inp["src_obs"]),
                             inp["n_src_obs"], inp["n_src"], _p(inp["map"]), _p(inp["map_count"]), inp["map_room"], inp["cap"], inp["n_blocks"],
                             _p(inp["src_blocks"]), len(inp["src_blocks"]), inp["bridge_block"], _p(inp["src_pose"]), _p(inp["skip"]),
                             inp["obs_room"], inp["lm_room"], *[_p(o[k]) for k in IR_OUTPUTS])
    assert r == 0
    return o


def out_rows(o, n_rows=None):
    """The filled rows of an output table as lists of (block, feature)."""
    n = int(o["counts_out"][0]) if n_rows is None else n_rows
    s = o["start_out"]
    return [[tuple(int(v) for v in ob) for ob in o["obs_out"][s[r]:s[r + 1]]] for r in range(n)]


def check_incorporate_against_statement(inp, o, bound):
    """Every output buffer `o` of a call against the statement's result for the same inputs -> (the result, the largest
    absolute pose difference).  Integers exactly, rows as lists in the documented order; poses under `bound`."""
    import reconstruction_merge_statement as S
    n_map = min(int(inp["map_count"][0]), inp["map_room"])
    st = S.incorporate(inp["dst_rows"], inp["src_rows"], inp["pairs"][:n_map], [int(b) for b in inp["src_blocks"]], inp["bridge_block"],
                       inp["src_pose"], inp["poses"], inp["cap"], inp["n_blocks"], None if inp["skip"] is None else [int(s) for s in inp["skip"]])
    assert int(o["call_verdict"][0]) == st["verdict"]
    assert [int(v) for v in o["counts_out"]] == st["counts"]
    n_rows, total = st["counts"][0], st["counts"][1]
    assert out_rows(o) == st["rows"]
    lens = [len(r) for r in st["rows"]]
    assert [int(v) for v in o["obs_counts_out"][:inp["lm_room"]]] == lens + [0] * (inp["lm_room"] - n_rows)
    assert np.all(o["start_out"][n_rows:] == total) and (n_rows == 0 or o["start_out"][0] == 0)
    assert np.all(o["obs_out"][total:] == FILL32)                                  # nothing is written behind the total
    want = np.full((inp["n_blocks"], inp["cap"]), NONE, np.uint32)
    for (blk, feat), key in st["landmarks"].items():
        if blk < inp["n_blocks"] and feat < inp["cap"]:
            want[blk, feat] = key
    assert np.array_equal(o["landmarks_out"], want)
    assert [int(v) for v in o["src_key_out"][:inp["n_src"]]] == st["src_key"]
    diff = float(np.max(np.abs(o["poses"] - st["poses"])))
    assert diff <= bound, diff
    touched = {int(b) for b, s in zip(inp["src_blocks"], inp["skip"] if inp["skip"] is not None else [0] * len(inp["src_blocks"])) if not s}
    for b in range(inp["n_blocks"]):
        if b not in touched or st["verdict"] != OK:
            assert np.array_equal(o["poses"][b], inp["poses"][b]), b               # every other pose keeps its bytes
    return st, diff


def dst_small():
    """destination landmarks 0..5 over the views 0..3 and the bridging frame's block 4; 4 is a tombstone"""
    return [[(0, 0), (1, 0), (4, 0)], [(2, 0), (3, 0)], [(0, 1), (2, 1), (3, 1), (4, 1)], [(1, 1)], [], [(3, 2), (4, 2)]]


def src_small():
    """source landmarks 0..6 over the views 6..8 and the bridging frame's block 4 (as the source saw it); 3 is a tombstone, 5 is
    seen by the bridging frame alone"""
    return [[(6, 0), (7, 0), (4, 3)], [(6, 1), (8, 0)], [(7, 1), (8, 1), (4, 4)], [], [(6, 2)], [(4, 5)], [(8, 2), (7, 2), (6, 3)]]


def designed_incorporate_cases():
    """name -> inputs.  Blocks 0..3 the destination's views, 4 the bridging frame, 6..8 the source's."""
    views, bridge = (6, 7, 8), 4
    case = lambda pairs, dst=None, src=None, **kw: incorporate_inputs(dst_small() if dst is None else dst, src_small() if src is None else src, pairs,
                                                                     kw.pop("src_blocks", views), bridge, **kw)
    only_bridge = [[(4, 3)], [], [(4, 4)]]
    return {
        "an empty map": case([]),
        "a map of one": case([(0, 2)]),
        "every source landmark mapped": case([(0, 0), (1, 1), (2, 2), (3, 3), (4, 4), (5, 5)], src=src_small()[:6]),
        "two entries with one destination": case([(0, 2), (1, 2), (4, 0)]),
        "two entries with one source": case([(0, 2), (0, 3), (4, 0)]),
        "an entry that names a landmark outside the source": case([(7, 1), (0, 2)]),
        "an entry that names a landmark outside the destination": case([(1, 6), (0, 2)]),
        "an outside entry still names its other landmark": case([(0, 99), (0, 2)]),
        "a source whose every observation is the bridging frame's": case([(0, 1)], src=only_bridge),
        "source tombstones": case([(3, 0)], src=[[], [(6, 0)], [], [(7, 0), (8, 0)], []]),
        "a skipped view": case([(0, 2), (4, 1)], skip=[0, 1, 0]),
        "a skip array of zeros": case([(0, 2)], skip=[0, 0, 0]),
        "every view skipped": case([(0, 2)], skip=[1, 1, 1]),
        "no source views": case([(0, 2)], src_blocks=()),
        "a block in both tables": case([(0, 2)], src=src_small() + [[(2, 5)]], src_blocks=(6, 7, 8, 2)),
        "a block in both tables, skipped": case([(0, 2)], src=src_small() + [[(2, 5)]], src_blocks=(6, 7, 8, 2), skip=[0, 0, 0, 1]),
        "a kept feature at the capacity": case([(0, 2)], src=src_small() + [[(7, 8)]]),
        "a dropped feature at the capacity": case([(0, 2)], src=src_small() + [[(4, 8)]]),
        "descending starts in the destination": case([(0, 2)], dst_start=[0, 3, 2, 9, 10, 10, 12]),
        "descending starts in the source": case([(0, 2)], src_start=[0, 3, 5, 4, 8, 9, 10, 13]),
        "a last start above n_obs": case([(0, 2)], src_start=[0, 3, 5, 8, 8, 9, 10, 99]),
        "a map count above its room": case([(0, 2), (1, 1), (4, 0)], map_room=2, map_count=7),
        "a map count below its room": case([(0, 2), (1, 1), (4, 0)], map_room=3, map_count=1),
        "an empty destination": case([(0, 0)], dst=[]),
        "an empty source": case([(0, 0)], src=[]),
        "both empty": case([], dst=[], src=[]),
        "rooms above the least": case([(0, 2)], extra_room=5),
    }


def random_incorporate(seed, n_dst=30, n_src=30, dst_views=5, src_views=5, cap=8, n_pairs=8, collide=True, skip=True, extra_room=0):
    """Two clean tables (a feature in one row, a view at most once per row) over disjoint blocks but for the bridging frame's,
    which both name; a map of n_pairs entries from the bridging frame's features — with `collide` some name a landmark twice."""
    rng = np.random.default_rng(seed)
    bridge = dst_views
    n_blocks = dst_views + 1 + src_views

    def rows(n, blocks):
        used = {b: 0 for b in blocks}
        out = []
        for _ in range(n):
            row = []
            for b in rng.permutation(blocks)[:rng.integers(0, len(blocks) + 1)]:
                if used[int(b)] < cap:
                    row.append((int(b), used[int(b)]))
                    used[int(b)] += 1
            out.append(row)
        return out

    dst_rows = rows(n_dst, list(range(dst_views)) + [bridge] * (n_dst > 0))
    src_blocks = list(range(dst_views + 1, n_blocks))
    src_rows = rows(n_src, src_blocks + [bridge] * (n_src > 0))
    with_bridge = lambda rs: [k for k, r in enumerate(rs) if any(b == bridge for b, _ in r)]
    cs, cd = with_bridge(src_rows), with_bridge(dst_rows)
    n = min(n_pairs, len(cs), len(cd))
    ps, pd = list(rng.permutation(cs)[:n]), list(rng.permutation(cd)[:n])
    pairs = [(int(s), int(d)) for s, d in zip(ps, pd)]
    if collide and n >= 3:
        pairs[1] = (pairs[1][0], pairs[0][1])
        pairs.append((pairs[2][0], int(rng.integers(0, max(n_dst, 1)))))
    order = list(rng.permutation(src_blocks))
    sk = [int(rng.random() < 0.2) for _ in order] if skip else None
    return incorporate_inputs(dst_rows, src_rows, pairs, [int(b) for b in order], bridge, cap=cap, n_blocks=n_blocks, skip=sk, seed=seed,
                              extra_room=extra_room)


# ---- the map ----------------------------------------------------------------------------------------------------------
def map_inputs(matches, final=None, cap=8, count=None, slot=1, n_slots=3, n_world=6, n_dst=6, best=None, src_landmarks=None, bridge_block=2,
               n_blocks=4, nmatches=None):
    """Every array of an rs_merge_map_device call: matches [(feature, world row)] of slot `slot`, final flags (default all set),
    best {feature: (a, b)} or None for no d_best, src_landmarks {feature: key} of the bridging frame in the source."""
    m = np.full((n_slots, cap, 2), FILL32, np.uint32)
    fm = np.full((n_slots, cap), FILL8, np.uint8)
    nm = np.zeros(n_slots, np.uint32)
    if len(matches):
        m[slot, :len(matches)] = np.array(matches, np.uint32).reshape(-1, 2)[:cap]
    fm[slot, :len(matches)] = np.array([1] * len(matches) if final is None else final, np.uint8)[:cap]
    nm[slot] = len(matches) if nmatches is None else nmatches
    d_best = None
    if best is not None:
        d_best = np.full((n_slots, cap, 3, 2), NONE, np.uint32)
        for j, (a, b) in best.items():
            d_best[slot, j, 0], d_best[slot, j, 1] = (a, 0), (b, 0)
    counts = np.zeros(n_blocks, np.uint32)
    counts[bridge_block] = cap if count is None else count
    lm = np.full((n_blocks, cap), NONE, np.uint32)
    for j, key in (src_landmarks or {}).items():
        lm[bridge_block, j] = key
    return dict(matches=m, nmatches=nm, final=fm, best=d_best, n_world=n_world, n_dst=n_dst, cap=cap, slot=slot, counts=counts, src_landmarks=lm,
                n_blocks=n_blocks, bridge_block=bridge_block)


def map_outputs(inp):
    return dict(map=np.full((inp["cap"], 2), FILL32, np.uint32), map_count=np.full(1, FILL32, np.uint32))


def merge_map(inp):
    """rs_merge_map_device on the host -> dict(map, map_count)"""
    o = map_outputs(inp)
    r = lib().mr_merge_map(_p(inp["matches"]), _p(inp["nmatches"]), _p(inp["final"]), _p(inp["best"]), inp["n_world"], inp["n_dst"], inp["cap"],
                           inp["slot"], _p(inp["counts"]), _p(inp["src_landmarks"]), inp["n_blocks"], inp["bridge_block"], _p(o["map"]),
                           _p(o["map_count"]))
    assert r == 0
    return o


def designed_map_cases():
    """name -> (inputs, the map the statement's terms give).  n_world = n_dst = 6, cap = 8, slot 1: merged rows are 6 + 8 + feature."""
    src = {j: 10 + j for j in range(8)}
    full = [(j, j % 6) for j in range(8)]
    return {
        "no matches": (map_inputs([], src_landmarks=src), []),
        "one match": (map_inputs([(3, 2)], src_landmarks=src), [(13, 2)]),
        "cap matches, handed over in descending feature order": (map_inputs(full[::-1], src_landmarks=src), [(10 + j, j % 6) for j in range(8)]),
        "a merged row takes best[0]": (map_inputs([(5, 6 + 8 + 5), (1, 4)], best={5: (3, 0)}, src_landmarks=src), [(11, 4), (15, 3)]),
        "features without a source landmark": (map_inputs([(0, 1), (2, 3), (4, 5)], src_landmarks={2: 7}), [(7, 3)]),
        "a match that is not final": (map_inputs([(0, 1), (2, 3)], final=[0, 1], src_landmarks=src), [(12, 3)]),
        "a match that names nothing": (map_inputs([(0, 6), (2, 3), (7, 1)], count=7, src_landmarks=src), [(12, 3)]),
        "a merged row without d_best": (map_inputs([(5, 6 + 8 + 5), (1, 4)], src_landmarks=src), [(11, 4)]),
        "a feature in two final matches takes the first": (map_inputs([(2, 3), (2, 4)], src_landmarks=src), [(12, 3)]),
        "a match count above the capacity": (map_inputs([(2, 3)], nmatches=9, src_landmarks=src), []),
        "a count above the capacity": (map_inputs([(2, 3)], count=9, src_landmarks=src), []),
    }


# ---- normalise ----------------------------------------------------------------------------------------------------------
def normalize_inputs(seed, n_features, n_views, cap=None, n_constraints=3, n_blocks=None, w_zero=(), none=(), no_landmark=(), world_pad=2):
    """A reconstruction of n_views views (blocks in a shuffled order) whose first view has n_features features, feature j on
    landmark j with a world point at distance 1 to 20 from that view; `w_zero` / `none` / `no_landmark`: features whose world row
    has w == 0 / is akz_tri_none / whose landmark is outside the world table."""
    rng = np.random.default_rng(seed)
    cap = max(n_features, 1) if cap is None else cap
    n_blocks = n_views + 2 if n_blocks is None else n_blocks
    blocks = rng.permutation(n_blocks)[:n_views].astype(np.uint32)
    poses = np.stack([random_pose(rng) for _ in range(n_blocks)])
    counts = np.zeros(n_blocks, np.uint32)
    counts[blocks[0]] = n_features
    lm = np.full((n_blocks, cap), NONE, np.uint32)
    n_world = n_features + world_pad
    world = np.zeros((max(n_world, 1), 4))
    world[:, 3] = -1.0
    first = poses[blocks[0]].reshape(3, 4)
    for j in range(n_features):
        lm[blocks[0], j] = j
        d = rng.normal(size=3)
        cam = d / np.linalg.norm(d) * rng.uniform(1.0, 20.0)
        p = first[:, :3].T @ (cam - first[:, 3])
        w = 1.0 / np.linalg.norm(p)
        world[j] = np.concatenate([p * w, [w]])
        if j in w_zero:
            world[j, 3] = 0.0 if j % 2 else -0.0
        if j in none:
            world[j] = (0.0, 0.0, 0.0, -1.0)
        if j in no_landmark:
            lm[blocks[0], j] = n_world + j
    cposes = np.stack([random_pose(rng) for _ in range(2 * max(n_constraints, 1))]).reshape(-1, 2, 12)
    return dict(view_blocks=blocks, counts=counts, landmarks=lm, cap=cap, n_blocks=n_blocks, world=world, n_world=n_world, poses=poses,
                constraint_poses=cposes, n_constraints=n_constraints)


def normalize_outputs(inp):
    return dict(poses=inp["poses"].copy(), constraint_poses=inp["constraint_poses"].copy(), stats=np.full(2, FILL64), verdict=np.full(1, FILL32, np.uint32))


def normalize(inp):
    """rs_normalize_reconstruction_device on the host -> dict(poses, constraint_poses, stats, verdict)"""
    o = normalize_outputs(inp)
    lib().mr_normalize(_p(inp["view_blocks"]), len(inp["view_blocks"]), _p(inp["counts"]), _p(inp["landmarks"]), inp["cap"], inp["n_blocks"],
                       _p(inp["world"]), inp["n_world"], _p(o["poses"]), _p(o["constraint_poses"]) if inp["n_constraints"] else None,
                       inp["n_constraints"], _p(o["stats"]), _p(o["verdict"]))
    return o


def check_normalize_against_statement(inp, o, bound):
    """-> the largest absolute difference of the mean, the poses and the constraint poses from the float64 statement"""
    import reconstruction_merge_statement as S
    st = S.normalize([int(b) for b in inp["view_blocks"]], inp["counts"], inp["landmarks"], inp["world"][:inp["n_world"]], inp["poses"],
                     inp["constraint_poses"][:inp["n_constraints"]], inp["cap"], inp["n_blocks"])
    assert int(o["verdict"][0]) == st["verdict"]
    assert o["stats"][1] == st["count"]
    diff = abs(float(o["stats"][0]) - st["mean"])
    if st["verdict"] != NR_OK:
        assert np.array_equal(o["poses"], inp["poses"]) and np.array_equal(o["constraint_poses"], inp["constraint_poses"])
    diff = max(diff, float(np.max(np.abs(o["poses"] - st["poses"]))))
    if inp["n_constraints"]:
        diff = max(diff, float(np.max(np.abs(o["constraint_poses"][:inp["n_constraints"]] - st["constraint_poses"]))))
    assert np.array_equal(o["constraint_poses"][inp["n_constraints"]:], inp["constraint_poses"][inp["n_constraints"]:])
    assert diff <= bound, diff
    return diff


def designed_normalize_cases():
    return {
        "no robust point": normalize_inputs(1, 5, 3, none=range(5)),
        "no feature": normalize_inputs(2, 0, 3),
        "one point": normalize_inputs(3, 1, 3),
        "a point at w == 0": normalize_inputs(4, 6, 3, w_zero=(1, 4)),
        "only points at w == 0": normalize_inputs(5, 2, 2, w_zero=(0, 1)),
        "a landmark outside the world table": normalize_inputs(6, 6, 3, no_landmark=(2,)),
        "a constraint array of length 0": normalize_inputs(7, 9, 4, n_constraints=0),
        "one view": normalize_inputs(8, 9, 1),
        "a capacity above the count": normalize_inputs(9, 5, 3, cap=8),
    }
