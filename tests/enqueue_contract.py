"""The enqueue contract of include/akz.h as a table of calls, and the protocol that holds an entry to it.

Every `*_device` entry takes a `stream_to_wait`: the stream that produces its device inputs.  The entry orders its own work
behind that stream and returns; a host index list is read before it returns.  The GPU tests of the stages upload their inputs
and wait before they call, so none of them would notice an entry that drops the wait, orders one of two internal streams, reads
a device word on the host too early or goes on reading a host list.  tests/test_gpu_enqueue_contract.py calls every row of
ROWS with a producer that is still running; this module is the part that needs no GPU: the rows, their inputs, the bounds the
inputs keep (tests/test_enqueue_contract_cases.py), and the protocol as functions that take `torch`.

A row builds one call from a seed -> Call: the device inputs and the host lists as numpy arrays, the output buffers under their
fill, the scalars, and `args`, which lays the raw arguments of the symbol out.  TRUE is the call of one seed, DECOY that of
another: equal shapes, equal scalars, and BOTH valid inputs of the entry — every index in range, every start table ascending,
every count at most its capacity — because the entry under test may read either."""
import ctypes as C

import numpy as np

NONE = 0xFFFFFFFF
SEED_TRUE, SEED_DECOY = 1, 2


class Call:
    """One call of an entry point, on the host.  ins: {name: array} the device inputs; lists: {name: uint32 array} the host index
    lists; outs: {name: array under its fill} the device outputs — a name that is in `ins` too is updated in place and starts as
    the input; scalars: {name: value}; args(d, l, wait): the arguments behind the context handle, d[name] the device buffer of an
    input or output, l[name] = (ctypes array, count) of a list; check(): the bounds, as assertions."""

    def __init__(self, symbol, ins, outs, args, check, lists=None, scalars=None):
        self.symbol, self.ins, self.outs, self.args, self.check = symbol, ins, outs, args, check
        self.lists, self.scalars = lists or {}, scalars or {}

    def shapes(self):
        sig = lambda d: {k: (v.shape, v.dtype.str) for k, v in d.items()}
        return sig(self.ins), sig(self.outs), sig(self.lists), self.scalars


class Row:
    """name; family: which context the entry runs on ('rs', 'hm', 'akz'); build(seed) -> Call; host_list: the entry takes a
    host list; staged: it stages what its kernels read (the lists too) through the matcher's pinned ring.  An entry without a
    host list only records an event, waits for it and launches, and a staged one copies into pinned memory of its own: both
    must return while the producer is still busy.  An rs entry with a host list uploads it from the caller's pageable memory:
    whether that returns at once is the runtime's business, measured and not asserted."""

    def __init__(self, name, family, build, host_list=False, staged=False):
        self.name, self.family, self.build, self.host_list, self.staged = name, family, build, host_list, staged

    @property
    def must_return_early(self):
        return self.staged or not self.host_list

    def __repr__(self):
        return self.name


# ---- bounds ----------------------------------------------------------------------------------------------------------------
def ascending(start, limit):
    s = np.asarray(start, np.int64)
    assert len(s) >= 1 and s[0] >= 0 and np.all(np.diff(s) >= 0) and s[-1] <= limit, (s[:4], s[-1], limit)


def below(idx, n, none_ok=False):
    a = np.asarray(idx, np.int64).reshape(-1)
    if none_ok:
        a = a[a != NONE]
    assert a.size == 0 or (a.min() >= 0 and a.max() < n), (int(a.max()), n)


def one_to_one(block_map, n_out):
    m = np.asarray(block_map, np.int64)
    kept = m[m != NONE]
    below(kept, n_out)
    assert len(set(kept.tolist())) == len(kept)


def csr_obs(start, obs, n_blocks, cap):
    ascending(start, len(obs))
    used = np.asarray(obs)[:int(start[-1])]
    below(used[:, 0], n_blocks)
    below(used[:, 1], cap)


# ---- repack (cv_amd/csrc/rs_repack.hip) --------------------------------------------------------------------------------------
def _seeded_table(seed, n_blocks=9, n_rows=40, cap=64):
    """rows of 1, 2, 3, 5, 0 and 2 observations in turn — the lengths of repack_catalogue.small_rows, so that two seeds give
    equal starts — over views the seed draws; every feature of a view handed out once"""
    import repack_catalogue as cat
    rng = np.random.default_rng(seed)
    feats = cat.Features(n_blocks, cap)
    return [feats.row([int(v) for v in rng.permutation(n_blocks)[:(1, 2, 3, 5, 0, 2)[r % 6]]]) for r in range(n_rows)]


def _seeded_map(seed, n_blocks):
    """one view removed, the rest permuted -> (map, n_blocks_out)"""
    rng = np.random.default_rng(seed + 100)
    m = np.full(n_blocks, NONE, np.uint32)
    keep = rng.permutation(n_blocks)[:n_blocks - 1]
    m[keep] = rng.permutation(n_blocks - 1)
    return m, n_blocks - 1


def repack_table(seed):
    import repack_catalogue as cat
    nb = 9
    block_map, out = _seeded_map(seed, nb)
    case = cat.Case("seed_%d" % seed, _seeded_table(seed, nb), nb, block_map, out, recon_start=[0, 10, 10, 40])
    ins = dict(start=case.start, obs=np.ascontiguousarray(case.obs), map=case.map, recon_start=case.recon_start)
    outs = cat.blank(case)
    scalars = dict(n_obs=case.n_obs, n_landmarks=case.n_landmarks, cap=case.cap, n_blocks=nb, n_blocks_out=out, n_recons=3,
                   obs_room=case.obs_room, lm_room=case.lm_room)

    def args(d, l, wait):
        return (d["start"], d["obs"], case.n_obs, case.n_landmarks, case.cap, nb, d["map"], out, d["recon_start"], 3, case.obs_room, case.lm_room,
                d["obs_start_out"], d["obs_out"], d["obs_counts_out"], d["landmarks_out"], d["key_out"], d["recon_start_out"], d["counts_out"],
                d["call_verdict"], wait)

    def check():
        csr_obs(case.start, case.obs, nb, case.cap)
        one_to_one(case.map, out)
        ascending(case.recon_start, case.n_landmarks)
        assert case.n_obs <= case.obs_room and case.n_landmarks <= case.lm_room

    return Call("rs_repack_table_device", ins, outs, args, check, scalars=scalars)


def gather_blocks(seed):
    import repack_catalogue as cat
    nb, row_bytes = 9, 48
    block_map, out = _seeded_map(seed, nb)
    src = np.random.default_rng(seed).integers(0, 256, (nb, row_bytes)).astype(np.uint8)
    outs = dict(dst=np.full((out, row_bytes), 0xA5, np.uint8), verdict=np.full(1, cat.POISON, np.uint32))
    args = lambda d, l, wait: (d["src"], d["dst"], row_bytes, nb, d["map"], out, d["verdict"], wait)
    return Call("rs_gather_blocks_device", dict(src=src, map=block_map), outs, args, lambda: one_to_one(block_map, out),
                scalars=dict(row_bytes=row_bytes, n_blocks=nb, n_blocks_out=out))


def repack_constraints(seed):
    import repack_catalogue as cat
    nb, n = 9, 300
    rng = np.random.default_rng(seed)
    views = np.stack([rng.permutation(nb)[:3] for _ in range(n)]).astype(np.uint32)
    poses = rng.normal(size=(n, 2, 12))
    verdict = rng.integers(0, 3, n).astype(np.uint32)
    block_map, out = _seeded_map(seed, nb)
    start = np.array([0, 100, 100, n], np.uint32)
    w = lambda *shape: np.full(shape, cat.POISON, np.uint32)
    outs = dict(views_out=w(n, 3), poses_out=np.full((n, 2, 12), -7.0), verdict_out=w(n), count=w(1), start_out=w(len(start)))
    args = lambda d, l, wait: (d["views"], d["poses"], d["verdict"], n, d["map"], nb, out, d["start"], len(start) - 1, d["views_out"], d["poses_out"],
                               d["verdict_out"], d["count"], d["start_out"], wait)

    def check():
        below(views, nb)
        one_to_one(block_map, out)
        ascending(start, n)

    return Call("rs_repack_constraints_device", dict(views=views, poses=poses, verdict=verdict, map=block_map, start=start), outs, args, check,
                scalars=dict(n=n, n_blocks=nb, n_blocks_out=out, n_ranges=len(start) - 1))


def remap_views(seed):
    nb, n = 9, 300
    rng = np.random.default_rng(seed)
    block_map, _ = _seeded_map(seed, nb)
    recon = rng.integers(0, 3, n).astype(np.uint32)
    recon[rng.integers(0, n, 20)] = NONE                                           # free rows
    view = rng.integers(0, nb, n).astype(np.uint32)
    ins = dict(recon=recon, view=view, map=block_map)
    outs = dict(recon=recon.copy(), view=view.copy(), flags=np.full(1, 0xA5A5A5A5, np.uint32))
    args = lambda d, l, wait: (d["recon"], d["view"], n, 1, d["map"], nb, d["flags"], wait)
    return Call("hm_place_remap_views_device", ins, outs, args, lambda: (below(view, nb), below(block_map, nb, none_ok=True)),
                scalars=dict(n_stored=n, recon=1, n_blocks=nb))


# ---- merge (cv_amd/csrc/rs_reconstruction_merge.hip) --------------------------------------------------------------------------
def _pad_rows(a, n, fill):
    return a if len(a) == n else np.concatenate([a, np.full((n - len(a),) + a.shape[1:], fill, a.dtype)])


MERGE_OBS = 400                          # the room both seeds' observation arrays are padded to (rows behind a table are not its own)


def incorporate(seed):
    import reconstruction_merge_checker as K
    inp = K.random_incorporate(40 + seed, n_dst=60, n_src=50, dst_views=12, src_views=14, n_pairs=20, collide=True, skip=False)
    inp["map"], inp["map_room"] = _pad_rows(inp["map"], 24, K.FILL32), 24
    for side in ("dst", "src"):
        inp[side + "_obs"], inp["n_%s_obs" % side] = _pad_rows(inp[side + "_obs"], MERGE_OBS, K.FILL32), MERGE_OBS
    inp["obs_room"], inp["lm_room"] = 2 * MERGE_OBS, inp["n_dst"] + inp["n_src"]
    names = ("dst_start", "dst_obs", "src_start", "src_obs", "map", "map_count", "src_pose", "poses")
    ins = {k: inp[k] for k in names}
    outs = K.incorporate_outputs(inp)
    scalars = {k: inp[k] for k in ("n_dst_obs", "n_dst", "n_src_obs", "n_src", "map_room", "cap", "n_blocks", "bridge_block", "obs_room", "lm_room")}

    def args(d, l, wait):
        blocks, n = l["src_blocks"]
        return (d["dst_start"], d["dst_obs"], inp["n_dst_obs"], inp["n_dst"], d["src_start"], d["src_obs"], inp["n_src_obs"], inp["n_src"], d["map"],
                d["map_count"], inp["map_room"], inp["cap"], inp["n_blocks"], blocks, n, inp["bridge_block"], d["src_pose"], None, inp["obs_room"],
                inp["lm_room"]) + tuple(d[k] for k in K.IR_OUTPUTS) + (wait,)

    def check():
        ascending(inp["dst_start"], inp["n_dst_obs"])
        ascending(inp["src_start"], inp["n_src_obs"])
        csr_obs(inp["dst_start"], inp["dst_obs"], inp["n_blocks"], inp["cap"])
        csr_obs(inp["src_start"], inp["src_obs"], inp["n_blocks"], inp["cap"])
        assert int(inp["map_count"][0]) <= inp["map_room"]
        below(inp["src_blocks"], inp["n_blocks"])
        assert len(set(inp["src_blocks"].tolist())) == len(inp["src_blocks"]) and inp["bridge_block"] not in inp["src_blocks"]
        assert inp["n_dst_obs"] + inp["n_src_obs"] <= inp["obs_room"] and inp["n_dst"] + inp["n_src"] <= inp["lm_room"]

    return Call("rs_incorporate_reconstruction_device", ins, outs, args, check, lists=dict(src_blocks=inp["src_blocks"]), scalars=scalars)


def merge_map(seed):
    import reconstruction_merge_checker as K
    rng = np.random.default_rng(seed)
    cap, n_world, n_dst = 8, 6, 6
    feats = rng.permutation(cap)[:6]
    matches = [(int(f), int(rng.integers(0, n_world))) for f in feats]
    inp = K.map_inputs(matches, final=[int(v) for v in rng.integers(0, 2, len(matches))], cap=cap, n_world=n_world, n_dst=n_dst,
                       src_landmarks={int(j): int(10 + rng.integers(0, 20)) for j in rng.permutation(cap)[:6]})
    names = ("matches", "nmatches", "final", "counts", "src_landmarks")
    args = lambda d, l, wait: (d["matches"], d["nmatches"], d["final"], None, n_world, n_dst, cap, inp["slot"], d["counts"], d["src_landmarks"],
                               inp["n_blocks"], inp["bridge_block"], d["map"], d["map_count"], wait)

    def check():
        assert np.all(inp["nmatches"] <= cap) and np.all(inp["counts"] <= cap)
        below(inp["matches"][inp["slot"], :len(matches), 0], cap)

    return Call("rs_merge_map_device", {k: inp[k] for k in names}, K.map_outputs(inp), args, check,
                scalars=dict(n_world=n_world, n_dst=n_dst, cap=cap, slot=inp["slot"], n_blocks=inp["n_blocks"], bridge_block=inp["bridge_block"]))


def normalize(seed):
    import reconstruction_merge_checker as K
    inp = K.normalize_inputs(20 + seed, 9, 4, cap=12, n_constraints=3, n_blocks=6)
    ins = dict(counts=inp["counts"], landmarks=inp["landmarks"], world=inp["world"], poses=inp["poses"], constraint_poses=inp["constraint_poses"])
    args = lambda d, l, wait: (l["view_blocks"][0], l["view_blocks"][1], d["counts"], d["landmarks"], inp["cap"], inp["n_blocks"], d["world"],
                               inp["n_world"], d["poses"], d["constraint_poses"], inp["n_constraints"], d["stats"], d["verdict"], wait)

    def check():
        below(inp["view_blocks"], inp["n_blocks"])
        assert np.all(inp["counts"] <= inp["cap"])
        below(inp["landmarks"], inp["n_world"], none_ok=True)

    return Call("rs_normalize_reconstruction_device", ins, K.normalize_outputs(inp), args, check, lists=dict(view_blocks=inp["view_blocks"]),
                scalars={k: inp[k] for k in ("cap", "n_blocks", "n_world", "n_constraints")})


# ---- export (cv_amd/csrc/rs_export.hip) --------------------------------------------------------------------------------------
EXPORT_OBS = 200


def export(seed):
    import export_checker as E
    inp = E.random_export(30 + seed, 60, [6, 4, 5], cap=8)
    inp["obs"], inp["n_obs"] = _pad_rows(inp["obs"], EXPORT_OBS, E.FILL32), EXPORT_OBS
    names = ("world", "start", "obs", "colors", "counts", "landmarks", "poses")
    scalars = {k: inp[k] for k in ("n_world", "n_obs", "n_landmarks", "cap", "n_blocks", "room")}

    def args(d, l, wait):
        blocks, n = l["view_blocks"]
        return (d["world"], inp["n_world"], d["start"], d["obs"], inp["n_obs"], inp["n_landmarks"], d["colors"], blocks, n, d["counts"],
                d["landmarks"], inp["cap"], inp["n_blocks"], d["poses"], inp["room"]) + tuple(d[k] for k in E.OUTPUTS) + (wait,)

    def check():
        csr_obs(inp["start"], inp["obs"], inp["n_blocks"], inp["cap"])
        below(inp["view_blocks"], inp["n_blocks"])
        assert np.all(inp["counts"] <= inp["cap"]) and inp["n_landmarks"] <= inp["n_world"]

    return Call("rs_export_reconstruction_device", {k: inp[k] for k in names}, E.outputs(inp), args, check,
                lists=dict(view_blocks=inp["view_blocks"]), scalars=scalars)

# ---- the bootstrap tables (cv_amd/csrc/rs_bootstrap_table.hip) -----------------------------------------------------------------
def join_pairs(seed):
    import bootstrap_table_checker as B
    cap, rng = 64, np.random.default_rng(seed)
    slots = [B.drawn_slot(rng, cap, 60, 40 + k, centres=50) for k in range(4)]
    scenes = [tuple(int(v) for v in rng.permutation(4)[:2]) for _ in range(5)]
    inp = B.join_inputs(slots, scenes, cap, minimum=8, shuffle=True, seed=0x0123456789ABCDEF)
    names = ("pairs", "npairs", "inliers", "n_inliers", "best_id", "pose")

    def args(d, l, wait):
        (a, n), (b, _) = l["slot_first"], l["slot_second"]
        return tuple(d[k] for k in names) + (inp["n_slots"], cap, a, b, n, inp["minimum"], inp["flags"], inp["seed"]) + \
            tuple(d[k] for k in B.JOIN_OUTPUT_NAMES) + (wait,)

    def check():
        below(inp["slot_first"], inp["n_slots"])
        below(inp["slot_second"], inp["n_slots"])
        assert np.all(inp["npairs"] <= cap) and np.all(inp["n_inliers"] <= inp["npairs"])
        for k in range(inp["n_slots"]):
            below(inp["pairs"][k, :inp["npairs"][k]], cap)
            below(inp["inliers"][k, :inp["n_inliers"][k]], inp["npairs"][k])

    return Call("rs_join_pairs_batch_device", {k: inp[k] for k in names}, B.join_outputs(inp), args, check,
                lists=dict(slot_first=inp["slot_first"], slot_second=inp["slot_second"]),
                scalars={k: inp[k] for k in ("n_slots", "cap", "n_scenes", "minimum", "flags", "seed")})


def add_reconstruction(seed):
    import bootstrap_table_checker as B
    cap, rng = 64, np.random.default_rng(seed)
    blocks = [int(b) for b in rng.permutation(6)]
    scenes = [B.drawn_scene(rng, blocks[:3], (60, 64, 33), cap, (9, 5, 5)), B.drawn_scene(rng, blocks[3:], (64, 40, 50), cap, (7, 3, 7))]
    inp = B.add_inputs(scenes, cap, 6, 7, 1, counts=np.full(6, cap, np.uint32), seed=seed)
    names = ("triples", "ntriples", "first_only", "nfirst", "second_only", "nsecond", "combined", "first_ok", "second_ok", "pose_out", "tv_verdict")

    def args(d, l, wait):
        (a, n), (b, _), (c, _) = l["ic"], l["i_first"], l["i_second"]
        return tuple(d[k] for k in names) + (a, b, c, n, d["kps"], d["counts"], 6, cap, None, None, None, 0, 0, None, None, 0) + \
            tuple(d[k] for k in B.ADD_OUTPUT_NAMES[:3]) + (inp["n_blocks"], inp["view_base"], inp["obs_room"], inp["lm_room"]) + \
            tuple(d[k] for k in B.ADD_OUTPUT_NAMES[3:]) + (wait,)

    def check():
        frames = np.concatenate([inp["ic"], inp["i_first"], inp["i_second"]])
        below(frames, 6)
        assert len(set(frames.tolist())) == len(frames) and inp["view_base"] + len(frames) <= inp["n_blocks"]
        assert np.all(inp["counts"] <= cap)
        for k, w in (("triples", "ntriples"), ("first_only", "nfirst"), ("second_only", "nsecond")):
            assert np.all(inp[w] <= cap)
            for s in range(inp["n_scenes"]):
                below(inp[k][s, :inp[w][s]], cap)

    return Call("rs_add_reconstruction_batch_device", {k: inp[k] for k in names + ("kps", "counts")}, B.add_outputs(inp), args, check,
                lists=dict(ic=inp["ic"], i_first=inp["i_first"], i_second=inp["i_second"]),
                scalars={k: inp[k] for k in ("n_scenes", "n_src_blocks", "cap", "n_blocks", "view_base", "obs_room", "lm_room")})


# ---- the landmark table (cv_amd/csrc/rs_landmark_table.hip) ----------------------------------------------------------------------
TABLE_OBS = 160


def add_views(seed):
    import landmark_table_checker as L
    inp = L.random_call(60 + seed, n_landmarks=40, n_views=6, n_frames=3, cap=48, merges=2, collide=True)
    grow = inp["n_frames"] * inp["cap"]
    inp["obs"], inp["n_obs"] = _pad_rows(inp["obs"], TABLE_OBS, L.FILL32), TABLE_OBS
    inp["obs_room"], inp["lm_room"] = TABLE_OBS + grow, inp["n_landmarks"] + grow
    inp["skip"] = np.zeros(inp["n_frames"], np.uint32) if inp["skip"] is None else inp["skip"]
    names = ("start", "obs", "counts", "matches", "nmatches", "final", "verdict", "pose_out", "best", "skip", "poses")

    def args(d, l, wait):
        blocks, n = l["ik"]
        return (d["start"], d["obs"], inp["n_obs"], inp["n_landmarks"], inp["n_world"], None, None, 0, inp["cap"], inp["n_blocks"], blocks, n,
                d["counts"], d["matches"], d["nmatches"], d["final"], d["verdict"], d["pose_out"], d["best"], d["skip"], inp["obs_room"],
                inp["lm_room"]) + tuple(d[k] for k in L.OUTPUT_NAMES) + (wait,)

    def check():
        csr_obs(inp["start"], inp["obs"], inp["n_blocks"], inp["cap"])
        below(inp["ik"], inp["n_blocks"])
        assert len(set(inp["ik"].tolist())) == len(inp["ik"]) and np.all(inp["counts"] <= inp["cap"]) and np.all(inp["nmatches"] <= inp["cap"])
        for f in range(inp["n_frames"]):
            m = inp["matches"][f, :inp["nmatches"][f]]
            below(m[:, 0], inp["cap"])
            below(m[:, 1], inp["n_world"] + inp["n_frames"] * inp["cap"])
        below(inp["best"][..., 0], inp["n_landmarks"], none_ok=True)

    return Call("rs_add_views_device", {k: inp[k] for k in names}, L.outputs(inp), args, check, lists=dict(ik=inp["ik"]),
                scalars={k: inp[k] for k in ("n_obs", "n_landmarks", "n_world", "cap", "n_blocks", "n_frames", "obs_room", "lm_room")})


def sharing_view(seed):
    import landmark_table_checker as L
    rng = np.random.default_rng(seed)
    inp = L.random_call(80 + seed, n_landmarks=40, n_views=6, n_frames=2, cap=48)
    F, cap, n_lm = 2, 48, inp["n_landmarks"]
    best = np.full((F, cap, 3, 2), NONE, np.uint32)
    best[:, :, :2, 0] = rng.integers(0, n_lm, (F, cap, 2))
    best[:, :, :, 1] = 7
    decision = rng.integers(0, 3, (F, cap)).astype(np.uint32)
    obs = _pad_rows(inp["obs"], TABLE_OBS, L.FILL32)
    ins = dict(start=inp["start"], obs=obs, best=best, decision=decision)
    args = lambda d, l, wait: (d["start"], d["obs"], TABLE_OBS, n_lm, d["best"], d["decision"], cap, F, d["mask"], wait)
    return Call("rs_landmarks_sharing_view_device", ins, dict(mask=np.full((F, cap), L.FILL8, np.uint8)), args,
                lambda: (ascending(inp["start"], TABLE_OBS), below(best[:, :, :2, 0], n_lm)), scalars=dict(n_obs=TABLE_OBS, n_landmarks=n_lm, cap=cap, n_frames=F))


# ---- the pose graph (cv_amd/csrc/rs_pose_graph.hip) ------------------------------------------------------------------------------
def _graph(seed, n=40, n_views=9):
    import reconstruction_merge_checker as K
    rng = np.random.default_rng(seed)
    views = np.stack([rng.permutation(n_views)[:3] for _ in range(n)]).astype(np.uint32)
    poses = np.stack([K.random_pose(rng, 2.0) for _ in range(2 * n)]).reshape(n, 24)
    verdict = (rng.random(n) < 0.2).astype(np.uint32)
    return views, poses, verdict


def pose_graph_rows(seed):
    n, n_views = 40, 9
    views, _, _ = _graph(seed, n, n_views)
    w = lambda k: np.full(k, 0xA5A5A5A5, np.uint32)
    args = lambda d, l, wait: (d["views"], n, n_views, d["row_start"], d["row_edges"], d["flags"], wait)
    return Call("rs_pose_graph_rows_device", dict(views=views), dict(row_start=w(n_views + 1), row_edges=w(6 * n), flags=w(1)), args,
                lambda: below(views, n_views), scalars=dict(n=n, n_views=n_views))


def pose_graph_edges(seed):
    n = 40
    views, poses, verdict = _graph(seed, n)
    args = lambda d, l, wait: (d["views"], d["poses"], d["verdict"], n, d["edges"], wait)
    return Call("rs_pose_graph_edges_device", dict(views=views, poses=poses, verdict=verdict), dict(edges=np.full((n, 6, 12), -7.0)), args,
                lambda: below(views, 9), scalars=dict(n=n))

# ---- the matcher (cv_amd/csrc/hm_match.hip, hm_place.hip) ---------------------------------------------------------------------------
HM_CAP, HM_BLOCKS = 128, 6
NB = np.dtype([("index", "<u4"), ("distance", "<u4")])


def _descriptor_blocks(seed, n_blocks=HM_BLOCKS, cap=HM_CAP):
    """n_blocks blocks of cap descriptors: every block is a permutation of one random set with ten bits of each row flipped, so
    that any two blocks match in many rows; counts between 100 and cap -> (blocks [n][cap][64] u8, counts [n] u32)"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (cap, 64), dtype=np.uint8)
    blocks = np.stack([base[rng.permutation(cap)] for _ in range(n_blocks)])
    for _ in range(10):
        blocks[np.arange(n_blocks)[:, None], np.arange(cap)[None, :], rng.integers(0, 64, (n_blocks, cap))] ^= \
            (1 << rng.integers(0, 8, (n_blocks, cap))).astype(np.uint8)
    return blocks, rng.integers(100, cap + 1, n_blocks).astype(np.uint32)


def _problems(seed, n):
    rng = np.random.default_rng(seed + 7)
    return rng.integers(0, HM_BLOCKS, n).astype(np.uint32), rng.integers(0, HM_BLOCKS, n).astype(np.uint32)


def knn_batch(seed):
    blocks, counts = _descriptor_blocks(seed)
    n, k = 7, 3
    iq, it = _problems(seed, n)
    args = lambda d, l, wait: (d["blocks"], d["counts"], d["blocks"], d["counts"], HM_CAP, l["iq"][0], l["it"][0], n, k, d["out"], wait)
    return Call("hm_knn_batch_device", dict(blocks=blocks, counts=counts), dict(out=np.full((n, HM_CAP, k, 2), NONE, np.uint32)), args,
                lambda: (below(iq, HM_BLOCKS), below(it, HM_BLOCKS), below(counts, HM_CAP + 1)), lists=dict(iq=iq, it=it),
                scalars=dict(cap=HM_CAP, n_probs=n, k=k))


def match_batch(seed):
    blocks, counts = _descriptor_blocks(seed)
    n = 7
    ia, ib = _problems(seed, n)
    args = lambda d, l, wait: (d["blocks"], d["counts"], d["blocks"], d["counts"], HM_CAP, l["ia"][0], l["ib"][0], n, 1, 24, 0.0, 1, d["pairs"],
                               d["n_out"], wait)
    outs = dict(pairs=np.full((n, HM_CAP, 2), NONE, np.uint32), n_out=np.full(n, NONE, np.uint32))
    return Call("hm_match_batch_device", dict(blocks=blocks, counts=counts), outs, args,
                lambda: (below(ia, HM_BLOCKS), below(ib, HM_BLOCKS), below(counts, HM_CAP + 1)), lists=dict(ia=ia, ib=ib),
                scalars=dict(cap=HM_CAP, n_pairs=n, rule=1, param_u=24, symmetric=1))


def hash_bag(seed):
    blocks, counts = _descriptor_blocks(seed, 3)
    ncw = 64
    codewords = np.random.default_rng(seed + 5).integers(0, 256, (ncw, 64), dtype=np.uint8)
    args = lambda d, l, wait: (d["blocks"], d["counts"], HM_CAP, 3, d["codewords"], ncw, d["hash"], d["words"], wait)
    outs = dict(hash=np.full((3, ncw // 8), 0xEE, np.uint8), words=np.full((3, HM_CAP, 2), NONE, np.uint32))
    return Call("hm_hash_bag_device", dict(blocks=blocks, counts=counts, codewords=codewords), outs, args, lambda: below(counts, HM_CAP + 1),
                scalars=dict(cap=HM_CAP, n_frames=3, n_codewords=ncw))


def best_of_views_batch(seed):
    import matching_statement as S
    n_views, k, F = 5, 3, 2
    frames = [S.best_of_views_case(n_views, k, nq=40, better_by=24, seed=10 * seed + f) for f in range(F)]
    cap, nblk = frames[0]["cap"], n_views + 2
    ins = dict(knn=np.stack([c["nb"] for c in frames]), nq=np.array([7, 40, 33], np.int32), landmarks=np.concatenate([c["landmarks"] for c in frames]),
               counts=np.concatenate([c["counts"] for c in frames]))
    views = np.stack([c["view_sel"] + f * nblk for f, c in enumerate(frames)]).astype(np.uint32)
    iq = np.array([1, 2] if seed == SEED_TRUE else [2, 1], np.uint32)
    args = lambda d, l, wait: (d["knn"], d["nq"], l["iq"][0], cap, l["views"][0], F, n_views, k, d["landmarks"], d["counts"], 24, d["best"],
                               d["decision"], wait)
    outs = dict(best=np.full((F, cap, 3, 2), 0xEEEEEEEE, np.uint32), decision=np.full((F, cap), 0xEEEEEEEE, np.uint32))

    def check():
        below(views, F * nblk)
        below(iq, 3)
        below(ins["nq"], cap + 1)
        below(ins["knn"]["index"], cap)
        assert np.all(ins["counts"] <= cap)

    return Call("hm_best_of_views_batch_device", ins, outs, args, check, lists=dict(iq=iq, views=views),
                scalars=dict(cap=cap, n_frames=F, n_views=n_views, k=k, better_by=24))


def _landmark_entry(symbol, head, tail):
    """the four landmark entries take one frame layout: (best, decision, *head, nq, iq, cap, F, *tail, pairs, npairs)"""
    def build(seed):
        import matching_statement as S
        cap, n_world, F = 512, 4000, 2
        cases = [S.landmark_case("mixed", cap, n_world, seed=10 * seed + f) for f in range(F)]
        world = np.ones((n_world + F * cap, 4), np.float64)
        for f, c in enumerate(cases):
            world[n_world + f * cap:n_world + (f + 1) * cap, 3] = np.where(c["world_ok"], 0.0, -1.0)
        world[:n_world, 3] = np.where(cases[0]["world_lm"], 1.0, -1.0)
        ins = dict(best=np.stack([c["best"] for c in cases]), decision=np.stack([c["decision"] for c in cases]),
                   merge_ok=np.stack([c["merge_ok"] for c in cases]), obs=cases[0]["obs"], nq=np.array([cap, cap - 9, cap - 40], np.int32), world=world)
        ins = {k: v for k, v in ins.items() if k in ("best", "decision", "nq") + head + tail}
        iq = np.random.default_rng(seed).permutation(3)[:F].astype(np.uint32)
        args = lambda d, l, wait: (d["best"], d["decision"]) + tuple(d[k] for k in head) + (d["nq"], l["iq"][0], cap, F) + \
            tuple(d[k] for k in tail) + (n_world, d["pairs"], d["npairs"], wait)
        outs = dict(pairs=np.full((F, cap, 2), NONE, np.uint32), npairs=np.full(F, NONE, np.uint32))
        return Call(symbol, ins, outs, args, lambda: (below(iq, 3), below(ins["nq"], cap + 1)), lists=dict(iq=iq),
                    scalars=dict(cap=cap, n_frames=F, n_world=n_world))
    return build


landmark_pairs = _landmark_entry("hm_landmark_pairs_batch_device", (), ("world",))
landmark_matches = _landmark_entry("hm_landmark_matches_batch_device", ("merge_ok",), ("world",))
landmark_matches_ordered = _landmark_entry("hm_landmark_matches_ordered_batch_device", ("merge_ok", "obs"), ("world",))
landmark_original_matches = _landmark_entry("hm_landmark_original_matches_batch_device", ("merge_ok", "obs"), ())


def knn_views(seed):
    blocks, counts = _descriptor_blocks(seed)
    n_views, k = 4, 3
    view_idx = np.random.default_rng(seed + 9).permutation(HM_BLOCKS)[:n_views].astype(np.uint32)
    query, nq = blocks[0][np.random.default_rng(seed + 11).permutation(HM_CAP)], np.array([HM_CAP - 5], np.uint32)
    args = lambda d, l, wait: (d["query"], d["nq"], d["blocks"], d["counts"], HM_CAP, l["view_idx"][0], n_views, k, d["out"], wait)
    return Call("hm_knn_views_device", dict(query=query, nq=nq, blocks=blocks, counts=counts), dict(out=np.full((n_views, HM_CAP, k, 2), NONE, np.uint32)),
                args, lambda: (below(view_idx, HM_BLOCKS), below(counts, HM_CAP + 1)), lists=dict(view_idx=view_idx),
                scalars=dict(cap=HM_CAP, n_views=n_views, k=k))


def best_of_views(seed):
    import matching_statement as S
    n_views, k = 5, 3
    c = S.best_of_views_case(n_views, k, nq=40, better_by=24, seed=20 + seed)
    cap = c["cap"]
    ins = dict(knn=c["nb"], nq=np.array([40], np.int32), landmarks=c["landmarks"], counts=c["counts"])
    args = lambda d, l, wait: (d["knn"], d["nq"], cap, l["views"][0], n_views, k, d["landmarks"], d["counts"], 24, d["best"], d["decision"], wait)
    outs = dict(best=np.full((cap, 3, 2), 0xEEEEEEEE, np.uint32), decision=np.full(cap, 0xEEEEEEEE, np.uint32))
    return Call("hm_best_of_views_device", ins, outs, args, lambda: (below(c["view_sel"], n_views + 2), below(c["nb"]["index"], cap)),
                lists=dict(views=c["view_sel"]), scalars=dict(cap=cap, n_views=n_views, k=k, better_by=24))


def find_frames(seed):
    import place_statement as P
    c = P.size_case(70, 9, hash_bytes=64, seed=seed)
    t, p = c["table"], c["params"]
    R = P.room(p)
    f = lambda *shape: np.full(shape, NONE, np.uint32)
    nq = len(c["queries"])
    ins = dict(hashes=t["hashes"], feed=t["feed"], pos=t["pos"], recon=t["recon"], view=t["view"], queries=c["queries"])
    outs = dict(found=f(nq, R), views_out=f(nq, R), group_recon=f(nq, R), group_start=f(nq, R + 1), free=f(nq, R), search=f(nq, p["search_num"], 2),
                counts=f(nq, P.COUNTS), verdict=f(nq))

    def args(d, l, wait):
        from cv_amd import _lib
        prm = _lib.PlaceParams(p["num_similar"], p["num_recent"], p["recent_threshold"], p["search_num"])
        return (d["hashes"], d["feed"], d["pos"], d["recon"], d["view"], 70, 64, d["queries"], None, nq, prm, R, d["found"], d["views_out"],
                d["group_recon"], d["group_start"], d["free"], d["search"], d["counts"], d["verdict"], wait)

    return Call("hm_find_frames_batch_device", ins, outs, args, lambda: below(c["queries"], 70), scalars=dict(n_stored=70, hash_bytes=64, nq=nq, room=R, **p))


# ---- extraction (cv_amd/csrc/akz_api.hip, akz_color.hip) -----------------------------------------------------------------------
AKZ_W, AKZ_H, AKZ_N, AKZ_CAP = 1392, 512, 2, 2048


def _frames(seed):
    """the two frames of tests/golden/kitti_pair.npz: in their order, swapped, upside down, mirrored — four batches, by the seed"""
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kitti_pair.npz"))
    a, b = z["frame0"], z["frame14"]
    batches = ((a, b), (b, a), (a[::-1], b[::-1]), (b[:, ::-1], a[:, ::-1]))
    return np.ascontiguousarray(np.stack(batches[(seed - 1) % len(batches)]))


def extract_batch(seed):
    imgs = _frames(seed)
    assert imgs.shape == (AKZ_N, AKZ_H, AKZ_W) and imgs.dtype == np.uint8
    outs = dict(kps=np.full((AKZ_N, AKZ_CAP, 28), 0xEE, np.uint8), descs=np.full((AKZ_N, AKZ_CAP, 64), 0xEE, np.uint8), n_out=np.full(AKZ_N, NONE, np.uint32))
    args = lambda d, l, wait: (d["imgs"], 0, AKZ_N, AKZ_W, AKZ_H, d["kps"], d["descs"], AKZ_CAP, d["n_out"], wait)
    return Call("akz_extract_batch_device", dict(imgs=imgs), outs, args, lambda: None, scalars=dict(fmt=0, n=AKZ_N, w=AKZ_W, h=AKZ_H, cap=AKZ_CAP))


def sample_colors(seed):
    rng = np.random.default_rng(seed)
    n, w, h, cap = 3, 64, 48, 100
    stride = 3 * w + 4
    rgb = rng.integers(0, 256, (n, h, stride), dtype=np.uint8)
    kps = np.zeros((n, cap), np.dtype([("x", "<f4"), ("y", "<f4"), ("response", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("octave", "<u4"), ("class_id", "<u4")]))
    kps["x"], kps["y"] = rng.uniform(0, w - 1, (n, cap)), rng.uniform(0, h - 1, (n, cap))
    counts = rng.integers(60, cap + 1, n).astype(np.uint32)
    args = lambda d, l, wait: (d["rgb"], n, w, h, stride, d["kps"], d["counts"], cap, d["colors"], wait)
    return Call("akz_sample_colors_batch_device", dict(rgb=rgb, kps=kps, counts=counts), dict(colors=np.full((n, cap, 3), 0xEE, np.uint8)), args,
                lambda: below(counts, cap + 1), scalars=dict(n=n, w=w, h=h, stride=stride, cap=cap))

# ---- the geometry stages ----------------------------------------------------------------------------------------------------------
GEO_VIEWS, GEO_LANDMARKS = 8, 200
GEO_OBS = 6 * GEO_LANDMARKS


def _scene(seed):
    """observation_filter_checker.scene with its observation array padded to one length for every seed: kps [views][landmarks],
    poses, cam, start, obs [GEO_OBS][2] (the rows behind the last start are {0, 0}: valid indices nobody's list holds)"""
    import observation_filter_checker as F
    sc = F.scene(200 + seed, n_views=GEO_VIEWS, n_landmarks=GEO_LANDMARKS, lengths=(2, 6))
    sc["obs"] = _pad_rows(sc["obs"], GEO_OBS, 0)
    return sc


def _camera(cam):
    from cv_amd import _lib
    return _lib.Camera(cam.fx, cam.fy, cam.cx, cam.cy, cam.skew, cam.k1, cam.use_k1, 0)


def _scene_check(sc):
    csr_obs(sc["start"], sc["obs"], GEO_VIEWS, GEO_LANDMARKS)


def filter_observations(seed):
    import observation_filter_checker as F
    sc = _scene(seed)
    n, room = GEO_LANDMARKS, GEO_OBS
    ins = dict(kps=sc["kps"], poses=sc["poses"], start=sc["start"], obs=sc["obs"], recon_start=np.array([0, n], np.uint32),
               view_start=np.array([0, GEO_VIEWS], np.uint32))
    b = lambda k: np.full(k, F.FILL8, np.uint8)
    w = lambda *shape: np.full(shape, F.FILL32, np.uint32)
    outs = dict(keep=b(room), state=b(n), reason=b(n), robust=b(n), start_out=w(n + 1), obs_out=w(room, 2), split_out=w(room, 2), counts=w(2),
                verdict=w(1), stats=w(1, F.STATS))

    def args(d, l, wait):
        from cv_amd.reconstruction import ObservationFilter
        return (d["kps"], GEO_LANDMARKS, GEO_VIEWS, d["poses"], _camera(sc["cam"]), d["start"], d["obs"], room, n, d["recon_start"], d["view_start"], 1,
                None, ObservationFilter.params(minimum_robust_landmarks=1)) + tuple(d[k] for k in outs) + (wait,)

    return Call("rs_filter_observations_device", ins, outs, args, lambda: _scene_check(sc), scalars=dict(n_obs=room, n_landmarks=n))


def triangulate_landmarks(seed):
    sc = _scene(seed)
    n = GEO_LANDMARKS
    outs = dict(world=np.full((n, 4), -7.0), reason=np.full(n, 0xEE, np.uint8))

    def args(d, l, wait):
        from cv_amd import triangulation
        return (d["kps"], GEO_LANDMARKS, GEO_VIEWS, d["poses"], _camera(sc["cam"]), d["start"], d["obs"], GEO_OBS, n, triangulation.make_params(),
                d["world"], d["reason"], wait)

    return Call("rs_triangulate_landmarks_device", dict(kps=sc["kps"], poses=sc["poses"], start=sc["start"], obs=sc["obs"]), outs, args,
                lambda: _scene_check(sc), scalars=dict(n_obs=GEO_OBS, n_landmarks=n))


def triangulate_merged(seed):
    sc = _scene(seed)
    rng = np.random.default_rng(seed)
    n, F_, cap = GEO_LANDMARKS, 2, GEO_LANDMARKS
    best = np.full((F_, cap, 3, 2), NONE, np.uint32)
    best[:, :, :2, 0] = rng.integers(0, n, (F_, cap, 2))
    best[:, :, :, 1] = 7
    ins = dict(kps=sc["kps"], poses=sc["poses"], start=sc["start"], obs=sc["obs"], best=best, decision=rng.integers(0, 3, (F_, cap)).astype(np.uint32),
               merge_ok=(rng.random((F_, cap)) < 0.7).astype(np.uint8))
    outs = dict(world=np.full((n + F_ * cap, 4), -7.0), reason=np.full((F_, cap), 0xEE, np.uint8))

    def args(d, l, wait):
        from cv_amd import triangulation
        return (d["kps"], cap, GEO_VIEWS, d["poses"], _camera(sc["cam"]), d["start"], d["obs"], GEO_OBS, n, triangulation.make_params(), d["best"],
                d["decision"], d["merge_ok"], F_, n, d["world"], d["reason"], wait)

    return Call("rs_triangulate_merged_device", ins, outs, args, lambda: (_scene_check(sc), below(best[:, :, :2, 0], n)),
                scalars=dict(n_obs=GEO_OBS, n_landmarks=n, n_frames=F_, n_world=n))


def covisibility_candidates(seed):
    import covisibility_checker as Cv
    import covisibility_statement as CS
    tab = Cv.random_table(300 + seed, n_views=12, n_landmarks=120, cap=100)
    p = CS.settings(limit=8, min_cov=1, min_lm=1, min_new=1)
    obs = _pad_rows(tab["obs"], 8 * 120, 0)
    targets = np.random.default_rng(seed).permutation(12)[:3].astype(np.uint32)
    ins = dict(start=tab["start"], obs=obs, reason=tab["reason"], targets=targets)
    outs = Cv.outputs(3, p)

    def args(d, l, wait):
        from cv_amd.covisibility import Covisibility
        prm = Covisibility.params(optimization_robust_covisibility_minimum_landmarks=p["min_cov"],
                                  optimization_maximum_three_view_constraints=p["max_constraints"], optimization_minimum_new_constraints=p["min_new"],
                                  optimization_minimum_landmarks=p["min_lm"], optimization_maximum_landmarks=p["max_lm"], candidate_limit=p["limit"],
                                  shuffle_seed=p["seed"])
        return (d["start"], d["obs"], len(obs), 120, 100, 12, d["reason"], d["targets"], 3, prm, d["views"], d["lm_start"], d["lm"], d["slot_count"],
                d["verdict"], d["stats"], wait)

    return Call("rs_covisibility_candidates_device", ins, outs, args, lambda: (csr_obs(tab["start"], obs, 12, 100), below(targets, 12)),
                scalars=dict(n_obs=len(obs), n_landmarks=120, cap=100, n_blocks=12, n_targets=3, **p))


def covisibility_record(seed):
    import covisibility_checker as Cv
    import covisibility_statement as CS
    rng = np.random.default_rng(seed)
    p = CS.settings(limit=8, min_cov=1, min_lm=1, min_new=1, max_constraints=4)
    n_targets, n_slots = 3, 24
    targets = rng.permutation(12)[:n_targets].astype(np.uint32)
    cverdict = rng.integers(0, 3, n_slots).astype(np.uint32)
    verdict = np.zeros(n_targets, np.uint32)
    stats = rng.integers(0, 8, (n_targets, Cv.STATS)).astype(np.uint32)
    ins = dict(cverdict=cverdict, targets=targets, graph_start=np.array([0, 5, 12], np.uint32), verdict=verdict, stats=stats)
    outs = dict(recorded=np.full(n_slots, Cv.FILL32, np.uint32), verdict=verdict.copy(), stats=stats.copy())

    def args(d, l, wait):
        from cv_amd.covisibility import Covisibility
        prm = Covisibility.params(optimization_robust_covisibility_minimum_landmarks=p["min_cov"],
                                  optimization_maximum_three_view_constraints=p["max_constraints"], optimization_minimum_new_constraints=p["min_new"],
                                  optimization_minimum_landmarks=p["min_lm"], optimization_maximum_landmarks=p["max_lm"], candidate_limit=p["limit"],
                                  shuffle_seed=p["seed"])
        return (d["cverdict"], d["targets"], n_targets, d["graph_start"], 2, prm, d["recorded"], d["verdict"], d["stats"], wait)

    return Call("rs_covisibility_record_device", ins, outs, args, lambda: (below(targets, 12), ascending(ins["graph_start"], 12)),
                scalars=dict(n_targets=n_targets, n_graphs=2, **p))


def pose_graph_relax(seed):
    import pose_graph_checker as P
    A = P.batch([P.Graph(500 + seed, 8, noise=1e-2), P.Graph(600 + seed, 5, noise=1e-2)])
    n_views, n_g, n_c = len(A["poses"]), 2, len(A["views"])
    ins = {k: A[k] for k in ("poses", "graph_start", "row_start", "row_edges", "views", "cverdict", "edges")}
    w = lambda *shape: np.full(shape, P.FILL32, np.uint32)
    outs = dict(poses=A["poses"].copy(), verdict=w(n_g), state=w(n_views), stats=w(n_g, P.STATS))

    def args(d, l, wait):
        from cv_amd.pose_graph import PoseGraph
        return (d["poses"], n_views, d["graph_start"], n_g, d["row_start"], d["row_edges"], len(A["row_edges"]), d["views"], d["cverdict"], d["edges"],
                n_c, PoseGraph.params(optimization_iterations=16), d["verdict"], d["state"], d["stats"], wait)

    def check():
        ascending(A["graph_start"], n_views)
        ascending(A["row_start"], len(A["row_edges"]))
        below(A["row_edges"], 6 * n_c)
        below(A["views"], n_views)

    return Call("rs_pose_graph_relax_batch_device", ins, outs, args, check, scalars=dict(n_views=n_views, n_graphs=n_g, n_rows=len(A["row_edges"]), n_c=n_c))


CHAIN_OBS = 4000


def optimize_reconstruction(seed):
    import observation_filter_checker as F
    import pose_graph_checker as P
    from test_gpu_observation_filter import chain_scene
    cs = chain_scene(seed)
    A, rounds = cs["A"], 2
    obs = _pad_rows(cs["obs"], CHAIN_OBS, 0)
    n_views, n_g, n_c, n_lm, n_obs = len(A["poses"]), len(A["graph_start"]) - 1, len(A["views"]), len(cs["start"]) - 1, CHAIN_OBS
    ins = {k: A[k] for k in ("poses", "graph_start", "row_start", "row_edges", "views", "cverdict", "edges")}
    ins.update(kps=cs["kps"], start=cs["start"], obs=obs, recon_start=cs["recon_start"])
    size = dict(verdict=4 * n_g, gv=4 * n_g, state=4 * n_views, pg_stats=4 * P.STATS * n_g, keep=n_obs, lm_state=n_lm, reason=n_lm, robust=n_lm,
                start_out=4 * (n_lm + 1), obs_out=8 * n_obs, split_out=8 * n_obs * rounds, counts=8 * rounds, rv=4 * n_g * rounds,
                of_stats=4 * F.STATS * n_g * rounds, world=32 * n_lm, world_reason=n_lm)
    outs = dict(poses=A["poses"].copy())
    outs.update({k: np.full(n, F.FILL8, np.uint8) for k, n in size.items()})

    def args(d, l, wait):
        from cv_amd.pose_graph import PoseGraph
        from cv_amd.reconstruction import ObservationFilter
        return (d["poses"], n_views, d["graph_start"], n_g, d["row_start"], d["row_edges"], len(A["row_edges"]), d["views"], d["cverdict"], d["edges"],
                n_c, PoseGraph.params(optimization_iterations=16), d["kps"], cs["kps"].shape[1], _camera(cs["cam"]), d["start"], d["obs"], n_obs, n_lm,
                d["recon_start"], ObservationFilter.params(reconstruction_optimization_iterations=rounds)) + tuple(d[k] for k in size) + (wait,)

    def check():
        csr_obs(cs["start"], obs, n_views, cs["kps"].shape[1])
        ascending(A["graph_start"], n_views)
        ascending(cs["recon_start"], n_lm)
        below(A["row_edges"], 6 * n_c)
        below(A["views"], n_views)

    return Call("rs_optimize_reconstruction_batch_device", ins, outs, args, check, scalars=dict(n_views=n_views, n_graphs=n_g, n_c=n_c, n_obs=n_obs, n_lm=n_lm))


def three_view_constraint(seed):
    import three_view_checker as K3
    import three_view_constraint_checker as TVC
    cap = 64
    kps, poses, views, lm_start, lm = TVC.device_arrays([TVC.scene(700 + 10 * seed + k, 40) for k in range(3)], cap)
    views = views[np.random.default_rng(seed).permutation(3)]
    n = len(views)
    outs = dict(pose_out=np.full((n, 24), -7.0), verdict=np.full(n, 0xA5A5A5A5, np.uint32), stats=np.full((n, TVC.STATS), 0xA5A5A5A5, np.uint32))

    def args(d, l, wait):
        from cv_amd.three_view import ThreeViewConstraints
        return (d["kps"], cap, len(kps), d["poses"], K3.rig_camera_dev(), d["views"], d["lm_start"], d["lm"], len(lm), n,
                ThreeViewConstraints.params(constraint_patience=128), d["pose_out"], d["verdict"], d["stats"], wait)

    return Call("rs_three_view_constraint_batch_device", dict(kps=kps, poses=poses, views=views, lm_start=lm_start, lm=lm), outs, args,
                lambda: (below(views, len(kps)), ascending(lm_start, len(lm)), below(lm, cap)), scalars=dict(cap=cap, n_blocks=len(kps), n_lm=len(lm), n=n))


def three_view_init(seed):
    import three_view_checker as K3
    cap, S = 128, 2
    rigs = [K3.Rig(800 + 10 * seed + s, 80, noise=0.5, perturb=2e-3, n_first=9, n_second=5, outliers=5) for s in range(S)]
    arrays = [r.scene_arrays(cap, shuffle_seed=seed + s) for s, r in enumerate(rigs)]
    order = np.random.default_rng(seed).permutation(S)                        # where scene s lies in the block pool
    kps = np.zeros((3 * S, cap), arrays[0][0].dtype)
    for s in range(S):
        kps[3 * order[s]:3 * order[s] + 3] = arrays[s][0]
    ins = dict(kps=kps, pose_first=np.stack([r.pose_in[0] for r in rigs]), pose_second=np.stack([r.pose_in[1] for r in rigs]),
               triples=np.stack([a[1] for a in arrays]), first_only=np.stack([a[2] for a in arrays]), second_only=np.stack([a[3] for a in arrays]),
               ntriples=np.array([r.n for r in rigs], np.uint32), nfirst=np.array([r.n_first for r in rigs], np.uint32),
               nsecond=np.array([r.n_second for r in rigs], np.uint32))
    lists = dict(ic=(3 * order).astype(np.uint32), i_first=(3 * order + 1).astype(np.uint32), i_second=(3 * order + 2).astype(np.uint32))
    b = lambda *shape: np.full(shape, 0xA5, np.uint8)
    outs = dict(pose_out=b(S, 24 * 8), verdict=b(S, 4), combined=b(S, cap), first_ok=b(S, cap), second_ok=b(S, cap), stats=b(S, 4 * K3.STATS))

    def args(d, l, wait):
        from cv_amd.three_view import ThreeViewInit
        return (d["kps"], cap, 3 * S, l["ic"][0], l["i_first"][0], l["i_second"][0], K3.rig_camera_dev(), d["pose_first"], d["pose_second"], d["triples"],
                d["ntriples"], d["first_only"], d["nfirst"], d["second_only"], d["nsecond"], S,
                ThreeViewInit.params(three_view_patience=64, three_view_filter_loop_iterations=2), d["pose_out"], d["verdict"], d["combined"],
                d["first_ok"], d["second_ok"], d["stats"], wait)

    def check():
        for v in lists.values():
            below(v, 3 * S)
        for k, w in (("triples", "ntriples"), ("first_only", "nfirst"), ("second_only", "nsecond")):
            assert np.all(ins[w] <= cap)
            below(ins[k], cap)

    return Call("rs_three_view_init_batch_device", ins, outs, args, check, lists=lists, scalars=dict(cap=cap, n_blocks=3 * S, n_scenes=S))


def refine_poses(seed):
    import single_view_checker as V
    views = (6, 5) if seed == SEED_TRUE else (5, 6)
    b = V.Batch([V.Rig(900 + 10 * seed + s, 60, n_views=views[s], none=(3,), outliers=(5, 17), noise=0.3) for s in range(2)], 128)
    S = 2
    ins = dict(kps=b.kps, poses=b.poses, obs_start=b.obs_start, obs=b.obs, world=b.world, matches=b.matches, nmatches=b.nmatches, pose=b.pose,
               best_id=b.best_id, inliers=b.inliers, n_inliers=b.n_inliers)
    f = lambda *shape: np.full(shape, 0xA5, np.uint8)
    outs = dict(pose_out=f(S, 96), verdict=f(S, 4), final=f(S, b.cap), n_final=f(S, 4), stats=f(S, 4 * V.STATS))

    def args(d, l, wait):
        from cv_amd.single_view import SingleViewRefiner
        st = V.settings(single_view_optimization_rate=0.02, single_view_patience=120, single_view_filter_loop_iterations=2,
                        single_view_minimum_landmarks=0, single_view_minimum_robust_landmarks=1)
        return (d["kps"], b.cap, b.n_blocks, d["poses"], V.rig_camera_dev(), d["obs_start"], d["obs"], b.n_obs, b.n_landmarks, d["world"], b.n_world,
                l["ik"][0], d["matches"], d["nmatches"], None, d["pose"], d["best_id"], d["inliers"], d["n_inliers"], S,
                SingleViewRefiner.params(**V.settings_dict(st)), d["pose_out"], d["verdict"], d["final"], d["n_final"], d["stats"], wait)

    def check():
        csr_obs(b.obs_start, b.obs, b.n_blocks, b.cap)
        below(b.ik, b.n_blocks)
        assert np.all(b.nmatches <= b.cap) and np.all(b.n_inliers <= b.nmatches)
        below(b.matches[..., 0], b.cap)
        below(b.matches[..., 1], b.n_world)
        below(b.inliers, b.cap)

    return Call("rs_refine_poses_batch_device", ins, outs, args, check, lists=dict(ik=b.ik),
                scalars=dict(cap=b.cap, n_blocks=b.n_blocks, n_obs=b.n_obs, n_landmarks=b.n_landmarks, n_world=b.n_world))


# ---- the consensus (cv_amd/csrc/rs_ransac.hip) and the two-view triangulation (rs_triangulate.hip) -------------------------------
TWO_CAP, TWO_SCENES = 128, 3


def _two_view(seed):
    """TWO_SCENES rigs of three_view_checker: scene s's first camera in keypoint block a[s], its second in b[s] of one pool of
    2 * TWO_SCENES blocks, in an order the seed draws; pair k of a scene is (feature k, feature k), a tenth of them wrong"""
    import three_view_checker as K3
    rng = np.random.default_rng(seed)
    n = 100
    rigs = [K3.Rig(1000 + 10 * seed + s, n, noise=0.5) for s in range(TWO_SCENES)]
    where = rng.permutation(2 * TWO_SCENES)
    ia, ib = where[:TWO_SCENES].astype(np.uint32), where[TWO_SCENES:].astype(np.uint32)
    kps = np.zeros((2 * TWO_SCENES, TWO_CAP), rigs[0].scene_arrays(TWO_CAP)[0].dtype)
    pairs = np.zeros((TWO_SCENES, TWO_CAP, 2), np.uint32)
    for s, r in enumerate(rigs):
        for blk, px in ((ia[s], r.px[0]), (ib[s], r.px[1])):
            kps["x"][blk, :n], kps["y"][blk, :n] = px[:, 0], px[:, 1]
        other = np.arange(n)
        wrong = rng.permutation(n)[:n // 10]
        other[wrong] = other[np.roll(wrong, 1)]
        pairs[s, :n] = np.stack([np.arange(n), other], 1)[rng.permutation(n)]
    return rigs, kps, pairs, np.full(TWO_SCENES, n, np.uint32), ia, ib


def _arrsac(threshold):
    from cv_amd.ransac import EssentialConsensus
    return EssentialConsensus.make_params(threshold, n_hypotheses=256, seed=7, block_size=64, init_blocks=1, max_candidates=64, halve=True)


def _consensus_outs():
    w = lambda *shape: np.full(shape, 0xA5A5A5A5, np.uint32)
    return dict(pose=np.full((TWO_SCENES, 12), -7.0), best_id=w(TWO_SCENES), inliers=w(TWO_SCENES, TWO_CAP), n_inliers=w(TWO_SCENES))


def essential_arrsac(seed):
    import three_view_checker as K3
    _, kps, pairs, npairs, ia, ib = _two_view(seed)
    args = lambda d, l, wait: (d["kps"], d["kps"], TWO_CAP, l["ia"][0], l["ib"][0], d["pairs"], d["npairs"], TWO_SCENES, K3.rig_camera_dev(),
                               K3.rig_camera_dev(), _arrsac(1e-5), 1, d["pose"], d["best_id"], d["inliers"], d["n_inliers"], None, wait)
    check = lambda: (below(ia, 2 * TWO_SCENES), below(ib, 2 * TWO_SCENES), below(pairs, TWO_CAP), below(npairs, TWO_CAP + 1))
    return Call("rs_essential_arrsac_batch_device", dict(kps=kps, pairs=pairs, npairs=npairs), _consensus_outs(), args, check, lists=dict(ia=ia, ib=ib),
                scalars=dict(cap=TWO_CAP, n_scenes=TWO_SCENES))


def triangulate_pairs(seed):
    import three_view_checker as K3
    rigs, kps, pairs, npairs, ia, ib = _two_view(seed)
    rng = np.random.default_rng(seed + 3)
    pose = np.stack([r.first.reshape(12) for r in rigs])
    inliers = np.stack([rng.permutation(100)[:TWO_CAP - 28] for _ in rigs]).astype(np.uint32)
    inliers = np.concatenate([inliers, np.zeros((TWO_SCENES, 28), np.uint32)], 1)
    ins = dict(kps=kps, pairs=pairs, npairs=npairs, pose=pose, best_id=np.zeros(TWO_SCENES, np.uint32), inliers=inliers,
               n_inliers=np.array([90, 1, 77], np.uint32))
    outs = dict(points=np.full((TWO_SCENES, TWO_CAP, 4), -7.0), reason=np.full((TWO_SCENES, TWO_CAP), 0xEE, np.uint8))

    def args(d, l, wait):
        from cv_amd import triangulation
        return (d["kps"], d["kps"], TWO_CAP, l["ia"][0], l["ib"][0], d["pairs"], d["npairs"], TWO_SCENES, K3.rig_camera_dev(), K3.rig_camera_dev(),
                d["pose"], d["best_id"], d["inliers"], d["n_inliers"], triangulation.make_params(), d["points"], d["reason"], wait)

    check = lambda: (below(ia, 2 * TWO_SCENES), below(ib, 2 * TWO_SCENES), below(pairs, TWO_CAP), below(inliers, 100), below(ins["n_inliers"], 101))
    return Call("rs_triangulate_pairs_batch_device", ins, outs, args, check, lists=dict(ia=ia, ib=ib), scalars=dict(cap=TWO_CAP, n_scenes=TWO_SCENES))


def p3p_arrsac(seed):
    import single_view_checker as V
    rng = np.random.default_rng(seed)
    n = 100
    rigs = [V.Rig(1100 + 10 * seed + s, n, noise=0.3, outliers=(5, 17, 40)) for s in range(TWO_SCENES)]
    ik = rng.permutation(TWO_SCENES + 2)[:TWO_SCENES].astype(np.uint32)
    kps = np.zeros((TWO_SCENES + 2, TWO_CAP), V.KP_DTYPE)
    world = np.concatenate([r.world for r in rigs])
    pairs = np.zeros((TWO_SCENES, TWO_CAP, 2), np.uint32)
    for s, r in enumerate(rigs):
        kps["x"][ik[s], :n], kps["y"][ik[s], :n] = r.new_px[:, 0], r.new_px[:, 1]
        pairs[s, :n] = np.stack([np.arange(n), s * n + np.arange(n)], 1)[rng.permutation(n)]
    args = lambda d, l, wait: (d["kps"], TWO_CAP, l["ik"][0], d["pairs"], d["npairs"], TWO_SCENES, d["world"], len(world), V.rig_camera_dev(),
                               _arrsac(1e-5), 1, d["pose"], d["best_id"], d["inliers"], d["n_inliers"], None, wait)
    check = lambda: (below(ik, TWO_SCENES + 2), below(pairs[..., 0], TWO_CAP), below(pairs[..., 1], len(world)))
    return Call("rs_p3p_arrsac_batch_device", dict(kps=kps, pairs=pairs, npairs=np.full(TWO_SCENES, n, np.uint32), world=world), _consensus_outs(), args,
                check, lists=dict(ik=ik), scalars=dict(cap=TWO_CAP, n_scenes=TWO_SCENES, n_world=len(world)))


ROWS = [
    Row("rs_repack_table_device", "rs", repack_table),
    Row("rs_gather_blocks_device", "rs", gather_blocks),
    Row("rs_repack_constraints_device", "rs", repack_constraints),
    Row("hm_place_remap_views_device", "hm", remap_views),
    Row("rs_merge_map_device", "rs", merge_map),
    Row("rs_incorporate_reconstruction_device", "rs", incorporate, host_list=True),
    Row("rs_normalize_reconstruction_device", "rs", normalize, host_list=True),
    Row("rs_export_reconstruction_device", "rs", export, host_list=True),
    Row("rs_join_pairs_batch_device", "rs", join_pairs, host_list=True),
    Row("rs_add_reconstruction_batch_device", "rs", add_reconstruction, host_list=True),
    Row("rs_add_views_device", "rs", add_views, host_list=True),
    Row("rs_landmarks_sharing_view_device", "rs", sharing_view),
    Row("rs_pose_graph_rows_device", "rs", pose_graph_rows),
    Row("rs_pose_graph_edges_device", "rs", pose_graph_edges),
    Row("hm_knn_batch_device", "hm", knn_batch, host_list=True, staged=True),
    Row("hm_match_batch_device", "hm", match_batch, host_list=True, staged=True),
    Row("hm_hash_bag_device", "hm", hash_bag, staged=True),
    Row("hm_best_of_views_batch_device", "hm", best_of_views_batch, host_list=True, staged=True),
    Row("hm_landmark_matches_ordered_batch_device", "hm", landmark_matches_ordered, host_list=True, staged=True),
    Row("hm_landmark_pairs_batch_device", "hm", landmark_pairs, host_list=True, staged=True),
    Row("hm_landmark_matches_batch_device", "hm", landmark_matches, host_list=True, staged=True),
    Row("hm_landmark_original_matches_batch_device", "hm", landmark_original_matches, host_list=True, staged=True),
    Row("hm_knn_views_device", "hm", knn_views, host_list=True, staged=True),
    Row("hm_best_of_views_device", "hm", best_of_views, host_list=True, staged=True),
    Row("hm_find_frames_batch_device", "hm", find_frames),
    Row("akz_extract_batch_device", "akz", extract_batch),
    Row("akz_sample_colors_batch_device", "akz", sample_colors),
    Row("rs_essential_arrsac_batch_device", "rs", essential_arrsac, host_list=True),
    Row("rs_p3p_arrsac_batch_device", "rs", p3p_arrsac, host_list=True),
    Row("rs_triangulate_landmarks_device", "rs", triangulate_landmarks),
    Row("rs_triangulate_merged_device", "rs", triangulate_merged),
    Row("rs_triangulate_pairs_batch_device", "rs", triangulate_pairs, host_list=True),
    Row("rs_refine_poses_batch_device", "rs", refine_poses, host_list=True),
    Row("rs_three_view_init_batch_device", "rs", three_view_init, host_list=True),
    Row("rs_three_view_constraint_batch_device", "rs", three_view_constraint),
    Row("rs_pose_graph_relax_batch_device", "rs", pose_graph_relax),
    Row("rs_filter_observations_device", "rs", filter_observations),
    Row("rs_optimize_reconstruction_batch_device", "rs", optimize_reconstruction),
    Row("rs_covisibility_candidates_device", "rs", covisibility_candidates),
    Row("rs_covisibility_record_device", "rs", covisibility_record),
]
BY_NAME = {r.name: r for r in ROWS}


# ---- the protocol (needs torch and the MI355X) ----------------------------------------------------------------------------------
DELAY_MS = 150.0                         # the producer's delay: the host issues a call in well under a millisecond, a loaded host in a few
HM_STAGE_RING = 4                        # hm_ctx::kStageRing, cv_amd/csrc/hm_match.hip:1253: the slots of the matcher's pinned staging ring


class Context:
    """a fresh context of a family: the handle, the documented sync"""

    def __init__(self, family):
        from cv_amd import _lib
        self.family = family
        if family == "rs":
            from cv_amd.ransac import EssentialConsensus
            self.obj = EssentialConsensus(2048, 256)
            self.obj.reserve(16)
            self.handle, self._sync = self.obj._h, "rs_sync"
        elif family == "hm":
            from cv_amd.knn import Matcher
            self.obj = Matcher(max_descriptors=2048)
            self.handle, self._sync = self.obj._h, "hm_sync"
        elif family == "akz":
            from cv_amd.akaze import Akaze, Context as AkazeContext
            self.obj = AkazeContext(Akaze(detector_threshold=0.01, max_keypoints=AKZ_CAP), AKZ_W, AKZ_H, AKZ_N)
            self.handle, self._sync = self.obj._h, "akz_sync"
        else:
            raise ValueError(family)
        self._lib = _lib

    def sync(self):
        self._lib.check(getattr(self._lib.lib(), self._sync)(self.handle), self._sync)

    def close(self):
        self.obj.close()


def calibrate(torch, want_ms=DELAY_MS):
    """cycles of torch.cuda._sleep that last want_ms, measured once with events -> (cycles, the milliseconds they took)"""
    probe = 20_000_000
    torch.cuda._sleep(1000)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    torch.cuda._sleep(probe)
    b.record()
    b.synchronize()
    cycles = int(probe * want_ms / max(a.elapsed_time(b), 1e-3))
    a.record()
    torch.cuda._sleep(cycles)
    b.record()
    b.synchronize()
    return cycles, a.elapsed_time(b)


def upload(torch, arrays):
    from cv_amd import _lib
    dev = torch.device("cuda", 0)
    return {k: _lib.device_bytes(torch, v, dev) for k, v in arrays.items()}


def host_lists(call):
    from cv_amd import _device
    return {k: _device.index_list(v) for k, v in call.lists.items()}


def buffers(torch, call, ins=None):
    """device buffers of a call: the inputs (of `ins`, default the call's own) and the outputs under their fill; an in-place
    output IS its input buffer"""
    d = upload(torch, call.ins if ins is None else ins)
    d.update(upload(torch, {k: v for k, v in call.outs.items() if k not in call.ins}))
    return d


def read(call, d):
    """the compared buffers as bytes, read without any wait of torch's own"""
    return {k: d[k].cpu().numpy().tobytes()[:call.outs[k].nbytes] for k in call.outs}


def issue(ctx, call, d, lists, wait):
    from cv_amd import _device
    _device.call(call.symbol, ctx.handle, *call.args(d, lists, wait))


def settled(torch, ctx, call):
    """the call on inputs that are complete before it is made -> the compared buffers"""
    from cv_amd import _lib
    d, lists = buffers(torch, call), host_lists(call)
    torch.cuda.synchronize()
    issue(ctx, call, d, lists, _lib.wait_handle(torch.cuda.current_stream(torch.device("cuda", 0))))
    ctx.sync()
    return read(call, d)


def differs(a, b):
    return [k for k in a if a[k] != b[k]]


class Producer:
    """A side stream that is busy for `cycles` and then copies the TRUE inputs over the DECOY ones the buffers hold."""

    def __init__(self, torch, cycles):
        self.torch, self.cycles = torch, cycles
        self.side = torch.cuda.Stream()
        self.done = torch.cuda.Event()

    def start(self, pairs):
        """pairs: [(buffer, true tensor)], both on the device, settled"""
        torch = self.torch
        torch.cuda.synchronize()
        with torch.cuda.stream(self.side):
            torch.cuda._sleep(self.cycles)
            for buf, true in pairs:
                buf.copy_(true, non_blocking=True)
            self.done.record(self.side)

    def wait_handle(self):
        from cv_amd import _lib
        return _lib.wait_handle(self.side)


def overwrite(lists, decoy):
    """the host lists of a call that has returned take the DECOY's words"""
    for k, (words, n) in lists.items():
        a = np.ascontiguousarray(decoy.lists[k], np.uint32)
        assert a.size == n
        C.memmove(words, a.ctypes.data, a.nbytes)


def raced(torch, ctx, calls, cycles):
    """Steps 2 to 6 of the protocol for calls = [(TRUE, DECOY)], made one after the other on one context behind ONE busy
    producer, each with buffers of its own, before any sync -> ([the compared buffers of every call], [returned_early of
    every call])"""
    ds = [buffers(torch, true, ins=decoy.ins) for true, decoy in calls]
    d_trues = [upload(torch, true.ins) for true, _ in calls]
    lists = [host_lists(true) for true, _ in calls]
    p = Producer(torch, cycles)
    p.start([(d[k], d_true[k]) for (true, _), d, d_true in zip(calls, ds, d_trues) for k in true.ins])
    assert not p.done.query(), "the producer finished before the call was made: the test shows nothing"
    early = []
    for (true, decoy), d, l in zip(calls, ds, lists):
        issue(ctx, true, d, l, p.wait_handle())
        overwrite(l, decoy)
        early.append(not p.done.query())
    ctx.sync()
    return [read(true, d) for (true, _), d in zip(calls, ds)], early
