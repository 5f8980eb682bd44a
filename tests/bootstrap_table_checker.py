"""The CPU checker of the kernels that start a reconstruction, for the tests: tests/cpp/bootstrap_table_host.c (the host's
execution in include/akz_bootstrap_table_math.h) as host_build.load compiles it, loaded with ctypes; plus the one description of
a call (`join_inputs`, `add_inputs`) that the checker, the device and the statement (tests/bootstrap_table_statement.py) all
take, and the fills both sides start from."""
import ctypes as C

import numpy as np

import host_build

JP_OK, JP_NO_MODEL, JP_FEW_INLIERS, JP_BAD_INDEX = range(4)
AR_OK, AR_NOT_ACCEPTED, AR_BAD_INDEX, AR_TAKEN, AR_BAD_TABLE = range(5)
STATS, COUNTS = 4, 4
NONE = 0xFFFFFFFF
FILL8, FILL32, FILL64 = 0xA5, 0xA5A5A5A5, -7.25
TV_OK, TV_FEW_ROBUST = 0, 5
KP_BYTES = 28
TILE = 1024

_lib = None


def lib():
    global _lib
    if _lib is None:
        L = host_build.load("bootstrap_table_host.c")
        vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
        L.bt_join.argtypes = [vp] * 6 + [u32, vp, vp, u32, u32, u32, u64] + [vp] * 9
        L.bt_join.restype = None
        L.bt_add.argtypes = [vp] * 14 + [u32, vp, vp, u32, u32, u32, vp, vp, vp, u32, u32, vp, vp, u32, vp, vp, vp, u32, u32, u32, u32] + [vp] * 13
        L.bt_add.restype = None
        L.bt_shuffle_key.argtypes = [u64, u32, u32]
        L.bt_shuffle_key.restype = u32
        L.bt_stable_order.argtypes = [vp, u32, vp]
        L.bt_stable_order.restype = None
        L.bt_row_length.argtypes = [u32, u32]
        L.bt_row_length.restype = u32
        _lib = L
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data


# ---- the join ----
def slot(pairs, inliers=None, best_id=0, npairs=None, n_inliers=None, pose=None):
    """One slot of a consensus call: the matcher's pair list [(centre, other)], the inlier indices into it (default: all, in
    order), the consensus' id and pose."""
    pairs = [tuple(p) for p in pairs]
    inliers = list(range(len(pairs))) if inliers is None else list(inliers)
    return dict(pairs=pairs, inliers=inliers, best_id=best_id, npairs=len(pairs) if npairs is None else npairs,
                n_inliers=len(inliers) if n_inliers is None else n_inliers, pose=pose)


def join_inputs(slots, scenes, cap, minimum=0, shuffle=False, seed=0):
    """Every array of an rs_join_pairs_batch_device call, contiguous, as a dict.  scenes: [(slot_first, slot_second)]."""
    n = max(len(slots), 1)
    pairs, inliers = np.full((n, cap, 2), FILL32, np.uint32), np.full((n, cap), FILL32, np.uint32)
    npairs, n_inliers, best_id, pose = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros((n, 12))
    for k, s in enumerate(slots):
        p, i = np.array(s["pairs"], np.uint32).reshape(-1, 2)[:cap], np.array(s["inliers"], np.uint32)[:cap]
        pairs[k, :len(p)], inliers[k, :len(i)] = p, i
        npairs[k], n_inliers[k], best_id[k] = s["npairs"], s["n_inliers"], s["best_id"]
        pose[k] = np.arange(12) / 8.0 + 10 * k + 1 if s["pose"] is None else np.asarray(s["pose"], np.float64).reshape(12)
    return dict(pairs=pairs, npairs=npairs, inliers=inliers, n_inliers=n_inliers, best_id=best_id, pose=pose, n_slots=len(slots), cap=cap,
                slot_first=np.array([a for a, _ in scenes], np.uint32), slot_second=np.array([b for _, b in scenes], np.uint32),
                n_scenes=len(scenes), minimum=minimum, flags=1 if shuffle else 0, seed=seed)


def join_outputs(inp):
    """The output buffers of a join under their fill — what neither side writes stays FILL32."""
    n, cap = max(inp["n_scenes"], 1), inp["cap"]
    w = lambda *shape: np.full(shape, FILL32, np.uint32)
    return dict(triples=w(n, cap, 3), ntriples=w(n), first_only=w(n, cap, 2), nfirst=w(n), second_only=w(n, cap, 2), nsecond=w(n),
                pose_first=np.full((n, 12), FILL64), pose_second=np.full((n, 12), FILL64), verdict=w(n))


JOIN_OUTPUT_NAMES = ("triples", "ntriples", "first_only", "nfirst", "second_only", "nsecond", "pose_first", "pose_second", "verdict")


def join(inp):
    """rs_join_pairs_batch_device on the host -> dict of every output buffer."""
    o = join_outputs(inp)
    lib().bt_join(_p(inp["pairs"]), _p(inp["npairs"]), _p(inp["inliers"]), _p(inp["n_inliers"]), _p(inp["best_id"]), _p(inp["pose"]), inp["cap"],
                  _p(inp["slot_first"]), _p(inp["slot_second"]), inp["n_scenes"], inp["minimum"], inp["flags"], inp["seed"],
                  *(_p(o[k]) for k in JOIN_OUTPUT_NAMES))
    return o


# ---- add_reconstruction ----
def scene(blocks, counts, triples=(), combined=None, first_only=(), first_ok=None, second_only=(), second_ok=None, verdict=TV_OK, skip=0,
          pose=None, ntriples=None, nfirst=None, nsecond=None):
    """One scene of a bootstrap call: its source blocks (centre, first, second) with their feature counts, the three lists with
    their masks (default: all set), the bootstrap's verdict and poses."""
    lists = [[tuple(m) for m in l] for l in (triples, first_only, second_only)]
    masks = [[1] * len(l) if m is None else list(m) for l, m in zip(lists, (combined, first_ok, second_ok))]
    return dict(blocks=tuple(blocks), counts=tuple(counts), lists=lists, masks=masks, verdict=verdict, skip=skip, pose=pose,
                n=[len(l) if n is None else n for l, n in zip(lists, (ntriples, nfirst, nsecond))])


def add_inputs(scenes, cap, n_src_blocks, n_blocks, view_base, table=None, recon_start=None, view_start=None, counts=None, use_skip=None,
               extra_room=0, obs_room=None, lm_room=None, seed=7):
    """Every array of an rs_add_reconstruction_batch_device call, contiguous, as a dict.  table: (obs_start, obs [n_obs][2],
    n_obs) as landmark_table_checker.table gives it, or None."""
    n, m = len(scenes), max(len(scenes), 1)
    w = lambda *shape: np.full(shape, FILL32, np.uint32)
    rng = np.random.default_rng(seed)
    kps = rng.integers(0, 256, (n_src_blocks, cap, KP_BYTES), dtype=np.uint8)
    cnt = np.zeros(n_src_blocks, np.uint32) if counts is None else np.ascontiguousarray(counts, np.uint32).copy()
    arrays = [w(m, cap, 3), w(m, cap, 2), w(m, cap, 2)]
    masks = [np.full((m, cap), FILL8, np.uint8) for _ in range(3)]
    ns = np.zeros((3, m), np.uint32)
    verdict, skip, pose_out = np.zeros(m, np.uint32), np.zeros(m, np.uint32), np.zeros((m, 24))
    frames = np.zeros((3, m), np.uint32)
    for s, sc in enumerate(scenes):
        frames[:, s] = sc["blocks"]
        if counts is None:
            for b, c in zip(sc["blocks"], sc["counts"]):
                cnt[b] = c
        for k in range(3):
            rows = np.array(sc["lists"][k], np.uint32).reshape(-1, 3 if k == 0 else 2)[:cap]
            arrays[k][s, :len(rows)] = rows
            masks[k][s, :len(rows)] = np.array(sc["masks"][k], np.uint8)[:cap]
            ns[k, s] = sc["n"][k]
        verdict[s], skip[s] = sc["verdict"], sc["skip"]
        pose_out[s] = np.arange(24) / 32.0 + s + 1 if sc["pose"] is None else np.asarray(sc["pose"], np.float64).reshape(24)
    if use_skip is None:
        use_skip = bool(skip.any())
    if table is None:
        obs_start, obs, n_obs, n_lm = None, None, 0, 0
    else:
        obs_start, obs, n_obs = np.ascontiguousarray(table[0], np.uint32), np.ascontiguousarray(table[1], np.uint32).reshape(-1, 2), table[2]
        n_lm = len(obs_start) - 1
    n_recons = 0 if recon_start is None else len(recon_start) - 1
    grow = 3 * n * cap
    return dict(triples=arrays[0], ntriples=ns[0].copy(), first_only=arrays[1], nfirst=ns[1].copy(), second_only=arrays[2], nsecond=ns[2].copy(),
                combined=masks[0], first_ok=masks[1], second_ok=masks[2], pose_out=pose_out, tv_verdict=verdict, ic=frames[0].copy(),
                i_first=frames[1].copy(), i_second=frames[2].copy(), n_scenes=n, kps=kps, counts=cnt, n_src_blocks=n_src_blocks, cap=cap,
                skip=skip if use_skip else None, obs_start=obs_start, obs=obs, n_obs=n_obs, n_landmarks=n_lm,
                recon_start=None if recon_start is None else np.array(recon_start, np.uint32),
                view_start=None if view_start is None else np.array(view_start, np.uint32), n_recons=n_recons, n_blocks=n_blocks,
                view_base=view_base, obs_room=n_obs + grow + extra_room if obs_room is None else obs_room,
                lm_room=n_lm + grow + extra_room if lm_room is None else lm_room)


ADD_OUTPUT_NAMES = ("kps_dst", "counts_dst", "poses", "obs_start_out", "obs_out", "obs_counts_out", "counts_out", "landmarks_out", "recon_start_out",
                    "view_start_out", "views_out", "constraint_poses_out", "constraint_verdict_out", "frame_verdict", "stats", "call_verdict")


def add_outputs(inp):
    """The output buffers of a call under their fill — what neither side writes stays as it is."""
    m, cap, nb = max(inp["n_scenes"], 1), inp["cap"], inp["n_blocks"]
    w = lambda *shape: np.full(shape, FILL32, np.uint32)
    ranges = inp["n_recons"] + inp["n_scenes"] + 1
    return dict(kps_dst=np.full((nb, cap, KP_BYTES), FILL8, np.uint8), counts_dst=w(nb), poses=np.full((nb, 12), FILL64),
                obs_start_out=w(inp["lm_room"] + 1), obs_out=w(max(inp["obs_room"], 1), 2), obs_counts_out=w(max(inp["lm_room"], 1)),
                counts_out=w(COUNTS), landmarks_out=w(nb, cap), recon_start_out=w(ranges), view_start_out=w(ranges), views_out=w(m, 3),
                constraint_poses_out=np.full((m, 24), FILL64), constraint_verdict_out=w(m), frame_verdict=w(m), stats=w(m, STATS),
                call_verdict=w(1))


def add(inp):
    """rs_add_reconstruction_batch_device on the host -> dict of every output buffer."""
    o = add_outputs(inp)
    i = inp
    lib().bt_add(_p(i["triples"]), _p(i["ntriples"]), _p(i["first_only"]), _p(i["nfirst"]), _p(i["second_only"]), _p(i["nsecond"]), _p(i["combined"]),
                 _p(i["first_ok"]), _p(i["second_ok"]), _p(i["pose_out"]), _p(i["tv_verdict"]), _p(i["ic"]), _p(i["i_first"]), _p(i["i_second"]),
                 i["n_scenes"], _p(i["kps"]), _p(i["counts"]), i["n_src_blocks"], i["cap"], KP_BYTES, _p(i["skip"]), _p(i["obs_start"]), _p(i["obs"]),
                 i["n_obs"], i["n_landmarks"], _p(i["recon_start"]), _p(i["view_start"]), i["n_recons"], _p(o["kps_dst"]), _p(o["counts_dst"]),
                 _p(o["poses"]), i["n_blocks"], i["view_base"], i["obs_room"], i["lm_room"], *(_p(o[k]) for k in ADD_OUTPUT_NAMES[3:]))
    return o


# ---- designed and drawn inputs, shared by the CPU and the GPU tests ----
def drawn_slot(rng, cap, n_pairs, n_inliers, centres=None, **kw):
    """A slot with n_pairs pairs whose centre features are drawn from `centres` features (fewer than n_pairs: some occur twice)
    and n_inliers of them, ascending, as inliers."""
    centres = cap if centres is None else centres
    centre = rng.integers(0, centres, n_pairs) if centres < n_pairs else rng.permutation(centres)[:n_pairs]
    pairs = list(zip(centre.tolist(), rng.integers(0, cap, n_pairs).tolist()))
    return slot(pairs, sorted(rng.permutation(n_pairs)[:n_inliers].tolist()), **kw)


def drawn_scene(rng, blocks, counts, cap, lists, keep=0.8, **kw):
    """A valid scene: lists = (ntriples, nfirst, nsecond) matches over distinct features of each view, a share `keep` of them
    accepted by their masks."""
    (cc, cf, cs), (nt, nf, ns) = counts, lists
    assert nt + nf + ns <= cc and nt + nf <= cf and nt + ns <= cs and max(nt, nf, ns) <= cap
    c, f, g = rng.permutation(cc)[:nt + nf + ns].tolist(), rng.permutation(cf)[:nt + nf].tolist(), rng.permutation(cs)[:nt + ns].tolist()
    mask = lambda n: (rng.random(n) < keep).astype(np.uint8).tolist()
    return scene(blocks, counts, list(zip(c[:nt], f[:nt], g[:nt])), mask(nt), list(zip(c[nt:nt + nf], f[nt:])), mask(nf),
                 list(zip(c[nt + nf:], g[nt:])), mask(ns), **kw)


def same(a, b, names):
    """the names of the buffers in which two output dicts differ (byte for byte)"""
    return [k for k in names if a[k].tobytes() != b[k].tobytes()]
