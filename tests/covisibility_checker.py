"""The CPU checker of the covisibility kernels for the tests: tests/cpp/covisibility_host.c (thin wrappers around
include/akz_covisibility_math.h) as host_build.load compiles it, loaded with ctypes; plus the integer-only landmark tables
(starts, observations, reason bytes) the test files use."""
import ctypes as C

import numpy as np

import host_build

OK, FEW_CONSTRAINTS, BAD_INDEX, NO_GRAPH = range(4)
NOT_RECORDED, MAX_CANDIDATE_VIEWS, MAX_SLOTS, MAX_FEATURES, STATS = 16, 128, 256, 8192, 8
S_ROBUST, S_CANDIDATES, S_PAIRS, S_UNIQUE, S_EMITTED, S_FLAGS, S_RECORDED = range(7)
F_CAPPED, F_LIMIT = 1, 2
FILL8, FILL32 = 0xA5, 0xA5A5A5A5


class Settings(C.Structure):
    """akz_cv_settings (include/akz_covisibility_math.h)."""
    _fields_ = [("covisibility_minimum", C.c_uint32), ("maximum_constraints", C.c_uint32), ("minimum_new", C.c_uint32),
                ("minimum_landmarks", C.c_uint32), ("maximum_landmarks", C.c_uint32), ("limit", C.c_uint32), ("seed", C.c_uint32)]


def settings(p):
    """from covisibility_statement.settings' dict"""
    return Settings(p["min_cov"], p["max_constraints"], p["min_new"], p["min_lm"], p["max_lm"], p["limit"], p["seed"])


_lib = None


def lib():
    global _lib
    if _lib is None:
        L = host_build.load("covisibility_host.c")
        vp, u32, sp = C.c_void_p, C.c_uint32, C.POINTER(Settings)
        L.cv_candidates.argtypes = [vp, vp, u32, u32, u32, u32, vp, vp, u32, sp] + [vp] * 6
        L.cv_record.argtypes = [vp, vp, u32, vp, u32, sp, vp, vp, vp]
        L.cv_record.restype = None
        L.cv_rows.argtypes = [vp, u32, u32, vp, vp]
        L.cv_rows.restype = u32
        L.cv_mix.argtypes = [u32, u32]
        L.cv_mix.restype = u32
        L.cv_list_key.argtypes = [u32, u32, u32, u32]
        L.cv_list_key.restype = C.c_uint64
        L.cv_pair_from_index.argtypes = [u32, u32, vp]
        L.cv_pair_from_index.restype = None
        L.cv_record_one.argtypes = [vp, sp, u32, vp, vp]
        _lib = L
    return _lib


def _a(x, dt=np.uint32):
    return np.ascontiguousarray(x, dt)


def outputs(n_targets, p):
    """every output buffer of a candidates call, pre-filled with a pattern"""
    n_slots = n_targets * p["limit"]
    return dict(views=np.full((max(n_slots, 1), 3), FILL32, np.uint32), lm_start=np.full(n_slots + 1, FILL32, np.uint32),
                lm=np.full((max(n_slots * p["max_lm"], 1), 3), FILL32, np.uint32), slot_count=np.full(max(n_slots, 1), FILL32, np.uint32),
                verdict=np.full(max(n_targets, 1), FILL32, np.uint32), stats=np.full((max(n_targets, 1), STATS), FILL32, np.uint32))


def candidates(table, targets, p, n_obs=None):
    """rs_covisibility_candidates_device on the host -> dict of every output array; what the call does not write keeps its fill"""
    start, obs, reason = _a(table["start"]), _a(table["obs"]).reshape(-1, 2), _a(table["reason"], np.uint8)
    targets = _a(targets)
    o = outputs(len(targets), p)
    obs_in = obs if len(obs) else np.zeros((1, 2), np.uint32)
    st = settings(p)
    r = lib().cv_candidates(start.ctypes.data, obs_in.ctypes.data, len(obs) if n_obs is None else n_obs, len(start) - 1, table["cap"],
                            table["n_blocks"], reason.ctypes.data, targets.ctypes.data, len(targets), C.byref(st), o["views"].ctypes.data,
                            o["lm_start"].ctypes.data, o["lm"].ctypes.data, o["slot_count"].ctypes.data, o["verdict"].ctypes.data,
                            o["stats"].ctypes.data)
    assert r == 0
    return o


def record(constraint_verdict, targets, target_verdict, stats, graph_start, p):
    """rs_covisibility_record_device on the host -> (recorded, verdict, stats); the last two are copies updated"""
    cv, targets, gs = _a(constraint_verdict), _a(targets), _a(graph_start)
    verdict, stats = _a(target_verdict).copy(), _a(stats).copy()
    recorded = np.full(max(len(cv), 1), FILL32, np.uint32)
    st = settings(p)
    lib().cv_record(cv.ctypes.data, targets.ctypes.data, len(targets), gs.ctypes.data, len(gs) - 1, C.byref(st), recorded.ctypes.data,
                    verdict.ctypes.data, stats.ctypes.data)
    return recorded, verdict, stats


def rows(views, n_views):
    """rs_pose_graph_rows_device on the host -> (row_start, row_edges [6 n], flag)"""
    views = _a(views).reshape(-1, 3)
    row_start, row_edges = np.full(n_views + 1, FILL32, np.uint32), np.full(max(6 * len(views), 1), FILL32, np.uint32)
    v_in = views if len(views) else np.zeros((1, 3), np.uint32)
    flag = lib().cv_rows(v_in.ctypes.data, len(views), n_views, row_start.ctypes.data, row_edges.ctypes.data)
    return row_start, row_edges[:6 * len(views)], flag


def equals_statement(o, s, p):
    """every word of the host build's (or the device's) outputs `o` against the statement's result `s`"""
    n_slots = len(s["views"])
    assert np.array_equal(o["views"][:n_slots], np.array(s["views"], np.uint32).reshape(-1, 3))
    assert o["lm_start"].tolist() == s["lm_start"]
    n = len(s["lm"])
    assert np.array_equal(o["lm"][:n], np.array(s["lm"], np.uint32).reshape(-1, 3))
    assert not o["lm"][n:n_slots * p["max_lm"]].any()
    assert o["slot_count"][:n_slots].tolist() == s["slot_count"]
    assert o["verdict"][:len(s["verdict"])].tolist() == s["verdict"]
    assert o["stats"][:len(s["stats"])].tolist() == s["stats"]


# ---- tables ---------------------------------------------------------------------------------------------------------
def make_table(lists, n_blocks, cap, reason=None):
    """lists: per landmark a list of (block, feature) -> dict(start, obs, reason, n_blocks, cap)"""
    start = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint32)
    obs = np.array([o for x in lists for o in x], np.uint32).reshape(-1, 2)
    reason = np.zeros(len(lists), np.uint8) if reason is None else np.asarray(reason, np.uint8)
    return dict(start=start, obs=obs, reason=reason, n_blocks=n_blocks, cap=cap)


def random_table(seed, n_views=12, n_landmarks=300, lengths=(3, 8), not_robust=0.1, cap=None, scatter=True):
    """n_landmarks landmarks, each observed by lengths[0] .. lengths[1] distinct views chosen at random; a view's features are
    dealt in landmark order, at scattered positions of its block when `scatter`; a fraction `not_robust` of the reason bytes is
    not RS_TRI_OK (1 .. 5)."""
    rng = np.random.default_rng(seed)
    per_view = [[] for _ in range(n_views)]
    members = []
    for l in range(n_landmarks):
        n = int(rng.integers(lengths[0], min(lengths[1], n_views) + 1))
        vs = rng.permutation(n_views)[:n]
        members.append(vs)
        for v in vs:
            per_view[v].append(l)
    need = max(len(x) for x in per_view)
    cap = cap or need + 7
    assert cap >= need
    place = [rng.permutation(cap)[:len(x)] if scatter else np.arange(len(x)) for x in per_view]
    where = [dict(zip(x, pl.tolist())) for x, pl in zip(per_view, place)]
    lists = [[(int(v), where[v][l]) for v in members[l]] for l in range(n_landmarks)]
    reason = np.where(rng.random(n_landmarks) < not_robust, rng.integers(1, 6, n_landmarks), 0)
    return make_table(lists, n_views, cap, reason)


def star_table(n_coviews, per_coview, robust_features, cap, target=0, extra_blocks=0):
    """A table made to measure for target `target`: robust_features landmarks on its features 0 .. robust_features - 1; coview k
    (blocks 1 .. n_coviews, the target skipped) observes the first per_coview[k] of them (per_coview an int or a list)."""
    per = [per_coview] * n_coviews if np.isscalar(per_coview) else list(per_coview)
    n_blocks = n_coviews + 1 + extra_blocks
    blocks = [b for b in range(n_blocks) if b != target][:n_coviews]
    lists = []
    for k in range(robust_features):
        row = [(target, k)]
        for c, b in enumerate(blocks):
            if k < per[c]:
                row.append((b, k % cap))
        lists.append(row)
    return make_table(lists, n_blocks, cap)
