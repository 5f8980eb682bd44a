"""The CPU checker of the pose-graph kernels for the tests: tests/cpp/pose_graph_host.c (thin wrappers around
include/akz_pose_graph_math.h) as host_build.load compiles it — the host compiler, no contraction to FMA, as the kernels —
loaded with ctypes; plus the synthetic graphs the test files use."""
import ctypes as C

import numpy as np

import host_build
import pose_graph_statement as S

STATS = 8
S_VIEWS, S_UPDATED, S_EDGES, S_ROUNDS, S_STAGE, S_FIRST_BAD_VIEW = range(6)
OK, FEW_VIEWS, NONFINITE, BAD_INDEX = range(4)
VIEW_UPDATED, VIEW_NO_CONSTRAINT, VIEW_NONFINITE = range(3)
NO_VIEW = 0xFFFFFFFF
TVC_OK, TVC_FEW_LANDMARKS = 0, 1
FILL32 = 0xA5A5A5A5
SLOT_TARGET, SLOT_OTHER = (0, 0, 1, 1, 2, 2), (2, 1, 0, 2, 1, 0)


class Settings(C.Structure):
    """akz_pg_settings (include/akz_pose_graph_math.h)."""
    _fields_ = [("graph_optimization_rate", C.c_double), ("optimization_iterations", C.c_uint)]


def settings(iterations=1024, rate=1e-3):
    """The reference's defaults (cv-sfm/src/settings.rs:461-463, 477-479) unless told otherwise."""
    return Settings(rate, iterations)


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    L = host_build.load("pose_graph_host.c")
    vp, u32, dbl = C.c_void_p, C.c_uint32, C.c_double
    L.pg_acos.argtypes = [dbl]
    L.pg_acos.restype = dbl
    L.pg_acos_many.argtypes = [vp, u32, vp]
    for name in ("pg_log", "pg_exp", "pg_se3"):
        getattr(L, name).argtypes = [vp, vp]
        getattr(L, name).restype = None
    L.pg_edge_se3.argtypes = [vp, vp, vp, vp]
    L.pg_from_se3_mul.argtypes = [vp, vp, vp]
    L.pg_view_update.argtypes = [vp, dbl, vp, vp]
    L.pg_apply_delta.argtypes = [vp, vp]
    L.pg_slot_target.argtypes = L.pg_slot_other.argtypes = [u32]
    L.pg_slot_target.restype = L.pg_slot_other.restype = u32
    L.pg_edges.argtypes = [vp, vp, u32, vp]
    L.pg_sum.argtypes = [vp, u32, vp, u32, vp, vp, vp, C.c_int, vp]
    L.pg_relax_batch.argtypes = [vp, u32, vp, u32, vp, vp, u32, vp, vp, vp, u32, C.POINTER(Settings), C.c_int, vp, vp, vp]
    _lib = L
    return L


def _a(x, dt=np.float64):
    return np.ascontiguousarray(x, dt)


def acos(c):
    c = _a(c).reshape(-1)
    out = np.empty_like(c)
    lib().pg_acos_many(c.ctypes.data, len(c), out.ctypes.data)
    return out


def log(pose):
    p, w = _a(pose).reshape(12), np.empty(3)
    lib().pg_log(p.ctypes.data, w.ctypes.data)
    return w


def exp(w):
    w, r = _a(w).reshape(3), np.empty(9)
    lib().pg_exp(w.ctypes.data, r.ctypes.data)
    return r.reshape(3, 3)


def se3(delta):
    p, out = _a(delta).reshape(12), np.empty(6)
    lib().pg_se3(p.ctypes.data, out.ctypes.data)
    return out


def from_se3_mul(net, pose):
    n, p, out = _a(net).reshape(6), _a(pose).reshape(12), np.empty(12)
    lib().pg_from_se3_mul(n.ctypes.data, p.ctypes.data, out.ctypes.data)
    return out.reshape(3, 4)


def apply_delta(delta, pose):
    """akz_tv_apply_delta of akz_three_view_math.h (Se3TangentSpace::isometry): what from_se3 must NOT be"""
    d, p = _a(delta).reshape(6), _a(pose).reshape(12).copy()
    lib().pg_apply_delta(d.ctypes.data, p.ctypes.data)
    return p.reshape(3, 4)


def view_update(sum6, rate, pose):
    s, p, out = _a(sum6).reshape(6), _a(pose).reshape(12), np.empty(12)
    ok = lib().pg_view_update(s.ctypes.data, rate, p.ctypes.data, out.ctypes.data)
    return ok, out.reshape(3, 4)


def edges(cposes, cverdict):
    """rs_pose_graph_edges_device on the host: [n][6][12]"""
    p, v = _a(cposes).reshape(-1, 24), _a(cverdict, np.uint32)
    out = np.empty((len(v), 6, 12))
    lib().pg_edges(p.ctypes.data, v.ctypes.data, len(v), out.ctypes.data)
    return out


def view_sum(A, v, sequential=False, poses=None):
    """the sum of view v's row over the batch arrays A"""
    poses = _a(A["poses"] if poses is None else poses).reshape(-1, 12)
    row = _a(A["row_edges"][A["row_start"][v]:A["row_start"][v + 1]], np.uint32)
    out = np.empty(6)
    lib().pg_sum(poses.ctypes.data, v, row.ctypes.data, len(row), A["views"].ctypes.data, A["cverdict"].ctypes.data, A["edges"].ctypes.data,
                 int(sequential), out.ctypes.data)
    return out


def relax(A, st, sequential=False, n_rows=None, n_constraints=None):
    """rs_pose_graph_relax_batch_device on the host arrays of `batch` -> dict(poses, verdict, state, stats); what the call does
    not write keeps FILL32"""
    poses = _a(A["poses"]).reshape(-1, 12).copy()
    n_graphs = len(A["graph_start"]) - 1
    verdict = np.full(n_graphs, FILL32, np.uint32)
    state = np.full(len(poses), FILL32, np.uint32)
    stats = np.full((n_graphs, STATS), FILL32, np.uint32)
    row_edges = A["row_edges"] if len(A["row_edges"]) else np.zeros(1, np.uint32)
    r = lib().pg_relax_batch(poses.ctypes.data, len(poses), A["graph_start"].ctypes.data, n_graphs, A["row_start"].ctypes.data,
                             row_edges.ctypes.data, len(A["row_edges"]) if n_rows is None else n_rows, A["views"].ctypes.data,
                             A["cverdict"].ctypes.data, A["edges"].ctypes.data, len(A["views"]) if n_constraints is None else n_constraints,
                             C.byref(st), int(sequential), verdict.ctypes.data, state.ctypes.data, stats.ctypes.data)
    assert r == 0
    return dict(poses=poses, verdict=verdict, state=state, stats=stats)


# ---- synthetic graphs ----
def rodrigues(w):
    return S.exp(w)


def pose_of(t, w):
    return np.hstack([rodrigues(np.asarray(w, np.float64)), np.asarray(t, np.float64).reshape(3, 1)])


class Graph:
    """n views whose ground-truth WorldToCamera poses stand on a ring (or, `grid`, on a square grid) looking inwards, the
    constraints `triples` (default: every three neighbours (i, i + 1, i + 2) around the ring) with the exact relative poses
    first = w1 w0^-1, second = w2 w0^-1, and initial poses that are the truth moved by a seeded se(3) noise of size `noise`.
    `refused`: constraints whose verdict is RS_TVC_FEW_LANDMARKS (their poses are garbage nobody may read).  `rows`: view ->
    list of the graph's own edge ids 6 * constraint + slot, replacing the flattened row of that view."""

    def __init__(self, seed, n, triples=None, noise=1e-2, grid=False, refused=(), rows=None):
        rng = np.random.default_rng(seed)
        self.n = n
        truth = []
        side = int(np.ceil(np.sqrt(n)))
        for i in range(n):
            if grid:
                centre = np.array([i % side, i // side, 0.0]) * 1.5
                w = 0.05 * rng.standard_normal(3)
            else:
                a = 2.0 * np.pi * i / max(n, 3)
                centre = np.array([4.0 * np.cos(a), 0.3 * np.sin(3 * a), 4.0 * np.sin(a)])
                w = np.array([0.0, -a + np.pi / 2, 0.0]) + 0.05 * rng.standard_normal(3)
            r = rodrigues(w)
            truth.append(np.hstack([r, (-r @ centre).reshape(3, 1)]))
        self.truth = np.stack(truth) if n else np.zeros((0, 3, 4))
        self.poses = np.stack([S.mul(S.from_se3(noise * rng.standard_normal(6)), p) for p in truth]) if n else np.zeros((0, 3, 4))
        if triples is None:
            triples = [(i, (i + 1) % n, (i + 2) % n) for i in range(n)] if n >= 3 else []
        self.views = np.array(triples, np.uint32).reshape(-1, 3)
        self.cposes = np.zeros((len(self.views), 2, 3, 4))
        self.cverdict = np.zeros(len(self.views), np.uint32)
        for c, (v0, v1, v2) in enumerate(self.views):
            self.cposes[c, 0] = S.mul(self.truth[v1], S.inverse(self.truth[v0]))
            self.cposes[c, 1] = S.mul(self.truth[v2], S.inverse(self.truth[v0]))
        for c in refused:
            self.cverdict[c] = TVC_FEW_LANDMARKS
            self.cposes[c] = np.nan
        self.rows = flatten(self.views, n)
        for v, row in (rows or {}).items():
            self.rows[v] = list(row)

    def statement_graph(self):
        """the dict flatten_constraints builds from the accepted constraints (rows as flattened, no replacement)"""
        return S.flatten([(self.views[c], self.cposes[c, 0], self.cposes[c, 1]) for c in range(len(self.views)) if self.cverdict[c] == TVC_OK])


def flatten(views, n_views):
    """rows[v]: the edge ids whose target is v, constraint ascending, slot order within a constraint"""
    rows = [[] for _ in range(n_views)]
    for c, tri in enumerate(np.asarray(views).reshape(-1, 3)):
        for slot in range(6):
            rows[int(tri[SLOT_TARGET[slot]])].append(6 * c + slot)
    return rows


def batch(graphs):
    """The device call's inputs for a list of graphs, graph g owning consecutive views and constraints: dict of poses
    [n_views][12], graph_start, row_start, row_edges, views [n_c][3], cposes [n_c][24], cverdict, edges [n_c][6][12] (the
    host build's)."""
    poses, views, cposes, cverdict, row_edges = [], [], [], [], []
    graph_start, row_start = [0], [0]
    v0 = c0 = 0
    for gr in graphs:
        poses.append(gr.poses.reshape(-1, 12))
        views.append(gr.views + np.uint32(v0))
        cposes.append(gr.cposes.reshape(-1, 24))
        cverdict.append(gr.cverdict)
        for row in gr.rows:
            row_edges += [e + 6 * c0 for e in row]
            row_start.append(len(row_edges))
        v0 += gr.n
        c0 += len(gr.views)
        graph_start.append(v0)
    A = dict(poses=np.concatenate(poses + [np.zeros((0, 12))]), graph_start=np.array(graph_start, np.uint32),
             row_start=np.array(row_start, np.uint32), row_edges=np.array(row_edges, np.uint32),
             views=np.concatenate(views + [np.zeros((0, 3), np.uint32)]).astype(np.uint32),
             cposes=np.concatenate(cposes + [np.zeros((0, 24))]), cverdict=np.concatenate(cverdict + [np.zeros(0, np.uint32)]).astype(np.uint32))
    if len(A["views"]) == 0:       # a call without constraints still hands over arrays
        A["views"], A["cposes"], A["cverdict"] = np.zeros((1, 3), np.uint32), np.zeros((1, 24)), np.full(1, TVC_FEW_LANDMARKS, np.uint32)
    A["edges"] = edges(A["cposes"], A["cverdict"])
    return A


def residual(poses, A, g=0):
    """the largest |se3(expected * w_other * w_view^-1)| over the accepted edges of graph g's rows, by the host build"""
    poses = _a(poses).reshape(-1, 12)
    worst = 0.0
    out = np.empty(6)
    for v in range(int(A["graph_start"][g]), int(A["graph_start"][g + 1])):
        inv = S.inverse(poses[v].reshape(3, 4)).reshape(12).copy()
        for e in A["row_edges"][A["row_start"][v]:A["row_start"][v + 1]]:
            c, slot = divmod(int(e), 6)
            if A["cverdict"][c] != TVC_OK:
                continue
            o = int(A["views"][c, SLOT_OTHER[slot]])
            lib().pg_edge_se3(A["edges"][c, slot].ctypes.data, poses[o].ctypes.data, inv.ctypes.data, out.ctypes.data)
            worst = max(worst, float(np.linalg.norm(out)))
    return worst
