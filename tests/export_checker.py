"""The CPU checker of the export kernels for the tests: tests/cpp/export_host.c (the host's execution of
include/akz_export_math.h) as host_build.load compiles it, loaded with ctypes; plus the one description of a call (`inputs`)
that the checker, the device and the statement (tests/export_statement.py) all take, the designed cases and the seeded random
ones."""
import ctypes as C

import numpy as np

import host_build
from landmark_table_checker import FILL8, FILL32, NONE, table
from reconstruction_merge_checker import FILL64, random_pose

OK, OVERFLOW, BAD_TABLE = range(3)
COUNTS, CAMERA_WORDS, CAMERA_VERTICES = 4, 10, 5
NO_POINT = (0.0, 0.0, 0.0, -1.0)                          # akz_tri_none

_lib = None


def lib():
    global _lib
    if _lib is None:
        L = host_build.load("export_host.c")
        vp, u32 = C.c_void_p, C.c_uint32
        L.ex_export.argtypes = [vp, u32, vp, vp, u32, u32, vp, vp, u32, vp, vp, u32, u32, vp, u32, vp, vp, vp, vp, vp, vp]
        L.ex_export.restype = None
        L.ex_camera.argtypes = [vp, C.c_double, vp]
        L.ex_camera.restype = None
        L.ex_camera_vertex.argtypes = [vp, C.c_int, vp]
        L.ex_camera_vertex.restype = None
        _lib = L
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data


def inputs(world, rows, view_blocks, counts, landmarks, poses, cap, room=None, seed=0, pad=2, start=None, start_obs=None):
    """Every array of an rs_export_reconstruction_device call, contiguous, as a dict.  world [n_world][4]; rows: per-landmark
    lists of (block, feature) (or start / start_obs: ready CSR arrays, for the tables no list describes); landmarks
    [n_blocks][cap]; the colour table is seeded noise, so that two features rarely share a colour."""
    world = np.ascontiguousarray(world, np.float64).reshape(-1, 4)
    n_world = len(world)
    if start is None:
        s, obs, n_obs = table(rows, pad=pad)
    else:
        s, obs = np.ascontiguousarray(start, np.uint32), np.ascontiguousarray(start_obs, np.uint32).reshape(-1, 2)
        n_obs = len(obs)
        obs = obs if n_obs else np.full((1, 2), FILL32, np.uint32)
    poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 12)
    n_blocks = len(poses)
    colors = np.random.default_rng(seed + 77).integers(0, 256, (n_blocks, cap, 3)).astype(np.uint8)
    return dict(world=world if n_world else np.zeros((1, 4)), n_world=n_world, start=s, obs=obs, n_obs=n_obs, n_landmarks=len(s) - 1, colors=colors,
                view_blocks=np.array(view_blocks, np.uint32), counts=np.ascontiguousarray(counts, np.uint32),
                landmarks=np.ascontiguousarray(landmarks, np.uint32).reshape(n_blocks, cap), cap=cap, n_blocks=n_blocks, poses=poses,
                room=n_world if room is None else room, rows=rows)


OUTPUTS = ("xyz", "rgb", "key", "cameras", "counts_out", "verdict")


def outputs(inp):
    """The output buffers of a call under their fill — what neither side writes stays the fill."""
    n = CAMERA_VERTICES * len(inp["view_blocks"]) + inp["room"]
    return dict(xyz=np.full((n, 3), FILL64), rgb=np.full((n, 3), FILL8, np.uint8), key=np.full(max(inp["room"], 1), FILL32, np.uint32),
                cameras=np.full((len(inp["view_blocks"]), CAMERA_WORDS), FILL64), counts_out=np.full(COUNTS, FILL32, np.uint32),
                verdict=np.full(1, FILL32, np.uint32))


def export(inp):
    """rs_export_reconstruction_device on the host -> dict of every output buffer."""
    o = outputs(inp)
    lib().ex_export(_p(inp["world"]), inp["n_world"], _p(inp["start"]), _p(inp["obs"]), inp["n_obs"], inp["n_landmarks"], _p(inp["colors"]),
                    _p(inp["view_blocks"]), len(inp["view_blocks"]), _p(inp["counts"]), _p(inp["landmarks"]), inp["cap"], inp["n_blocks"],
                    _p(inp["poses"]), inp["room"], *[_p(o[k]) for k in OUTPUTS])
    return o


def is_fill(a):
    want = {8: FILL64, 4: FILL32, 1: FILL8}[a.dtype.itemsize]
    return bool(np.all(a.view(np.uint8) == np.full(1, want, a.dtype).view(np.uint8)[0]))


def check_against_statement(inp, o, bound):
    """Every output buffer `o` of a call on a clean table against the statement's result for the same inputs -> (the result, the
    largest absolute difference of a coordinate, a camera word or a frustum vertex).  Which landmarks are exported, their
    order, keys, colours, counters and the verdict exactly; the floats under `bound`."""
    import export_statement as S
    st = S.export(inp["world"][:inp["n_world"]], inp["rows"], inp["colors"], [int(b) for b in inp["view_blocks"]], inp["counts"], inp["landmarks"],
                  inp["poses"], inp["cap"], inp["n_blocks"], inp["room"])
    assert int(o["verdict"][0]) == st["verdict"]
    assert [int(v) for v in o["counts_out"]] == st["counts"]
    n = len(st["keys"])
    first = CAMERA_VERTICES * len(inp["view_blocks"])
    assert n == min(st["counts"][0], inp["room"])
    assert [int(k) for k in o["key"][:n]] == st["keys"]
    assert [tuple(int(c) for c in row) for row in o["rgb"][:first + n]] == st["colors"]
    assert is_fill(o["key"][n:]) and is_fill(o["rgb"][first + n:]) and is_fill(o["xyz"][first + n:])      # nothing lands behind the points
    diff = float(np.max(np.abs(o["xyz"][:first + n] - st["vertices"]), initial=0.0))
    for v, cam in enumerate(st["cameras"]):
        want = np.concatenate([cam["center"], cam["up"], cam["forward"], [cam["focal_length"]]])
        diff = max(diff, float(np.max(np.abs(o["cameras"][v] - want))))
        assert (cam["counted"] == 0) == (o["cameras"][v][9] == 0.0)
    assert diff <= bound, diff
    return st, diff


# ---- scenes -------------------------------------------------------------------------------------------------------------
def world_point(rng):
    """a homogeneous point at distance 1 to 20 from the origin, w in [0.5, 2]"""
    d = rng.normal(size=3)
    w = rng.uniform(0.5, 2.0)
    return np.concatenate([d / np.linalg.norm(d) * rng.uniform(1.0, 20.0) * w, [w]])


def random_export(seed, n_world, view_features, cap=8, n_extra_blocks=2, keep=0.6, room=None, world_pad=0, max_len=3):
    """A reconstruction of n_world landmarks: a fraction `keep` has a point, the rest is akz_tri_none or w == +-0; every list
    has 1 .. max_len observations but for a few tombstones.  view_features: per view how many of its features have a landmark
    with a Euclidean point — the other features below its count name nothing, a row without a point or a row outside the world
    table.  `world_pad` rows of the world table lie behind the landmark table."""
    rng = np.random.default_rng(seed)
    n_views = len(view_features)
    n_blocks = n_views + n_extra_blocks
    blocks = rng.permutation(n_blocks)[:n_views]
    poses = np.stack([random_pose(rng) for _ in range(n_blocks)])
    world = np.zeros((n_world, 4))
    kind = rng.random(n_world)
    for l in range(n_world):
        if kind[l] < keep:
            world[l] = world_point(rng)
        elif kind[l] < keep + (1 - keep) / 2:
            world[l] = NO_POINT
        else:
            world[l] = world_point(rng)
            world[l, 3] = 0.0 if l % 2 else -0.0
    rows = []
    for l in range(n_world - world_pad):
        n = 0 if rng.random() < 0.05 else int(rng.integers(1, max_len + 1))
        rows.append([(int(rng.integers(0, n_blocks)), int(rng.integers(0, cap))) for _ in range(n)])
    with_point = np.flatnonzero(world[:, 3] > 0)
    without = np.flatnonzero(~(world[:, 3] > 0))
    counts = np.zeros(n_blocks, np.uint32)
    lm = np.full((n_blocks, cap), NONE, np.uint32)
    for b, k in zip(blocks, view_features):
        k = min(k, cap) if len(with_point) else 0
        count = min(cap, k + int(rng.integers(0, 4)))
        counts[b] = count
        slots = rng.permutation(count)
        if k:
            lm[b, slots[:k]] = rng.choice(with_point, k)
        for j in slots[k:]:
            lm[b, j] = [NONE, n_world + int(j), int(rng.choice(without)) if len(without) else NONE][int(rng.integers(0, 3))]
        lm[b, count:] = rng.choice(with_point, cap - count) if len(with_point) else NONE         # behind the count: not looked at
    return inputs(world, rows, blocks, counts, lm, poses, cap, room=room, seed=seed)


def small(world, rows, room=None, cap=4, view_landmarks=(0, 1), count=2, start=None, start_obs=None):
    """two views (blocks 2 and 0 of 3) over a hand-written world table; both views see `view_landmarks`"""
    rng = np.random.default_rng(len(world))
    poses = np.stack([random_pose(rng) for _ in range(3)])
    lm = np.full((3, cap), NONE, np.uint32)
    for b in (0, 2):
        lm[b, :len(view_landmarks)] = view_landmarks
    return inputs(world, rows, [2, 0], [count, 0, count], lm, poses, cap, room=room, start=start, start_obs=start_obs)


def designed_cases():
    """name -> inputs.  P is a point at (1, 2, 4) / w."""
    P = lambda w: (1.0 * w, 2.0 * w, 4.0 * w, w)
    five = [P(1.0), P(1e-300), (1.0, 2.0, 4.0, 0.0), (1.0, 2.0, 4.0, -0.0), NO_POINT]
    lists = [[(0, 1), (2, 3)], [(2, 0), (0, 2)], [(1, 1)], [(1, 2)], [(0, 0), (1, 0)]]
    three = [P(1.0), P(2.0), P(0.5)]
    return {
        "w of 1, 1e-300, +0, -0 and -1": small(five, lists),
        "an empty list under w > 0": small(three, [[(0, 1)], [], [(2, 2), (0, 3)]]),
        "a first observation outside the blocks": small(three, [[(3, 1), (0, 0)], [(0, 1)], [(2, 2)]]),
        "a first observation outside the capacity": small(three, [[(0, 4), (0, 0)], [(0, 1)], [(2, 2)]]),
        "a later observation outside the colours": small(three, [[(0, 1), (9, 9)], [(0, 1)], [(2, 2)]]),
        "room exact": small(three, [[(0, 1)], [(1, 1)], [(2, 2)]], room=3),
        "room one short": small(three, [[(0, 1)], [(1, 1)], [(2, 2)]], room=2),
        "room of none": small(three, [[(0, 1)], [(1, 1)], [(2, 2)]], room=0),
        "a view with no feature that has a point": small(five, lists, view_landmarks=(2, 4, NONE), count=3),
        "a landmark key at and above n_world": small(three, [[(0, 1)], [(1, 1)], [(2, 2)]], view_landmarks=(3, 0, 7), count=3),
        "a count above the capacity": small(three, [[(0, 1)], [(1, 1)], [(2, 2)]], view_landmarks=(0, 1, 2, 0), count=9),
        "a world row behind the landmark table": small(three + [P(1.0)], [[(0, 1)], [(1, 1)], [(2, 2)]]),
        "no landmark": small([], []),
        "starts that do not ascend": small(three, None, start=[0, 2, 1, 3], start_obs=[(0, 1), (1, 1), (2, 2)]),
        "a first start above 0": small(three, None, start=[1, 1, 2, 3], start_obs=[(0, 1), (1, 1), (2, 2)]),
        "a last start above n_obs": small(three, None, start=[0, 1, 2, 4], start_obs=[(0, 1), (1, 1), (2, 2)]),
    }


BAD_TABLES = ("starts that do not ascend", "a first start above 0", "a last start above n_obs")
