"""The designed tables the repack tests walk (tests/test_repack_math.py on the host build, tests/test_gpu_repack.py on the
device), and the three ways to an answer: the host build of include/akz_repack_math.h (tests/cpp/repack_host.c), the
statement (tests/repack_statement.py) and, for a refusal, the empty table the header specifies.  Every answer is a dict of whole
output arrays that started from one fill (POISON), so that "every word written" is part of every comparison.

None of the tables is random: each is the smallest shape at which a pass of cv_amd/csrc/rs_repack.hip can go wrong — the edges
of RS_LT_TILE in the row count, rows of 1, 63, 64, 65 and 129 observations around the wave, dropped rows at the first and last
place of a tile, a whole tile dropped, tombstones, an empty tail, broken starts, maps and indices, rooms one short."""
import ctypes as C

import numpy as np

import host_build
import repack_statement as stmt

NONE = 0xFFFFFFFF
POISON = 0xA5A5A5A5
OK, BAD_TABLE, BAD_INDEX, BAD_MAP, NO_ROOM = range(5)
CAP = 64
TILE = 1024
BIG_BLOCKS, BIG_LIVE = 133, 100          # the large tables: views 100 .. 132 hold the rows that are to lose everything
LONG_ROWS = {2: 63, 3: 64, 5: 65, 6: 129, 1022: 65, 1023: 129, 1024: 64, 1030: 129}


class Case:
    def __init__(self, name, rows, n_blocks, block_map, n_blocks_out, expect=OK, recon_start=None, statement=True, n_obs=None,
                 start=None, obs_room=None, lm_room=None, cap=CAP, behind=0):
        self.name, self.n_blocks, self.n_blocks_out, self.expect, self.cap = name, n_blocks, n_blocks_out, expect, cap
        self.map = None if block_map is None else np.array(block_map, np.uint32)
        flat = [o for row in rows for o in row] + [(NONE, NONE)] * behind       # `behind`: observations that are not the table's
        self.obs = np.array(flat, np.uint32).reshape(-1, 2)
        self.start = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint32) if start is None else np.array(start, np.uint32)
        self.n_landmarks = len(self.start) - 1
        self.n_obs = len(flat) if n_obs is None else n_obs
        self.recon_start = None if recon_start is None else np.array(recon_start, np.uint32)
        self.statement = statement and expect == OK
        self.obs_room = n_blocks_out * cap if obs_room is None else obs_room
        self.lm_room = n_blocks_out * cap if lm_room is None else lm_room

    def list_map(self):
        return list(range(self.n_blocks)) if self.map is None else [int(m) for m in self.map]

    def removed(self):
        return [v for v, m in enumerate(self.list_map()) if m == NONE]

    def __repr__(self):
        return self.name


class Features:
    """hands every feature of a view out once: the tables are the reference's kind unless a case breaks one on purpose"""

    def __init__(self, n_blocks, cap=CAP):
        self.next, self.cap = [0] * n_blocks, cap

    def row(self, views):
        out = []
        for v in views:
            assert self.next[v] < self.cap, "the designed table outgrew a view"
            out.append((v, self.next[v]))
            self.next[v] += 1
        return out


def big_rows(n, doomed=(), tombstones=True):
    """n rows over BIG_BLOCKS views: lengths 1, 2, 3, 2 and a tombstone in turn, the LONG_ROWS (129 reaches into the doomed
    views: a wide row that keeps a part), and the rows of `doomed`, which observe a doomed view alone"""
    feats = Features(BIG_BLOCKS)
    rows = []
    for r in range(n):
        if r in doomed:
            views = [BIG_LIVE + r % (BIG_BLOCKS - BIG_LIVE)]
        elif r in LONG_ROWS:
            L = LONG_ROWS[r]
            views = [(r + i) % BIG_BLOCKS for i in range(L)] if L > BIG_LIVE else [(3 * r + i) % BIG_LIVE for i in range(L)]
        elif tombstones and r % 5 == 4:
            views = []
        else:
            views = [(3 * r + i) % BIG_LIVE for i in range((1, 2, 3, 2, 1)[r % 5])]
        rows.append(feats.row(views))
    return rows


BIG_MAP = [BIG_LIVE - 1 - b for b in range(BIG_LIVE)] + [NONE] * (BIG_BLOCKS - BIG_LIVE)      # the live views reversed, the doomed removed


def small_rows(n_blocks, n=40, doomed_head=0):
    """n rows over n_blocks views: lengths 1, 2, 3, min(5, n_blocks), a tombstone, 2 in turn.  doomed_head: so many rows in front
    observe the last view alone, which no other row then uses"""
    feats = Features(n_blocks)
    usable = n_blocks - (1 if doomed_head else 0)
    rows = []
    for r in range(n):
        if r < doomed_head:
            rows.append(feats.row([n_blocks - 1]))
            continue
        L = (1, 2, 3, min(5, usable), 0, 2)[r % 6]
        rows.append(feats.row([(r + i) % usable for i in range(L)]))
    return rows


def compact(n_blocks, removed):
    """the map that removes `removed` and closes the gaps -> (map, n_blocks_out)"""
    m, k = [], 0
    for b in range(n_blocks):
        m.append(NONE if b in removed else k)
        k += b not in removed
    return m, k


def kept_counts(case):
    """(rows kept, observations kept), counted on the arrays"""
    m, rows, observations = case.list_map(), 0, 0
    for r in range(case.n_landmarks):
        k = sum(1 for i in range(int(case.start[r]), int(case.start[r + 1])) if m[int(case.obs[i, 0])] != NONE)
        rows += k > 0
        observations += k
    return rows, observations


def table_cases():
    cases = []
    add = cases.append
    # ---- rows: the edges of the tile, the row lengths around the wave, tombstones interleaved
    for n in (0, 1, 1023, 1024, 1025, 2049):
        add(Case(f"rows_{n}", big_rows(n), BIG_BLOCKS, BIG_MAP, BIG_LIVE))
    # ---- drop patterns over three tiles
    n = 2 * TILE + 1
    add(Case("drop_first_of_tile", big_rows(n, {0, TILE, 2 * TILE}), BIG_BLOCKS, BIG_MAP, BIG_LIVE))
    add(Case("drop_last_of_tile", big_rows(n, {TILE - 1, 2 * TILE - 1}), BIG_BLOCKS, BIG_MAP, BIG_LIVE))
    add(Case("drop_whole_tile", big_rows(n, set(range(TILE, 2 * TILE))), BIG_BLOCKS, BIG_MAP, BIG_LIVE))
    add(Case("drop_every_row", big_rows(n), BIG_BLOCKS, [NONE] * BIG_BLOCKS, BIG_LIVE))
    add(Case("drop_no_row_identity", big_rows(n, tombstones=False), BIG_BLOCKS, None, BIG_BLOCKS))
    add(Case("drop_no_row_reversal", big_rows(n, tombstones=False), BIG_BLOCKS, list(range(BIG_BLOCKS))[::-1], BIG_BLOCKS))
    # ---- sizes and maps
    for nb in (5, 9):
        rows = small_rows(nb)
        add(Case(f"b{nb}_identity_null", rows, nb, None, nb))
        add(Case(f"b{nb}_identity", rows, nb, list(range(nb)), nb))
        add(Case(f"b{nb}_reversal", rows, nb, list(range(nb))[::-1], nb))
        for what, gone in (("first", {0}), ("middle", {nb // 2}), ("last", {nb - 1}), ("below", {1, nb - 2})):
            m, out = compact(nb, gone)
            add(Case(f"b{nb}_{what}_removed", rows, nb, m, out))
        add(Case(f"b{nb}_all_removed", rows, nb, [NONE] * nb, nb))
        add(Case(f"b{nb}_all_removed_no_blocks_out", rows, nb, [NONE] * nb, 0))
        add(Case(f"b{nb}_out_above", rows, nb, [2 * b + 1 for b in range(nb)], 2 * nb + 1))
        add(Case(f"b{nb}_shared_target", rows, nb, [0, 1, 1] + list(range(3, nb)), nb, BAD_MAP))
        add(Case(f"b{nb}_target_is_n_blocks_out", rows, nb, list(range(1, nb + 1)), nb, BAD_MAP))
    # ---- table shapes
    nb = 9
    rows = small_rows(nb)
    first, out = compact(nb, {0})
    total = sum(len(r) for r in rows)
    add(Case("empty_tail_3000", rows + [[]] * 3000, nb, first, out))
    add(Case("start_above_n_obs", rows, nb, first, out, BAD_TABLE, n_obs=total - 1))
    add(Case("observations_behind_the_table", rows, nb, first, out, behind=7))
    broken = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    broken[11] = broken[10] - 1
    add(Case("descending_starts", rows, nb, first, out, BAD_TABLE, start=broken))
    add(Case("feature_in_two_rows", rows + [[rows[1][0]], [rows[0][0]]], nb, list(range(nb))[::-1], nb, statement=False))
    # ---- rooms: exactly the kept counts, and one less in each
    for name, base in (("small", Case("", rows, nb, first, out)), ("big", Case("", big_rows(n, {0, TILE}), BIG_BLOCKS, BIG_MAP, BIG_LIVE))):
        k_rows, k_obs = kept_counts(base)
        mk = lambda nm, expect, **kw: Case(f"rooms_{name}_{nm}", [], base.n_blocks, base.map, base.n_blocks_out, expect, start=base.start, **kw)
        for c in (mk("exact", OK, lm_room=k_rows, obs_room=k_obs), mk("one_row_short", NO_ROOM, lm_room=k_rows - 1, obs_room=k_obs),
                  mk("one_observation_short", NO_ROOM, lm_room=k_rows, obs_room=k_obs - 1)):
            c.obs, c.n_obs = base.obs, base.n_obs
            add(c)
    # ---- ranges: three reconstructions, one that loses every row and one empty; broken ranges
    rows = small_rows(nb, doomed_head=10)
    last, out = compact(nb, {nb - 1})
    add(Case("ranges_three", rows, nb, last, out, recon_start=[0, 10, 10, 40]))
    add(Case("ranges_identity", rows, nb, None, nb, recon_start=[0, 10, 10, 40]))
    add(Case("ranges_descending_starts", rows, nb, last, out, BAD_TABLE, recon_start=[0, 20, 10, 40]))
    add(Case("ranges_beyond_the_table", rows, nb, last, out, BAD_TABLE, recon_start=[0, 10, 41]))
    # ---- bad indices
    rows = small_rows(nb)
    bad = [list(r) for r in rows]
    bad[7][0] = (nb, 0)
    add(Case("block_is_n_blocks", bad, nb, first, out, BAD_INDEX))
    v, f = next((v, f) for v, f in rows[8] if v != 0)
    bad = [list(r) for r in rows]
    bad[8] = [(v, CAP) if o == (v, f) else o for o in bad[8]]
    add(Case("kept_feature_is_cap", bad, nb, first, out, BAD_INDEX))
    r0 = next(k for k, r in enumerate(rows) if any(o[0] == 0 for o in r))
    bad = [list(r) for r in rows]
    bad[r0] = [(0, CAP) if o[0] == 0 else o for o in bad[r0]]
    add(Case("dropped_feature_is_cap", bad, nb, first, out, OK, statement=False))
    # where several apply: table, map, index, room
    add(Case("bad_map_and_bad_index", bad[:7] + [[(nb, 0)]], nb, [0, 0] + list(range(2, nb)), nb, BAD_MAP))
    assert len({c.name for c in cases}) == len(cases)
    return cases


SUMS_PASS = 256                          # tile sums one trip of k_rp_scan_sums takes (kRpBlock of cv_amd/csrc/rs_repack.hip)
SUMS_CAP = 4096                          # features per view of the tables below: BIG_LIVE * SUMS_CAP rows have room


def tile_sums_case(name, n, doomed):
    """n rows of ONE observation each, built with numpy alone: row r observes live view r % BIG_LIVE at feature r // BIG_LIVE;
    the k-th row of `doomed` observes a doomed view alone and loses everything under BIG_MAP.  No feature is handed out twice."""
    doomed = np.array(sorted(doomed), np.int64)
    assert n <= BIG_LIVE * SUMS_CAP and (len(doomed) == 0 or (doomed[0] >= 0 and doomed[-1] < n))
    r = np.arange(n, dtype=np.int64)
    obs = np.stack([r % BIG_LIVE, r // BIG_LIVE], 1)
    k = np.arange(len(doomed), dtype=np.int64)
    obs[doomed] = np.stack([BIG_LIVE + k % (BIG_BLOCKS - BIG_LIVE), k // (BIG_BLOCKS - BIG_LIVE)], 1)
    c = Case(name, [], BIG_BLOCKS, BIG_MAP, BIG_LIVE, start=np.arange(n + 1), cap=SUMS_CAP, statement=False)
    c.obs, c.n_obs, c.doomed = np.ascontiguousarray(obs.astype(np.uint32)).reshape(-1, 2), n, doomed
    return c


def tile_sums_cases():
    """Tables on either side of one trip of the tile-sum scan: SUMS_PASS tiles exactly, one row more, three rows more.  The rows
    removed are sparse — one in TILE + 7, so every tile and every trip keeps a sum that is not zero and no two tiles lose the
    same place — plus the rows next to the trip's boundary: the last of the first trip in every table and, where the second trip
    has more than one row, one of its own between two kept ones."""
    edge = SUMS_PASS * TILE
    sparse = set(range(5, edge, TILE + 7))
    return [tile_sums_case("rows_256T", edge, sparse | {edge - 1}),
            tile_sums_case("rows_256T+1", edge + 1, sparse | {edge - 1}),
            tile_sums_case("rows_256T+3", edge + 3, sparse | {edge - 1, edge + 1})]


def direct_table(case):
    """The answer for a tile_sums_case-like table — every row one observation, a valid map, rooms that hold everything — by
    numpy alone, not through the host build: the kept rows close up in order."""
    o = blank(case)
    m = np.array(case.list_map(), np.uint32)
    obs = case.obs[:case.n_landmarks]
    assert np.array_equal(case.start, np.arange(case.n_landmarks + 1)) and case.recon_start is None
    to = m[obs[:, 0]]
    keep = to != NONE
    rows = int(keep.sum())
    assert rows <= case.lm_room and rows <= case.obs_room
    o["obs_start_out"][:rows] = np.arange(rows)
    o["obs_start_out"][rows:] = rows
    o["obs_counts_out"][:case.lm_room] = 0
    o["obs_counts_out"][:rows] = 1
    o["obs_out"][:rows] = np.stack([to[keep], obs[keep, 1]], 1)
    o["landmarks_out"][:case.n_blocks_out] = NONE
    o["landmarks_out"][to[keep], obs[keep, 1]] = np.arange(rows, dtype=np.uint32)
    o["key_out"][:case.n_landmarks] = NONE
    o["key_out"][np.flatnonzero(keep)] = np.arange(rows, dtype=np.uint32)
    o["counts_out"][:] = (rows, rows, 0, case.n_landmarks - rows, case.n_landmarks - rows)
    o["call_verdict"][0] = OK
    return o


# ---------------------------------------------------------------------------------------------------------------------------
def blank(case):
    """the output arrays of a table call, every word POISON"""
    w = lambda *shape: np.full(shape, POISON, np.uint32)
    o = dict(obs_start_out=w(case.lm_room + 1), obs_out=w(max(case.obs_room, 1), 2), obs_counts_out=w(max(case.lm_room, 1)),
             landmarks_out=w(max(case.n_blocks_out, 1), case.cap), key_out=w(max(case.n_landmarks, 1)), counts_out=w(5), call_verdict=w(1))
    if case.recon_start is not None:
        o["recon_start_out"] = w(len(case.recon_start))
    return o


def _lib():
    L = host_build.load("repack_host.c")
    vp, u32 = C.c_void_p, C.c_uint32
    L.rp_table.argtypes = [vp, vp, u32, u32, u32, u32, vp, u32, vp, u32, u32, u32] + [vp] * 8
    L.rp_gather.argtypes = [vp, vp, u32, u32, vp, u32, vp]
    L.rp_constraints.argtypes = [vp, vp, vp, u32, vp, u32, u32, vp, u32] + [vp] * 5
    L.rp_frames.argtypes = [vp, vp, u32, u32, vp, u32, vp]
    L.rp_frames.restype = None
    L.rp_constant.restype = u32
    return L


def ptr(a):
    return None if a is None else a.ctypes.data


def host_table(case):
    """the host build's answer"""
    o = blank(case)
    n_recons = 0 if case.recon_start is None else len(case.recon_start) - 1
    obs = np.ascontiguousarray(case.obs)
    st = _lib().rp_table(ptr(case.start), ptr(obs), case.n_obs, case.n_landmarks, case.cap, case.n_blocks, ptr(case.map), case.n_blocks_out,
                         ptr(case.recon_start), n_recons, case.obs_room, case.lm_room, ptr(o["obs_start_out"]), ptr(o["obs_out"]),
                         ptr(o["obs_counts_out"]), ptr(o["landmarks_out"]), ptr(o["key_out"]), ptr(o.get("recon_start_out")),
                         ptr(o["counts_out"]), ptr(o["call_verdict"]))
    assert st == 0
    return o


def refused_table(case, verdict, counts=(0, 0, 0, 0, 0)):
    """the empty table the header specifies for a refusal"""
    o = blank(case)
    o["obs_start_out"][:] = 0
    o["obs_counts_out"][:case.lm_room] = 0
    o["landmarks_out"][:case.n_blocks_out] = NONE
    o["key_out"][:case.n_landmarks] = NONE
    if "recon_start_out" in o:
        o["recon_start_out"][:] = 0
    o["counts_out"][:] = counts
    o["call_verdict"][0] = verdict
    return o


def statement_table(case, order=None):
    """the statement's answer for a table it can hold, the removed views taken in `order`"""
    order = case.removed() if order is None else order
    r = stmt.repack(case.start, case.obs, case.n_landmarks, case.n_blocks, case.cap, case.list_map(), order, recon_start=case.recon_start)
    o = blank(case)
    rows = r["rows"]
    total = sum(len(row) for row in rows)
    assert len(rows) <= case.lm_room and total <= case.obs_room
    o["obs_start_out"][:len(rows)] = np.cumsum([0] + [len(row) for row in rows])[:-1]
    o["obs_start_out"][len(rows):] = total
    o["obs_counts_out"][:case.lm_room] = 0
    o["obs_counts_out"][:len(rows)] = [len(row) for row in rows]
    o["landmarks_out"][:case.n_blocks_out] = NONE
    at = 0
    for key, row in enumerate(rows):
        for blk, feat in row:
            o["obs_out"][at] = (blk, feat)
            o["landmarks_out"][blk, feat] = key
            at += 1
    o["key_out"][:case.n_landmarks] = [r["key_of"].get(k, NONE) for k in range(case.n_landmarks)]
    if "recon_start_out" in o:
        o["recon_start_out"][:] = r["recon_start"]
    lens = case.start[1:].astype(np.int64) - case.start[:-1]
    empty = int(np.count_nonzero(lens == 0))
    o["counts_out"][:] = (len(rows), total, empty, case.n_landmarks - len(rows) - empty, int(lens.sum()) - total)
    o["call_verdict"][0] = OK
    return o


def same(a, b):
    """two answers are equal in every word; -> the first name that differs, or None"""
    assert a.keys() == b.keys()
    for k in a:
        if a[k].shape != b[k].shape or not np.array_equal(a[k], b[k]):
            return k
    return None


# ---- the pools ---------------------------------------------------------------------------------------------------------------
GATHER_ROW_BYTES = (4, 12, 16, 48, 96)


def gather_cases():
    """(name, n_blocks, map, n_blocks_out, expected verdict)"""
    nb = 9
    first, out = compact(nb, {0})
    return [("identity_null", nb, None, nb, OK), ("reversal", nb, list(range(nb))[::-1], nb, OK), ("first_removed", nb, first, out, OK),
            ("all_removed", nb, [NONE] * nb, nb, OK), ("out_above", nb, [2 * b + 1 for b in range(nb)], 2 * nb + 1, OK),
            ("shared_target", nb, [0, 1, 1] + list(range(3, nb)), nb, BAD_MAP), ("target_is_n_blocks_out", nb, list(range(1, nb + 1)), nb, BAD_MAP),
            ("many_blocks", 300, [NONE if b % 7 == 3 else 299 - b for b in range(300)], 300, OK)]


def pool(n_blocks, row_bytes):
    """a pool no two bytes of which are alike in a way a wrong row or a wrong offset would keep"""
    i = np.arange(n_blocks * row_bytes, dtype=np.uint64)
    return ((i * 2654435761 >> 7) & 0xFF).astype(np.uint8).reshape(n_blocks, row_bytes) | 1


def host_gather(src, row_bytes, n_blocks, block_map, n_blocks_out):
    dst = np.full((max(n_blocks_out, 1), row_bytes), 0xA5, np.uint8)
    verdict = np.full(1, POISON, np.uint32)
    m = None if block_map is None else np.array(block_map, np.uint32)
    assert _lib().rp_gather(ptr(src), ptr(dst), row_bytes, n_blocks, ptr(m), n_blocks_out, ptr(verdict)) == 0
    return dst, verdict


# (row_bytes, (src offset, dst offset), blocks): rows around the edges of k_rp_gather's unroll (256 units a slot), of its grid
# (1024 units a workgroup), the workload's row (cap 8192 x 28 bytes) and one beyond the grid's cap (256 workgroups x 1024 units)
GATHER_LONG_ROWS = ([(16 * u, (0, 0), 9) for u in (255, 256, 257, 1023, 1024, 1025)] + [(229376, (0, 0), 5), (16 * (262144 + 1), (0, 0), 3)] +
                    [(4 * 257, (4, 4), 9), (4 * 1025, (4, 4), 9), (4 * (262144 + 1), (4, 4), 3)])


def direct_gather(src, block_map, n_blocks_out):
    """the answer of a gather under a VALID map (or None, the identity) by numpy alone: row map[b] of dst is row b of src, a
    row nothing maps to is zeros"""
    dst = np.zeros((n_blocks_out, src.shape[1]), np.uint8)
    if block_map is None:
        dst[:] = src[:n_blocks_out]
        return dst
    m = np.asarray(block_map, np.uint32)
    kept = np.flatnonzero(m != NONE)
    assert len(set(m[kept].tolist())) == len(kept) and (len(kept) == 0 or int(m[kept].max()) < n_blocks_out)
    dst[m[kept]] = src[kept]
    return dst


# ---- the constraints -----------------------------------------------------------------------------------------------------------
def constraint_case(n, n_blocks=9):
    """n designed constraints over n_blocks views: every triple of distinct views in turn, so that with any one view removed
    some lose their first, some their second, some their third view; every seventh is a duplicate of the one before; poses
    and verdicts that tell every constraint from every other"""
    views = np.zeros((n, 3), np.uint32)
    for c in range(n):
        k = c - 1 if c % 7 == 6 else c
        a = k % n_blocks
        views[c] = (a, (a + 1 + k // n_blocks % (n_blocks - 2)) % n_blocks, (a + n_blocks - 1) % n_blocks)
    poses = (np.arange(n * 24, dtype=np.float64).reshape(n, 2, 12) + 0.5) * 1.25
    verdict = (np.arange(n, dtype=np.uint32) % 3).astype(np.uint32)
    return views, poses, verdict


def host_constraints(views, poses, verdict, block_map, n_blocks, n_blocks_out, start=None):
    n = len(views)
    w = lambda *shape: np.full(shape, POISON, np.uint32)
    o = dict(views_out=w(max(n, 1), 3), poses_out=np.full((max(n, 1), 2, 12), -7.0), verdict_out=w(max(n, 1)), count=w(1))
    m = None if block_map is None else np.array(block_map, np.uint32)
    s = None if start is None else np.array(start, np.uint32)
    if s is not None:
        o["start_out"] = w(len(s))
    st = _lib().rp_constraints(ptr(views), ptr(poses), ptr(verdict), n, ptr(m), n_blocks, n_blocks_out, ptr(s), 0 if s is None else len(s) - 1,
                               ptr(o["views_out"]), ptr(o["poses_out"]), ptr(o["verdict_out"]), ptr(o["count"]), ptr(o.get("start_out")))
    assert st == 0
    return o


def host_frames(recon, view, which, block_map, n_blocks):
    recon, view = recon.copy(), view.copy()
    flags = np.full(1, POISON, np.uint32)
    m = None if block_map is None else np.array(block_map, np.uint32)
    _lib().rp_frames(ptr(recon), ptr(view), len(recon), which, ptr(m), n_blocks, ptr(flags))
    return recon, view, flags
