"""Which frames a frame is compared with, in plain numpy / Python, written from the reference line by line, and a catalogue of
designed frame tables.

Nothing here imports the product (cv_amd), the C oracle (oracle/) or ctypes.  What is stated, per query:

  find_one   VSlamData::find_visually_similar_and_recent_frames (cv-sfm/src/lib.rs:597-668) and the order try_localize gives its
             result (:853-855).  `recent_frames` is the feed's own list filtered by |feed_frame - ix| < num_recent_frames, the
             frame itself left out (:611-621); `similar_frames` is knn_values(lsh, search_num) through the filter_map of :626-636
             and take(num_similar_frames) (:637); the chain of the two is split into a map reconstruction -> views and a list of
             free frames (:643-652); try_localize sorts the map's entries by Reverse(len) (:853-855).
             The reference's knn_values asks an approximate index; the project's statement is the exact answer, hash_knn of
             tests/matching_statement.py: ascending (distance, insertion order), the query's own row like any other.  The
             reference leaves reconstructions with equal counts to a HashMap and an unstable sort; the project documents
             ascending reconstruction key.
  replay     the reference's sequence literally: a table that grows by one frame, and the question asked about the frame that was
             just inserted (add_frame, :790-806) — find_one with visible = query + 1 says the same.

A frame table is a dict of arrays in insertion order: hashes [n][hash_bytes] uint8, feed / pos / recon / view [n] uint32 (recon
NONE: Frame::view is None).  The feed's own list `self.feed(feed).frames` is the visible frames of the feed by position; a
well-formed table has one frame per (feed, pos), and a query whose window holds two is refused (BAD_TABLE), as is a query that
names no visible stored row (BAD_INDEX).  Params: dict num_similar, num_recent, recent_threshold, search_num.
"""
import numpy as np

from matching_statement import hash_knn

NONE = 0xFFFFFFFF
OK, BAD_INDEX, BAD_TABLE = 0, 1, 2
C_RECENT, C_SIMILAR, C_SEARCHED, C_GROUPS, C_FREE, COUNTS = 0, 1, 2, 3, 4, 5
DEFAULTS = dict(num_similar=0, num_recent=32, recent_threshold=0, search_num=512)       # settings.rs:437-451


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def room(p):
    """every slot of the window but the query's own, and the similar frames"""
    return max(2 * p["num_recent"] - 2, 0) + p["num_similar"]


# ------------------------------------------------------------------------------------------------ the statement
def abs_difference(a, b):
    return a - b if a > b else b - a


def find_one(t, query, visible, p):
    """-> dict(verdict, recent, search = (rows, distances), similar, groups = [(reconstruction, [views])], free)"""
    n = len(t["feed"])
    if query >= n or visible > n or query >= visible:
        return dict(verdict=BAD_INDEX)
    feed, pos = t["feed"][:visible], t["pos"][:visible]
    frame, frame_feed, frame_feed_ix = query, int(feed[query]), int(pos[query])
    # self.feed(feed).frames: the feed's frames by position
    frames = sorted((int(pos[r]), int(r)) for r in np.flatnonzero(feed == frame_feed))
    window = [ix for ix, _ in frames if abs_difference(frame_feed_ix, ix) < p["num_recent"]]
    if len(set(window)) != len(window):
        return dict(verdict=BAD_TABLE)
    recent_frames = [recent_frame for ix, recent_frame in frames
                     if recent_frame != frame and abs_difference(frame_feed_ix, ix) < p["num_recent"]]
    rows, dists = hash_knn(t["hashes"][query], t["hashes"][:visible], p["search_num"])
    similar_frames = []
    for found_frame in (int(r) for r in rows):
        is_too_close = int(feed[found_frame]) == frame_feed and abs_difference(frame_feed_ix, int(pos[found_frame])) < p["recent_threshold"]
        if found_frame == frame or found_frame in recent_frames or is_too_close:
            continue
        similar_frames.append(found_frame)
    similar_frames = similar_frames[:p["num_similar"]]
    reconstruction_frames, free_frames = {}, []
    for found_frame in recent_frames + similar_frames:
        if int(t["recon"][found_frame]) != NONE:
            reconstruction_frames.setdefault(int(t["recon"][found_frame]), []).append(int(t["view"][found_frame]))
        else:
            free_frames.append(found_frame)
    groups = sorted(reconstruction_frames.items(), key=lambda kv: (-len(kv[1]), kv[0]))
    return dict(verdict=OK, recent=recent_frames, search=(rows, dists), similar=similar_frames, groups=groups, free=free_frames)


def replay(t, p):
    """One frame after another: the table holds the frames so far, the question is about the newest."""
    out = []
    for k in range(len(t["feed"])):
        grown = {name: a[:k + 1] for name, a in t.items()}
        out.append(find_one(grown, k, k + 1, p))
    return out


def outputs(t, queries, visible, p, pitch=None, fill=NONE, search=True):
    """The call's output arrays as the ABI lays them out (uint32), `fill` wherever the call does not write."""
    nq, n = len(queries), len(t["feed"])
    R = room(p) if pitch is None else pitch
    f = lambda *shape: np.full(shape, fill, np.uint32)
    o = dict(found=f(nq, R), views_out=f(nq, R), group_recon=f(nq, R), group_start=f(nq, R + 1), free=f(nq, R), counts=f(nq, COUNTS),
             verdict=f(nq))
    if search:
        o["search"] = f(nq, p["search_num"], 2)
    for k, q in enumerate(queries):
        r = find_one(t, int(q), n if visible is None else int(visible[k]), p)
        o["verdict"][k] = r["verdict"]
        o["counts"][k] = 0
        if r["verdict"] != OK:
            continue
        chain = r["recent"] + r["similar"]
        o["found"][k, :len(chain)] = chain
        o["free"][k, :len(r["free"])] = r["free"]
        at = 0
        for g, (key, views) in enumerate(r["groups"]):
            o["group_recon"][k, g] = key
            o["group_start"][k, g] = at
            o["views_out"][k, at:at + len(views)] = views
            at += len(views)
        o["group_start"][k, len(r["groups"])] = at
        if search:
            o["search"][k, :len(r["search"][0]), 0] = r["search"][0]
            o["search"][k, :len(r["search"][0]), 1] = r["search"][1]
        o["counts"][k] = [len(r["recent"]), len(r["similar"]), len(r["search"][0]), len(r["groups"]), len(r["free"])]
    return o


# ------------------------------------------------------------------------------------------------ the catalogue
# Every case is a function of its arguments alone (generators seeded from them).

def _rng(*key):
    return np.random.default_rng([0x504C, *[int(k) & 0xFFFFFFFF for k in key]])


def table(hashes, feed, pos, recon=None, view=None):
    n = len(feed)
    u = lambda a: np.ascontiguousarray(a, np.uint32)
    return dict(hashes=np.ascontiguousarray(hashes, np.uint8).reshape(n, -1), feed=u(feed), pos=u(pos),
                recon=np.full(n, NONE, np.uint32) if recon is None else u(recon), view=u(np.arange(n) + 1000 if view is None else view))


def interleaved(n, n_feeds):
    """(feed, pos): frame i belongs to feed i % n_feeds and is its feed's next frame"""
    i = np.arange(n)
    return i % n_feeds, i // n_feeds


def with_views(t, seed, n_recons=3, share=0.6):
    """a share of the frames gets a view in one of n_recons reconstructions (keys 7, 14, ...)"""
    rng = _rng(seed, len(t["feed"]))
    has = rng.random(len(t["feed"])) < share
    t["recon"] = np.where(has, 7 * (1 + rng.integers(0, n_recons, len(has))), NONE).astype(np.uint32)
    return t


def near(base, bits, rng):
    """a copy of the hash `base` with `bits` distinct bits flipped"""
    h = base.copy()
    for b in rng.choice(8 * len(h), bits, replace=False):
        h[b >> 3] ^= 1 << (b & 7)
    return h


def random_table(n, hash_bytes, seed, n_feeds=2, few_values=False):
    """random hashes (few_values: bytes of 0 / 255 only, so that many distances tie) over interleaved feeds, views on a share"""
    rng = _rng(seed, n, hash_bytes)
    h = rng.integers(0, 2, (n, hash_bytes), dtype=np.uint8) * 255 if few_values else rng.integers(0, 256, (n, hash_bytes), dtype=np.uint8)
    return with_views(table(h, *interleaved(n, n_feeds)), seed)


def case(t, queries, p, visible=None):
    return dict(table=t, queries=np.ascontiguousarray(queries, np.uint32), visible=None if visible is None else np.ascontiguousarray(visible, np.uint32),
                params=p)


def size_case(n, nq, hash_bytes=64, seed=0, **kw):
    """n stored rows, nq queries drawn from them (again and again where nq > n)"""
    t = random_table(n, hash_bytes, seed)
    q = _rng(seed, n, nq).integers(0, n, nq)
    return case(t, q, params(**{**dict(num_similar=4, num_recent=3, search_num=16), **kw}))


def complement_case(hash_bytes):
    """a hash, its complement (the largest distance), and one a bit away from each"""
    rng = _rng(hash_bytes)
    h = rng.integers(0, 256, hash_bytes, dtype=np.uint8)
    rows = [h, ~h, near(h, 1, rng), near(~h, 1, rng)]
    return case(table(rows, *interleaved(4, 4)), [0, 1, 2, 3], params(num_similar=3, num_recent=0, search_num=4))


def ties_at_the_cut(search_num=8, n=40, hash_bytes=64, seed=0):
    """Around the query (row n // 2): search_num - 3 rows nearer than distance 5, then a block of 6 rows at distance 5 that
    straddles the cut (3 inside), the rest far; the rows shuffled, so that only the row order decides inside the block."""
    rng = _rng(seed, search_num, n)
    base = rng.integers(0, 256, hash_bytes, dtype=np.uint8)
    kinds = [0] + [1 + k % 4 for k in range(search_num - 4)] + [5] * 6
    kinds += [40 + k for k in range(n - len(kinds))]
    order = rng.permutation(n)
    hashes = np.zeros((n, hash_bytes), np.uint8)
    for place, bits in zip(order, kinds):
        hashes[place] = near(base, bits, rng)
    query = int(order[0])
    return case(with_views(table(hashes, *interleaved(n, 3)), seed), [query], params(num_similar=search_num, num_recent=2, search_num=search_num))


def query_outside_its_own_list(search_num=4, copies=7):
    """more than search_num rows equal to the query's hash at lower rows: the query is not in its own search list"""
    rng = _rng(search_num, copies)
    base = rng.integers(0, 256, 64, dtype=np.uint8)
    hashes = [base] * (copies + 1) + [near(base, 3 + k, rng) for k in range(5)]
    return case(table(hashes, *interleaved(len(hashes), 2)), [copies, 0, copies + 2], params(num_similar=search_num, num_recent=0, search_num=search_num))


def widest_case(n=2100, seed=0):
    """search_num = num_similar = 2048 and num_recent = 256 over 4-byte hashes of few values: every limit at once, ties everywhere"""
    t = random_table(n, 4, seed, n_feeds=1, few_values=True)
    return case(t, [0, n // 2, n - 1], params(num_similar=2048, num_recent=256, search_num=2048))


def window_case(n, n_feeds, num_recent, queries, num_similar=2, seed=0):
    """the recent window alone matters: clipped at the feed's ends for the first and last frames"""
    t = random_table(n, 64, seed, n_feeds=n_feeds)
    return case(t, queries, params(num_similar=num_similar, num_recent=num_recent, search_num=8))


def near_and_recent(seed=0, n=30):
    """One feed; the frames next to the query in the feed are also the nearest hashes: they are recent, are dropped from the
    similar frames and do not use up the take, which goes to the next nearest."""
    rng = _rng(seed, n)
    base = rng.integers(0, 256, 64, dtype=np.uint8)
    q = n // 2
    hashes = np.stack([near(base, 1 + abs(i - q), rng) if i != q else base for i in range(n)])
    return case(with_views(table(hashes, *interleaved(n, 1)), seed), [q, 0, n - 1], params(num_similar=3, num_recent=4, search_num=16))


def threshold_case(seed=0, n=40):
    """Two feeds at the same positions, all hashes close to one base: recent_threshold (10, above num_recent = 2) drops the
    frames of the query's feed near it in the feed, not the other feed's at the same positions."""
    rng = _rng(seed, n, 1)
    base = rng.integers(0, 256, 64, dtype=np.uint8)
    hashes = np.stack([near(base, 1 + (i * 7) % 11, rng) for i in range(n)])
    return case(with_views(table(hashes, *interleaved(n, 2)), seed), [20, 21, 0], params(num_similar=12, num_recent=2, recent_threshold=10, search_num=40))


def groups_case(kind, seed=0):
    """One feed of 24 frames, window of 8 either way, every frame outside it a similar one.  "free": no frame has a view; "three":
    three reconstructions, keys 9 and 5 with four views found each (three recent, one similar) and key 30 with two; "own": the
    query's frame has a view itself."""
    n, q = 24, 12
    t = random_table(n, 64, seed, n_feeds=1)
    recon = np.full(n, NONE, np.uint32)
    if kind != "free":
        recon[[5, 7, 9]] = 9
        recon[[6, 8, 10]] = 5
        recon[[13, 14]] = 30
        recon[0], recon[23] = 5, 9   # outside the window: found only as similar frames
    if kind == "own":
        recon[q] = 9
    t["recon"] = recon
    return case(t, [q], params(num_similar=7, num_recent=8, search_num=24))


def growing_case(n=80, seed=0, **kw):
    """every frame asks when it has just been inserted: visible = query + 1"""
    t = random_table(n, 64, seed, n_feeds=3)
    return case(t, np.arange(n), params(**{**dict(num_similar=5, num_recent=4, search_num=12), **kw}), visible=np.arange(n) + 1)


def refusal_case(seed=0, n=40):
    """Queries 0 and 3 answer; 1 names row n, 2 has visible = n + 1, 4 is not below its visible; 5's window holds two frames of
    one (feed, pos) (rows 30 and 31, both at position 30), which the windows of queries 0 and 3, far away in the feed, do not."""
    t = random_table(n, 64, seed, n_feeds=1)
    t["pos"][31] = 30
    return case(t, [2, n, 5, 3, 9, 29], params(num_similar=3, num_recent=4, search_num=8), visible=[n, n, n + 1, n, 9, n])


def cases():
    """name -> case: the catalogue both builds are held to"""
    c = {}
    for n in (1, 63, 64, 65, 197):
        for nq in (1, 65):
            c[f"size_n{n}_q{nq}"] = size_case(n, nq)
    for hb in (4, 64, 512, 4096):
        c[f"hash_bytes_{hb}"] = size_case(70, 3, hash_bytes=hb, seed=hb)
        c[f"complement_{hb}"] = complement_case(hb)
    c["ties_at_the_cut"] = ties_at_the_cut()
    c["ties_at_the_cut_wide"] = ties_at_the_cut(search_num=70, n=200, seed=1)
    c["query_outside_its_own_list"] = query_outside_its_own_list()
    c["search_num_1"] = size_case(50, 4, search_num=1, num_similar=1, seed=3)
    c["search_num_above_visible"] = size_case(30, 4, search_num=512, num_similar=512, seed=4)
    c["widest"] = widest_case()
    c["window_clipped"] = window_case(40, 1, 32, [0, 39, 20, 5])
    c["window_two_feeds"] = window_case(61, 2, 5, [0, 1, 30, 31, 59, 60])
    for nr in (0, 1, 32):
        c[f"num_recent_{nr}"] = window_case(90, 2, nr, [0, 44, 45, 89], seed=nr)
    c["num_recent_256"] = window_case(600, 1, 256, [0, 300, 599], seed=256)
    c["near_and_recent"] = near_and_recent()
    c["recent_threshold"] = threshold_case()
    c["num_similar_0"] = size_case(50, 5, num_similar=0, seed=5)
    c["num_similar_search_num"] = size_case(50, 5, num_similar=16, seed=6)
    for kind in ("free", "three", "own"):
        c[f"groups_{kind}"] = groups_case(kind)
    c["growing"] = growing_case()
    c["sees_newer_rows"] = case(random_table(80, 64, 0, n_feeds=3), np.arange(0, 80, 7), params(num_similar=5, num_recent=4, search_num=12))
    c["refusals"] = refusal_case()
    c["room_0"] = size_case(20, 3, num_similar=0, num_recent=1, seed=7)
    return c


def many_queries_case(n=20000, nq=1700):
    """more queries than one pass of the device code takes at this table size (4-byte hashes: ties everywhere)"""
    t = random_table(n, 4, 11, n_feeds=64, few_values=True)
    return case(t, _rng(n, nq).integers(0, n, nq), params(num_similar=2, num_recent=2, search_num=4))


def largest_case():
    """20 000 stored rows of 512 bytes, 64 queries, the defaults with num_similar = 8"""
    t = random_table(20000, 512, 9, n_feeds=4)
    return case(t, _rng(20000).integers(0, 20000, 64), params(num_similar=8))
