"""The matcher stage in plain numpy / Python, written from the reference's definitions, and a catalogue of designed inputs.

Nothing here imports the product (cv_amd), the C oracle (oracle/) or ctypes.  What is stated:

  hamming            bitarray's Hamming distance of two BitArray<64>: the popcount of the XOR over all 64 bytes — all 512
                     bits.  (An extracted descriptor has bits 486..511 clear, akaze/src/descriptors.rs; the matcher's entry
                     points take any 64-byte row, so the pad bits count like every other.)
  knn                space 0.17 LinearKnn::knn(query, num): the first `num` items sorted by distance, every later item
                     inserted at partition_point(d <= new) and the tail popped.  An item is therefore kept in front of
                     another exactly when its distance is smaller, or equal with a smaller position: the result is the first
                     min(num, len) items of the targets in (distance, index) order.  knn_literal() is that insertion
                     procedure word for word, for small problems; knn() is the sorted form.
  match              matching() / symmetric_matching() of tutorial-code/chapter5-geometric-verification/src/main.rs
                     (d0 + 24 < d1), of cv-sfm/src/lib.rs (d0 + better_by <= d1, nothing when a side has fewer than two
                     descriptors) and match_descriptors() of akaze/tests/estimate_pose.rs (f32 Lowe ratio).
  best_of_views      register_frame_subset of cv-sfm/src/lib.rs: the HashMap that keeps the best distance of every distinct
                     landmark over the views' neighbour lists, its three best entries and the two better_by rules.  The
                     reference leaves the order of equal distances to its HashMap; the project documents (distance, landmark
                     key), which is what is stated here.
  landmark_pairs     the same function further down: original_matches, landmark_counts / retain, the stable sort by
                     Reverse(summed observation count) and the filter_map on the triangulation.
  hash_bag, hash_knn HammingHasher::hash_bag as the bag-of-words form its type parameters imply (one bit per codeword, set by
                     the features whose nearest codeword it is) and the exact nearest-hash search.

Conventions: descriptors are [n, 64] uint8; neighbour tables are (index, distance) pairs of int64 arrays with -1 for a slot
that does not exist (the caller maps it to the ABI's {2^22 - 1, 1023} or the oracle's 0xFFFFFFFF); NONE = 0xFFFFFFFF is the
absent landmark of a best-of-views row.
"""
from collections import Counter
from functools import lru_cache

import numpy as np

NONE = 0xFFFFFFFF
RULE_STRICT, RULE_BETTER_BY, RULE_LOWE = 0, 1, 2
NB = np.dtype([("index", "<u4"), ("distance", "<u4")])
ABI_ABSENT = ((1 << 22) - 1, 1023)            # include/akz.h, hm_knn
ORACLE_ABSENT = (0xFFFFFFFF, 0xFFFFFFFF)      # oracle/match_oracle.c, orc_knn


# ------------------------------------------------------------------------------------------------ the statement
def _rows(d, width=64):
    return np.ascontiguousarray(d, np.uint8).reshape(-1, width)


def hamming(a, b):
    """Distances of every row of a to every row of b: [na, nb] int64, over all 512 bits."""
    a = _rows(a).view(np.uint64)
    b = _rows(b).view(np.uint64)
    out = np.empty((len(a), len(b)), np.int64)
    for i in range(len(a)):                      # (one query at a time: 2^21 targets stay at 16 MB of popcounts)
        out[i] = np.bitwise_count(a[i][None, :] ^ b).sum(axis=1, dtype=np.int64)
    return out


def knn(q, t, k):
    """(index [nq, k], distance [nq, k]) int64, the first min(k, nt) targets in (distance, index) order, -1 past them."""
    q = _rows(q); t = _rows(t)
    idx = np.full((len(q), k), -1, np.int64)
    dist = np.full((len(q), k), -1, np.int64)
    m = min(k, len(t))
    if m:
        tw = t.view(np.uint64)
        for i, row in enumerate(q.view(np.uint64)):
            d = np.bitwise_count(row[None, :] ^ tw).sum(axis=1, dtype=np.int64)
            order = np.argsort(d, kind="stable")[:m]        # stable: equal distances stay in index order
            idx[i, :m] = order
            dist[i, :m] = d[order]
    return idx, dist


def knn_literal(q, t, k):
    """LinearKnn::knn as the crate writes it, one item at a time (small problems only)."""
    q = _rows(q); t = _rows(t)
    idx = np.full((len(q), k), -1, np.int64)
    dist = np.full((len(q), k), -1, np.int64)
    for i in range(len(q)):
        d = [int(np.unpackbits(q[i] ^ t[j]).sum()) for j in range(len(t))]
        kept = sorted(range(min(k, len(t))), key=lambda j: d[j])            # sort_by_key is stable on the first `num`
        for j in range(k, len(t)):
            pos = 0
            while pos < len(kept) and d[kept[pos]] <= d[j]:                  # partition_point(|n| n.distance <= d)
                pos += 1
            if pos != k:
                kept.pop()
                kept.insert(pos, j)
        idx[i, :len(kept)] = kept
        dist[i, :len(kept)] = [d[j] for j in kept]
    return idx, dist


def as_neighbors(idx, dist, absent):
    """The (index, distance) tables as an NB array with `absent` in the slots that do not exist."""
    out = np.empty(idx.shape, NB)
    out["index"] = np.where(idx < 0, absent[0], idx)
    out["distance"] = np.where(idx < 0, absent[1], dist)
    return out


def accept(rule, d0, d1, pu, pf):
    if rule == RULE_STRICT:
        return d0 + pu < d1
    if rule == RULE_BETTER_BY:
        return d0 + pu <= d1
    return bool(np.float32(d0) < np.float32(d1) * np.float32(pf))


def match(a, b, rule, pu, pf, symmetric):
    """[n, 2] int64 pairs (a, b), ascending a.  Fewer than two descriptors on either side: no pairs."""
    a = _rows(a); b = _rows(b)
    if len(a) < 2 or len(b) < 2:
        return np.zeros((0, 2), np.int64)
    fi, fd = knn(a, b, 2)
    if symmetric:
        ri, rd = knn(b, a, 2)
    pairs = []
    for i in range(len(a)):
        if not accept(rule, int(fd[i, 0]), int(fd[i, 1]), pu, pf):
            continue
        j = int(fi[i, 0])
        if symmetric and not (accept(rule, int(rd[j, 0]), int(rd[j, 1]), pu, pf) and int(ri[j, 0]) == i):
            continue
        pairs.append((i, j))
    return np.array(pairs, np.int64).reshape(-1, 2)


def best_of_views(nb, nq, landmarks, view_sel, counts, better_by):
    """nb [n_views, cap, k] NB: feature i's neighbours in view v (view v of the call is block view_sel[v], which holds
    min(counts[block], cap) features, each observing landmarks[block][feature]).  Returns best [nq, 3, 2] uint32
    {landmark, distance} (NONE, NONE where there is none) and decision [nq] uint32."""
    n_views, cap, k = nb.shape
    best = np.full((nq, 3, 2), NONE, np.uint32)
    decision = np.zeros(nq, np.uint32)
    for i in range(nq):
        seen = {}
        for v in range(n_views):
            blk = int(view_sel[v])
            for j in range(min(k, int(counts[blk]), cap)):
                lm = int(landmarks[blk][int(nb[v, i, j]["index"])])
                d = int(nb[v, i, j]["distance"])
                if lm not in seen or seen[lm] > d:
                    seen[lm] = d
        top = sorted((d, lm) for lm, d in seen.items())[:3]
        for r, (d, lm) in enumerate(top):
            best[i, r] = (lm, d)
        if len(top) == 3:                                    # the reference unwraps three entries
            if top[0][0] + better_by <= top[1][0]:
                decision[i] = 1
            elif top[1][0] + better_by <= top[2][0]:
                decision[i] = 2
    return best, decision


def landmark_pairs(best, decision, merge_ok, world, n_world, merged_base, obs_counts=None):
    """[n, 2] int64 {feature, world row}.  A feature's original match is ([best0], feature) under decision 1 and
    ([best0, best1], feature) under decision 2 when merge_ok[feature] is set (merge_ok None: never); a match survives when
    each of its landmarks is named exactly once over all original matches; it leaves with row best0 (dropped when that is
    no row of the table, >= n_world) or, merged, with row merged_base + feature; a world row with w < 0 is "no
    triangulation" (world None: nothing is dropped for its point).  Feature order, or with obs_counts the stable order of
    descending summed observation count (a key >= n_world counts 0; the sum saturates at 2^32 - 1)."""
    matches = []
    for i in range(len(decision)):
        l0, l1 = int(best[i][0][0]), int(best[i][1][0])
        if l0 == NONE:
            continue
        if int(decision[i]) == 1:
            matches.append(((l0,), i))
        elif int(decision[i]) == 2 and merge_ok is not None and merge_ok[i] and l1 != NONE:
            matches.append(((l0, l1), i))
    named = Counter(l for lms, _ in matches for l in lms)
    matches = [m for m in matches if all(named[l] == 1 for l in m[0])]
    if obs_counts is not None:
        count = lambda l: int(obs_counts[l]) if l < n_world else 0
        matches.sort(key=lambda m: -min(sum(count(l) for l in m[0]), 0xFFFFFFFF))       # list.sort is stable
    out = []
    for lms, i in matches:
        if len(lms) == 2:
            row = merged_base + i
        elif lms[0] >= n_world:
            continue
        else:
            row = lms[0]
        if world is not None and not world[row][3] >= 0.0:
            continue
        out.append((i, row))
    return np.array(out, np.int64).reshape(-1, 2)


def hash_bag(features, codewords):
    """(hash [n_codewords / 8] uint8, word index [n], word distance [n]): bit w (byte w >> 3, position w & 7) is set when w
    is the nearest codeword of some feature, the lowest index among equally near ones."""
    codewords = _rows(codewords)
    assert len(codewords) and len(codewords) % 32 == 0
    idx, dist = knn(features, codewords, 1)
    h = np.zeros(len(codewords) // 8, np.uint8)
    for w in idx[:, 0]:
        h[w >> 3] |= 1 << (w & 7)
    return h, idx[:, 0], dist[:, 0]


def hash_knn(query, hashes, k):
    """(index [m], distance [m]), m = min(k, n): the stored hashes nearest to query in (distance, insertion order)."""
    q = np.ascontiguousarray(query, np.uint8).reshape(-1)
    hs = np.ascontiguousarray(hashes, np.uint8).reshape(-1, len(q))
    d = np.bitwise_count(hs ^ q[None, :]).sum(axis=1, dtype=np.int64)
    order = np.argsort(d, kind="stable")[:min(k, len(hs))]
    return order.astype(np.int64), d[order]


# ------------------------------------------------------------------------------------------------ the catalogue
# Every case is a function of its arguments alone (generators seeded from them).  Rows are arbitrary 64-byte rows: the pad
# bits 486..511 are set as often as any other.

def _rng(*key):
    return np.random.default_rng([0x4D41, *[int(k) & 0xFFFFFFFF for k in key]])


def random_rows(rng, n):
    return rng.integers(0, 256, (n, 64), dtype=np.uint8)


def flip(row, bits):
    """row with the given bit positions flipped (bit b = byte b >> 3, position b & 7)."""
    out = np.array(row, np.uint8, copy=True)
    bits = np.asarray(bits, np.int64)
    np.bitwise_xor.at(out, bits >> 3, (1 << (bits & 7)).astype(np.uint8))
    return out


# where the three nearest of a ladder are planted: one lane's registers (rows 0..3 of a 32-row tile are registers 0..3 of
# half-wave 0, rows 4..7 those of half-wave 1, rows 8..11 registers 4..7 again of half 0, ...), the two half-waves, two
# tiles, the two tiles of a stage | the next stage (64), the ring's revolution (3 stages x 64 = 192), the partial last tile
LADDER_PLACEMENTS = [(0, 1, 2), (2, 3, 8), (3, 4, 9), (11, 16, 27), (28, 31, 32), (62, 63, 64), (64, 191, 192), (190, 193, 255),
                     (256, 384, 512), (510, 511, 512), (512, 0, 257)]


def ladder(seed, lo=0, hi=512, nearest_at=None, far_at=None):
    """One base row and targets at every distance lo..hi from it, exactly once each, in a seeded order; with nearest_at the
    three smallest distances sit at those indices (in that order), with far_at the three largest.  Queries: the base row
    (target i at distance d[i]) and its complement (target i at 512 - d[i]).  Returns dict(q, t, d)."""
    rng = _rng(1, seed, lo, hi)
    base = random_rows(rng, 1)[0]
    d = rng.permutation(np.arange(lo, hi + 1))
    def plant(values, at):
        for v, pos in zip(values, at):
            j = int(np.flatnonzero(d == v)[0])
            d[j], d[pos] = d[pos], d[j]
    if nearest_at is not None:
        plant((lo, lo + 1, lo + 2), nearest_at)
    if far_at is not None:
        plant((hi, hi - 1, hi - 2), far_at)
    t = np.stack([flip(base, rng.permutation(512)[:di]) for di in d])      # 487..512 necessarily reach into the pad bits
    return dict(q=np.stack([base, ~base]), t=t, d=d.astype(np.int64))


def ladder_answer(d, k):
    """The closed form for the ladder's two queries: distinct distances, so the order is the order of d (query 0) and of
    512 - d (query 1)."""
    idx = np.full((2, k), -1, np.int64); dist = np.full((2, k), -1, np.int64)
    m = min(k, len(d))
    for qi, dd in enumerate((d, 512 - d)):
        order = np.argsort(dd, kind="stable")[:m]
        idx[qi, :m] = order; dist[qi, :m] = dd[order]
    return idx, dist


def one_bit_probes(seed):
    """Queries base ^ e_b for every bit b against t[0] = base and t[1 + c] = base ^ e_c ^ e_(c+1 mod 512).  Query b is at
    distance 1 from t[0], t[1 + b] and t[1 + (b - 1) mod 512] and at distance 3 from every other row — if and only if every
    bit weighs exactly 1."""
    base = random_rows(_rng(2, seed), 1)[0]
    q = np.stack([flip(base, [b]) for b in range(512)])
    t = np.stack([base] + [flip(base, [c, (c + 1) % 512]) for c in range(512)])
    return dict(q=q, t=t)


def one_bit_answer(k):
    idx = np.array([sorted((0, 1 + b, 1 + (b - 1) % 512))[:k] for b in range(512)], np.int64)
    return idx, np.ones_like(idx)


TIE_COUNTS = (1, 2, 3, 4, 5, 31, 32, 33, 64, 65, 193, 257)
TIE_BOUNDARIES = (4, 8, 28, 32, 64, 192)         # the pair sits at (b - 1, b): 3|4, 7|8, 27|28, 31|32, 63|64, 191|192


def all_ties(nt, seed=0):
    """nt identical targets; three queries at distance 0, 7 and 512 from them.  The answer is indices 0..min(k, nt) - 1."""
    rng = _rng(3, seed, nt)
    row = random_rows(rng, 1)[0]
    q = np.stack([row, flip(row, rng.permutation(512)[:7]), ~row])
    return dict(q=q, t=np.repeat(row[None], nt, 0), d=np.array([0, 7, 512], np.int64))


def tie_pair_across(boundary, nt=257, seed=0):
    """Distinct random targets, and one row planted twice at indices (boundary - 1, boundary), 5 bits from query 0 and 507
    from query 1 (its complement): nearest pair of the first, farthest of the second."""
    rng = _rng(4, seed, boundary)
    t = random_rows(rng, nt)
    q0 = random_rows(rng, 1)[0]
    t[boundary - 1] = t[boundary] = flip(q0, rng.permutation(512)[:5])
    return dict(q=np.stack([q0, ~q0]), t=t)


def short_extreme(nt, d, seed=0):
    """nt identical targets (fewer than k), each exactly d bits from the one query: slots 0..nt-1 are {i, d}, the rest are
    absent.  d = 512 is the largest real key, right below the sentinel."""
    rng = _rng(5, seed, nt, d)
    q = random_rows(rng, 1)
    row = flip(q[0], rng.permutation(512)[:d]) if d < 512 else ~q[0]
    return dict(q=q, t=np.repeat(row[None], nt, 0))


def far_nearest(variant, nt=33):
    """A query whose nearest neighbour is 512 bits away, with one row in the partial second tile.  Variant 0: every target is
    the query's complement (answer 0, 1, 2 at 512).  Variant 1: rows 0..31 are the complement and row 32 is one bit nearer
    (answer 32 at 511, then 0, 1 at 512)."""
    rng = _rng(6, variant, nt)
    q = random_rows(rng, 1)
    t = np.repeat((~q[0])[None], nt, 0)
    if variant == 1:
        t[nt - 1] = flip(t[nt - 1], [int(rng.integers(0, 512))])
    return dict(q=q, t=t)


LARGEST_NT = (1 << 21) - 1
LARGEST_PLANTS = ((LARGEST_NT - 1, 0), (0, 1), (LARGEST_NT - 2, 1), (1048575, 2))      # (index, distance from query 0)


@lru_cache(maxsize=1)
def largest_target_set():
    """The largest target set hm_create_ex admits: 2^21 - 1 random rows with distance 0, 1, 1, 2 from query 0 planted at
    indices 2^21 - 2, 0, 2^21 - 3 and 1 048 575.  Queries: the base, its complement and two random rows.  Computed once per
    process and shared, with the statement's answer for k = 3 (answers for smaller k are its leading columns)."""
    rng = _rng(7)
    t = rng.integers(0, 256, (LARGEST_NT, 64), dtype=np.uint8)
    base = random_rows(rng, 1)[0]
    for pos, d in LARGEST_PLANTS:
        t[pos] = flip(base, rng.permutation(512)[:d])
    q = np.stack([base, ~base, random_rows(rng, 1)[0], random_rows(rng, 1)[0]])
    t.setflags(write=False); q.setflags(write=False)
    idx, dist = knn(q, t, 3)
    return dict(q=q, t=t, idx=idx, dist=dist)


def aliased_blocks(seed=0, cap=320, n_blocks=3):
    """One descriptor buffer [n_blocks, cap, 64] used as the query AND as the target argument of a batched call, with
    different counts per side: nq = (5, 320, 40), nt = (300, 33, 40).  Rows past both counts of a block hold a pattern that
    must never be read as a descriptor.  Problems pair every block with every block."""
    rng = _rng(8, seed)
    buf = random_rows(rng, n_blocks * cap).reshape(n_blocks, cap, 64)
    nq = np.array([5, 320, 40], np.int32)[:n_blocks]
    nt = np.array([300, 33, 40], np.int32)[:n_blocks]
    buf[0, 7] = buf[0, 2]; buf[0, 250] = buf[0, 2]; buf[1, 30] = buf[0, 2]      # exact hits beyond the shorter count
    for b in range(n_blocks):
        buf[b, max(nq[b], nt[b]):] = 0x5A
    iq = np.repeat(np.arange(n_blocks), n_blocks).astype(np.uint32)
    it = np.tile(np.arange(n_blocks), n_blocks).astype(np.uint32)
    return dict(buf=buf, nq=nq, nt=nt, iq=iq, it=it, cap=cap)


def aliased_codebook(seed=0, cap=96, n_codewords=64):
    """hm_hash_bag_device with the frame block 0 at the codebook's address: [2, cap, 64], frame 0 holds 5 features and its
    first n_codewords rows are the codebook; frame 1 holds 70 features of its own."""
    rng = _rng(9, seed)
    buf = random_rows(rng, 2 * cap).reshape(2, cap, 64)
    buf[1, :20] = buf[0, rng.integers(5, n_codewords, 20)]            # exact hits on codewords beyond frame 0's count
    return dict(buf=buf, counts=np.array([5, 70], np.int32), cap=cap, n_codewords=n_codewords)


PAIR_COUNTS = (1023, 1024, 1025, 2049)


def pairs_case(na, kind, pu=24, seed=0):
    """Rows with scripted nearest and second-nearest distances.  b holds 256 groups {c_g, c_g ^ F_g} (|F_g| = delta_g); a_i is
    c_g(i) with x_i bits flipped outside F_g: d0 = x_i to b[2 g], d1 = x_i + delta_g to b[2 g + 1], every other row ~256 away.
    kind "better_by": delta in {pu - 1, pu, pu + 1} — below, at and above equality of both better-by rules —, the class
    cycling with i (so accepted and rejected alternate inside every wave and every pass of 1 024) except that every fifth
    wave is all-rejected and every seventh all-accepted, and the last row is accepted (na = 1 025: the one row of the second
    pass).  kind "lowe": (d0, d1) cycling through (12, 24) — equality at
    pf = 0.5, rejected —, (11, 24), (12, 25), (13, 24).  kind "twins" (for symmetric matching with pu = 0): the a rows of a
    group come in equal-distance twins, so rev[b] names the lower twin and the higher one must be dropped.
    Returns dict(a, b, d0, d1)."""
    rng = _rng(10, seed, na, pu, {"better_by": 0, "lowe": 1, "twins": 2}[kind])
    G = 256
    if kind == "lowe":
        spec = [((12, 24), (11, 24), (12, 25), (13, 24))[i % 4] for i in range(na)]
    elif kind == "twins":
        spec = [(3 + (i // 2) % 5, 3 + (i // 2) % 5 + 9) for i in range(na)]
    else:
        cls = lambda i: 2 if i == na - 1 else 0 if (i // 64) % 5 == 4 else 2 if (i // 64) % 7 == 3 else i % 3
        spec = [(x, x + pu - 1 + cls(i)) for i, x in enumerate(rng.integers(0, 30, na).tolist())]
    deltas = sorted({d1 - d0 for d0, d1 in spec})
    delta_g = np.array([deltas[g % len(deltas)] for g in range(G)])
    centres = random_rows(rng, G)
    perms = np.stack([rng.permutation(512) for _ in range(G)])
    b = np.empty((2 * G, 64), np.uint8)
    for g in range(G):
        b[2 * g] = centres[g]
        b[2 * g + 1] = flip(centres[g], perms[g, :delta_g[g]])
    a = np.empty((na, 64), np.uint8)
    by_delta = {d: np.flatnonzero(delta_g == d) for d in deltas}
    for i, (d0, d1) in enumerate(spec):
        g = (i // 2) % G if kind == "twins" else int(rng.choice(by_delta[d1 - d0]))    # twins: same group, same distance, other bits
        rest = perms[g, delta_g[g]:]
        a[i] = flip(centres[g], rng.permutation(rest)[:d0])
    return dict(a=a, b=b, d0=np.array([s[0] for s in spec]), d1=np.array([s[1] for s in spec]))


BOV_SCENARIOS = ("again_at_0", "again_at_1", "again_at_2", "again_2_to_0", "again_2_to_1", "again_1_to_0", "again_worse",
                 "equal_keys", "two_landmarks", "one_landmark", "unique_at_equality", "unique_below", "merge_at_equality",
                 "merge_below", "all_equal", "random")


def _bov_script(name, better_by, rng, slots):
    """(landmark, distance) entries of one feature, at most `slots` of them (prefixes stay meaningful: 3 slots is one view)."""
    A, B, C, D = (int(x) for x in rng.choice(5000, 4, replace=False) + 10)
    bb = better_by
    s = {
        "again_at_0": [(A, 50), (B, 100), (C, 150), (A, 40)],
        "again_at_1": [(A, 50), (B, 100), (C, 150), (B, 90)],
        "again_at_2": [(A, 50), (B, 100), (C, 150), (C, 140)],
        "again_2_to_0": [(A, 50), (B, 100), (C, 150), (C, 10)],
        "again_2_to_1": [(A, 50), (B, 100), (C, 150), (D, 160), (C, 60)],
        "again_1_to_0": [(A, 50), (B, 100), (C, 150), (B, 50), (B, 49)],
        "again_worse": [(A, 50), (B, 100), (C, 150), (A, 60), (B, 100), (C, 151)],
        "equal_keys": [(max(A, B, C), 77), (min(A, B, C), 77), (A + B + C - max(A, B, C) - min(A, B, C), 77), (D, 77)],
        "two_landmarks": [(A, 50), (B, 100), (A, 45), (B, 120), (A, 50)],
        "one_landmark": [(A, 50), (A, 40), (A, 60)],
        "unique_at_equality": [(B, 50 + bb), (A, 50), (C, 50 + bb)],
        "unique_below": [(B, 50 + bb - 1), (A, 50), (C, 50 + bb - 1)],
        "merge_at_equality": [(C, 51 + 2 * bb - 1), (A, 50), (B, 50 + bb - 1)],
        "merge_below": [(C, 51 + 2 * bb - 3), (A, 50), (B, 50 + bb - 1)],
        "all_equal": [(A, 9), (B, 9), (C, 9)],
        "random": [(int(rng.integers(0, 12)), int(rng.integers(0, 40))) for _ in range(slots)],
    }[name][:slots]
    if name in ("two_landmarks", "one_landmark", "random"):
        pad = [s[j % len(s)] for j in range(slots - len(s))]                   # repeats: the number of landmarks stays
        pad = [(l, d + 1) for l, d in pad]
    else:
        far = rng.choice(np.arange(6000, 9000), slots, replace=False)          # far landmarks that change no answer
        pad = [(int(l), 300 + int(rng.integers(0, 200))) for l in far[:slots - len(s)]]
    return s + pad


def best_of_views_case(n_views, k=3, nq=300, better_by=24, seed=0):
    """Scripted neighbour lists: feature i plays scenario i mod 16 (BOV_SCENARIOS).  View v of the call is block view_sel[v]
    of a table with two blocks more than views, in a seeded order; every fourth view holds fewer than k features (count 0,
    1 or 2) and its slots past the count carry a distance-0 hit on a fresh landmark that must be ignored — the scripted
    entries skip those slots.  Returns dict(nb, nq, landmarks, view_sel, counts, cap, better_by, names)."""
    rng = _rng(11, seed, n_views, k, better_by)
    n_blocks = n_views + 2
    cap = nq * k
    view_sel = rng.permutation(n_blocks)[:n_views].astype(np.uint32)
    counts = np.full(n_blocks, cap, np.int32)
    if n_views >= 4:
        for v in range(3, n_views, 4):
            counts[view_sel[v]] = (v // 4) % 3
    live = [(v, j) for v in range(n_views) for j in range(min(k, int(counts[view_sel[v]])))]
    nb = np.zeros((n_views, cap, k), NB)
    landmarks = rng.integers(9000, 9500, (n_blocks, cap)).astype(np.uint32)
    names = []
    for i in range(nq):
        name = BOV_SCENARIOS[i % len(BOV_SCENARIOS)]
        names.append(name)
        script = _bov_script(name, better_by, rng, len(live))
        for (v, j), (lm, d) in zip(live, script):          # in the order the views are walked: view, then neighbour
            nb[v, i, j] = (i * k + j, d)
            landmarks[view_sel[v], i * k + j] = lm
        for v in range(n_views):                                               # the poison past a short view's count
            for j in range(min(k, int(counts[view_sel[v]])), k):
                nb[v, i, j] = (i * k + j, 0)
                landmarks[view_sel[v], i * k + j] = 20000 + i
    return dict(nb=nb, nq=nq, landmarks=landmarks, view_sel=view_sel, counts=counts, cap=cap, better_by=better_by, names=names)


LM_SLOTS = 32768
LM_MULT = 2654435761


def lm_slot(key):
    """The landmark set's documented hash (hm_match.hip, lm_slot): the top 15 bits of key * 2654435761 mod 2^32."""
    return ((int(key) * LM_MULT) & 0xFFFFFFFF) >> 17


def keys_of_slot(slot, n, start=0):
    """n distinct keys that hash to `slot`: the multiplier is odd, so key = (slot << 17 | r) / multiplier mod 2^32."""
    inv = pow(LM_MULT, -1, 1 << 32)
    return [(((slot << 17) | r) * inv) & 0xFFFFFFFF for r in range(start, start + n)]


def landmark_case(kind, cap=8192, n_world=20000, seed=0):
    """One frame of best-of-views output for the landmark-pair stage, cap features.
    "full":    every feature a merge (decision 2, merge_ok) and 2 * cap distinct keys — the set at its load factor of one half:
               3 000 keys of slot 32 760 (a probe chain that wraps past the last slot), 1 000 of slot 5, key 0xFFFFFFFE, the rest
               small keys whose slots collide as the hash scatters them; every observation count equal, every world row valid:
               cap survivors, feature order.
    "counts":  the same keys; observation counts in a few values (long runs of ties) and pairs whose sum passes 2^32 - 1
               beside pairs that reach exactly 2^32 - 1; every ninth merged world row invalid.
    "mixed":   decisions 0 / 1 / 2 at random, some masks clear, keys drawn from a small pool so that many are named twice,
               0xFFFFFFFE named twice, absent landmarks, keys beyond n_world.
    Returns dict(best [cap, 3, 2] u32, decision, merge_ok, obs [n_world] u32, world_ok [cap] (validity of the merged rows),
    world_lm [n_world] (validity of the landmark rows), n_world)."""
    rng = _rng(12, seed, cap, {"full": 0, "counts": 1, "mixed": 2}[kind])
    best = np.full((cap, 3, 2), NONE, np.uint32)
    best[:, :, 1] = rng.integers(0, 300, (cap, 3))
    obs = np.zeros(n_world, np.uint32)                 # ("full": the crafted keys lie beyond the table and count 0 — so does every key)
    world_ok = np.ones(cap, bool)
    world_lm = np.ones(n_world, bool)
    if kind in ("full", "counts"):
        crafted = keys_of_slot(32760, 3000) + keys_of_slot(5, 1000) + [0xFFFFFFFE]
        taken = set(crafted)
        small = [x for x in rng.permutation(n_world).tolist() if x not in taken][:2 * cap - len(crafted)]
        keys = np.array(crafted + small, np.uint64)
        assert len(set(keys.tolist())) == 2 * cap
        keys = keys[rng.permutation(2 * cap)]
        best[:, 0, 0] = keys[:cap]; best[:, 1, 0] = keys[cap:]
        best[:, 2, 0] = rng.integers(0, n_world, cap)
        decision = np.full(cap, 2, np.uint32)
        merge_ok = np.ones(cap, np.uint8)
        if kind == "counts":
            obs = rng.choice(np.array([0, 1, 2, 2, 7, 1 << 16, 1 << 31, 0xFFFFFFFF, 0xFFFFFFF0, 0x10, 0xF], np.uint32), n_world)
            world_ok[::9] = False
    else:
        pool = np.array(rng.permutation(n_world + 500)[:cap].tolist() + [0xFFFFFFFE, 0xFFFFFFFE] + keys_of_slot(32767, 40), np.uint64)
        best[:, :, 0] = pool[rng.integers(0, len(pool), (cap, 3))]
        same = best[:, 0, 0] == best[:, 1, 0]
        best[same, 1, 0] = (best[same, 1, 0] + 1) % n_world                     # a feature's landmarks are distinct
        best[rng.random(cap) < 0.02, 0, 0] = NONE
        best[rng.random(cap) < 0.05, 1, 0] = NONE
        decision = rng.integers(0, 3, cap).astype(np.uint32)
        merge_ok = (rng.random(cap) < 0.7).astype(np.uint8)
        obs = rng.integers(0, 6, n_world).astype(np.uint32)
        world_ok = rng.random(cap) < 0.8
        world_lm = rng.random(n_world) < 0.8
    return dict(best=best, decision=decision, merge_ok=merge_ok, obs=obs, world_ok=world_ok, world_lm=world_lm, n_world=n_world)


def landmark_world(case, merged_base, rows):
    """The [rows, 4] f64 world table of a case: w >= 0 where the row is valid, -1 where it is not."""
    world = np.ones((rows, 4), np.float64)
    world[:case["n_world"], 3] = np.where(case["world_lm"], 1.0, -1.0)
    world[merged_base:merged_base + len(case["world_ok"]), 3] = np.where(case["world_ok"], 0.0, -1.0)     # w = 0 is valid
    return world


CODEWORD_COUNTS = (32, 64, 4096, 65536)


def hash_bag_case(n_codewords, n, seed=0):
    """A codebook with its first word repeated in the middle and at the end (ties go to the lowest index) and n features:
    exact hits on the first and the last distinct word, on the repeated word, the rest random."""
    rng = _rng(13, seed, n_codewords, n)
    cw = random_rows(rng, n_codewords)
    cw[n_codewords // 2] = cw[0]
    cw[n_codewords - 1] = cw[0]
    f = random_rows(rng, n)
    picks = [0, n_codewords - 2, n_codewords // 2, 1]
    for i in range(min(n, len(picks))):
        f[i] = cw[picks[i]]
    if n > 8:
        f[8] = flip(cw[n_codewords - 1], [511])                                 # one pad bit from the repeated word
    return dict(features=f, codewords=cw)


HASH_BYTES = (4, 8, 252, 256, 260, 512, 516)
HASH_COUNTS = (1, 3, 4, 5, 257)


def hash_knn_case(hash_bytes, n, kind="random", seed=0):
    """n stored hashes of hash_bytes bytes and a query.  "random": hash 0 repeated at the end (a tie across the whole store),
    the query one bit (the last bit of the last byte) from stored hash n // 2.  "equal": every stored hash the same distance
    from the query — one bit each, a different one where there are enough —, so the answer is insertion order."""
    rng = _rng(14, seed, hash_bytes, n, kind == "equal")
    if kind == "equal":
        q = rng.integers(0, 256, hash_bytes, dtype=np.uint8)
        hs = np.repeat(q[None], n, 0)
        for i in range(n):
            b = (i * 37) % (8 * hash_bytes)
            hs[i, b >> 3] ^= 1 << (b & 7)
        return dict(query=q, hashes=hs)
    hs = rng.integers(0, 256, (n, hash_bytes), dtype=np.uint8)
    hs[n - 1] = hs[0]
    q = hs[n // 2].copy()
    q[hash_bytes - 1] ^= 0x80
    return dict(query=q, hashes=hs)


# ------------------------------------------------------------------------------------------------ the k-NN catalogue as a list
def _closed(idx_rows, dist_rows, k, known=None):
    """Rows of (index, distance) lists -> ([nq, k] idx, [nq, k] dist, [nq, k] mask): -1 where the slot does not exist; mask is
    False where the closed form does not name the entry (the statement alone decides there)."""
    nq = len(idx_rows)
    idx = np.full((nq, k), -1, np.int64); dist = np.full((nq, k), -1, np.int64); mask = np.ones((nq, k), bool)
    for i in range(nq):
        m = min(k, len(idx_rows[i]))
        idx[i, :m] = idx_rows[i][:m]; dist[i, :m] = dist_rows[i][:m]
        if known is not None:
            mask[i, known[i]:] = False
    return idx, dist, mask


def knn_cases():
    """Every designed k-NN input but the largest: (name, q, t, closed) with closed(k) -> (idx, dist, mask), the answer known
    without any search."""
    out = []
    for n, at in enumerate(LADDER_PLACEMENTS):
        c = ladder(n, nearest_at=at, far_at=tuple(reversed([(p + 100) % 513 for p in at])))
        out.append((f"ladder 0..512, nearest at {at}", c["q"], c["t"],
                    lambda k, d=c["d"]: ladder_answer(d, k) + (np.ones((2, k), bool),)))
    for n, at in enumerate(((0, 1, 2), (3, 4, 32), (31, 64, 112), (96, 97, 111))):
        c = ladder(100 + n, lo=400, nearest_at=at)
        out.append((f"ladder 400..512, nearest at {at}", c["q"][:1], c["t"],
                    lambda k, d=c["d"]: tuple(x[:1] for x in ladder_answer(d, k)) + (np.ones((1, k), bool),)))
    c = one_bit_probes(0)
    out.append(("one-bit probes", c["q"], c["t"], lambda k: one_bit_answer(k) + (np.ones((512, k), bool),)))
    for nt in TIE_COUNTS:
        c = all_ties(nt)
        out.append((f"{nt} identical targets", c["q"], c["t"],
                    lambda k, nt=nt, d=c["d"]: _closed([list(range(nt))] * 3, [[int(x)] * nt for x in d], k)))
    for b in TIE_BOUNDARIES:
        c = tie_pair_across(b)
        # query 0: the pair first; query 1 (the complement): nothing known in closed form
        out.append((f"identical pair at {b - 1}|{b}", c["q"], c["t"],
                    lambda k, b=b: _closed([[b - 1, b, -1], [-1, -1, -1]], [[5, 5, -1], [-1, -1, -1]], k, known=[2, 0])))
    for nt in (1, 2):
        for d in (486, 512):
            c = short_extreme(nt, d)
            out.append((f"{nt} target(s) at distance {d}", c["q"], c["t"],
                        lambda k, nt=nt, d=d: _closed([list(range(nt))], [[d] * nt], k)))
    c = far_nearest(0)
    out.append(("33 targets, all at 512", c["q"], c["t"], lambda k: _closed([[0, 1, 2]], [[512] * 3], k)))
    c = far_nearest(1)
    out.append(("33 targets, the last at 511, the rest at 512", c["q"], c["t"], lambda k: _closed([[32, 0, 1]], [[511, 512, 512]], k)))
    return out


def check_neighbors(got, idx, dist, absent, what, mask=None):
    """got (an NB array) equals (idx, dist) with `absent` in the slots that do not exist — every entry, or those of mask."""
    want = as_neighbors(idx, dist, absent)
    mask = np.ones(idx.shape, bool) if mask is None else mask
    for f in ("index", "distance"):
        bad = np.argwhere((np.asarray(got[f]) != want[f]) & mask)
        assert len(bad) == 0, (f"{what}: {f} differs in {len(bad)} entries; first at {tuple(bad[0])}: "
                               f"{got[f][tuple(bad[0])]} != {want[f][tuple(bad[0])]}")
