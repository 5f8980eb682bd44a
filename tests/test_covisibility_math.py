"""include/akz_covisibility_math.h through its host build (tests/cpp/covisibility_host.c) against the independent statement
(tests/covisibility_statement.py): equal in every output word, on random tables and on hand-made ones that each catch one way
of getting the search wrong.  No GPU."""
import numpy as np
import pytest

import covisibility_checker as K
import covisibility_statement as S


def both(table, targets, p):
    """host build and statement on one call; asserts they agree in every word -> (host outputs, statement result)"""
    s = S.candidates(table["start"], table["obs"], table["reason"], targets, table["n_blocks"], table["cap"], p)
    o = K.candidates(table, targets, p)
    K.equals_statement(o, s, p)
    return o, s


def grouped(groups, n_blocks, target=0, reason=None):
    """groups: [(views, n)]: n landmarks each seen by `target` and by `views`; every view's features are dealt in order"""
    used = [0] * n_blocks
    lists = []
    for views, n in groups:
        for _ in range(n):
            row = []
            for v in (target,) + tuple(views):
                row.append((v, used[v]))
                used[v] += 1
            lists.append(row)
    return K.make_table(lists, n_blocks, max(used) + 3, reason)


SMALL = dict(min_cov=1, min_lm=1, min_new=1)


def emitted_views(o, n):
    return [tuple(r) for r in o["views"][:n].tolist()]


def test_any_stops_inserting_at_the_first_new_view():
    # sorted triples: (0,1,2) 5, (0,1,3) 4, (0,2,3) 3, (0,1,4) 2.  With the short-circuit the walk inserts 0, 1, 2, 4: all four are
    # unique and keep the sorted order.  Inserting all three views makes (0,2,3) a repeat that drops behind (0,1,4).
    tab = grouped([((1, 2), 5), ((1, 3), 4), ((2, 3), 3), ((1, 4), 2)], 5)
    o, s = both(tab, [0], S.settings(limit=8, **SMALL))
    assert emitted_views(o, 5) == [(0, 1, 2), (0, 1, 3), (0, 2, 3), (0, 1, 4), (0, 0, 0)]
    assert o["stats"][0, K.S_UNIQUE] == 4 and o["stats"][0, K.S_EMITTED] == 4
    assert o["slot_count"][:5].tolist() == [5, 4, 3, 2, 0]


def test_a_triple_between_the_two_minimums_takes_a_unique_slot_and_is_not_emitted():
    # defaults: 16 <= 20 < 24
    tab = K.star_table(3, [30, 20, 30], 30, 40)
    o, s = both(tab, [0], S.settings())
    assert o["stats"][0].tolist() == [30, 3, 3, 3, 1, 0, 0, 0]
    assert emitted_views(o, 2) == [(0, 1, 3), (0, 0, 0)] and o["slot_count"][0] == 30
    assert o["lm_start"][:3].tolist() == [0, 30, 30]
    assert [len(b) for _, b in s["detail"][0]["triples"]] == [30, 20, 20] and s["detail"][0]["unique"] == [0, 1, 2]


def test_repeats_pad_the_chain_once_the_unique_triples_run_out():
    tab = grouped([((1, 2, 3, 4), 6)], 5)
    o, s = both(tab, [0], S.settings(limit=8, **SMALL))
    # (0,2,4) is the one triple that brings no new view; it comes last
    assert emitted_views(o, 6) == [(0, 1, 2), (0, 1, 3), (0, 1, 4), (0, 2, 3), (0, 3, 4), (0, 2, 4)]
    assert o["stats"][0, K.S_UNIQUE] == 5 and o["stats"][0, K.S_EMITTED] == 6 and o["stats"][0, K.S_FLAGS] == 0
    # take(maximum) stops the walk: with two unique slots the rest follows in sorted order
    o, s = both(tab, [0], S.settings(max_constraints=2, limit=8, **SMALL))
    assert emitted_views(o, 6) == [(0, 1, 2), (0, 1, 3), (0, 1, 4), (0, 2, 3), (0, 2, 4), (0, 3, 4)]
    assert o["stats"][0, K.S_UNIQUE] == 2


def test_a_limit_below_the_chain_says_so():
    tab = grouped([((1, 2, 3, 4), 6)], 5)
    o, s = both(tab, [0], S.settings(limit=3, **SMALL))
    assert o["stats"][0, K.S_EMITTED] == 3 and o["stats"][0, K.S_FLAGS] == K.F_LIMIT
    assert emitted_views(o, 3) == [(0, 1, 2), (0, 1, 3), (0, 1, 4)]
    o, s = both(tab, [0], S.settings(limit=6, **SMALL))
    assert o["stats"][0, K.S_EMITTED] == 6 and o["stats"][0, K.S_FLAGS] == 0


def test_equal_counts_keep_the_lexicographic_order_of_the_pairs():
    # target 2 in the middle of its triples: the canonical order sorts it in; (0,1), (0,3), (1,3) all count 4
    tab = grouped([((0, 1, 3), 4)], 4, target=2)
    o, s = both(tab, [2], S.settings(limit=4, **SMALL))
    assert emitted_views(o, 4) == [(0, 1, 2), (0, 2, 3), (1, 2, 3), (0, 0, 0)]
    # a larger count goes first whatever its place among the pairs
    tab = grouped([((0, 1, 3), 4), ((1, 3), 1)], 4, target=2)
    o, s = both(tab, [2], S.settings(limit=4, **SMALL))
    assert emitted_views(o, 3) == [(1, 2, 3), (0, 1, 2), (0, 2, 3)]


def test_equal_observation_counts_are_ordered_by_position_or_by_the_seeded_mix():
    tab = grouped([((1, 2), 9), ((1, 2, 3), 2)], 4)          # nine landmarks of three observations, then two of four
    p = S.settings(limit=1, max_lm=6, **SMALL)
    o, s = both(tab, [0], p)
    assert emitted_views(o, 1) == [(0, 1, 2)] and o["slot_count"][0] == 11
    assert o["lm"][:6, 0].tolist() == [9, 10, 0, 1, 2, 3]       # the longer lists first, then feature order
    seed = 12345
    o, s = both(tab, [0], S.settings(limit=1, max_lm=6, seed=seed, **SMALL))
    tail = sorted(range(9), key=lambda l: (S.mix(seed, l), l))
    head = sorted((9, 10), key=lambda l: (S.mix(seed, l), l))
    assert o["lm"][:6, 0].tolist() == head + tail[:4] and tail != list(range(9))
    for l in (0, 1, 77, 2 ** 31 + 5):
        assert K.lib().cv_mix(seed, l) == S.mix(seed, l)
    # the key: count, then mix, then position; counts beyond 19 bits compare equal
    key = K.lib().cv_list_key
    assert key(5, 0, 3, 1) < key(4, 0, 3, 0) and key(4, 0, 3, 0) < key(4, 0, 9, 1)
    assert key(1 << 19, 0, 0, 0) == key((1 << 19) - 1, 0, 0, 0)


def test_a_landmark_observed_twice_in_a_view_counts_once_and_gives_its_first_feature():
    lists = [[(0, k), (1, 10 + k), (1, 20 + k), (2, k)] for k in range(3)]
    tab = K.make_table(lists, 3, 32)
    o, s = both(tab, [0], S.settings(limit=1, **SMALL))
    assert o["slot_count"][0] == 3 and o["stats"][0, K.S_CANDIDATES] == 2
    assert o["lm"][:3].tolist() == [[0, 10, 0], [1, 11, 1], [2, 12, 2]]
    # its observation count is 3 views, not 4 entries: landmark 3 with four views sorts in front of the three above
    tab = K.make_table(lists + [[(0, 3), (1, 13), (2, 3), (3, 0)]], 4, 32)
    o, s = both(tab, [0], S.settings(limit=1, **SMALL))
    assert o["lm"][:4, 0].tolist() == [3, 0, 1, 2]
    tab = K.make_table(lists, 3, 32)
    # a minimum of 4 would be met only by counting view 1 twice
    o, s = both(tab, [0], S.settings(limit=1, min_cov=4, min_lm=1))
    assert o["stats"][0].tolist() == [3, 0, 0, 0, 0, 0, 0, 0]


def test_a_target_without_a_robust_landmark_emits_nothing():
    tab = grouped([((1, 2), 5)], 3, reason=[2] * 5)
    o, s = both(tab, [0, 1], S.settings(limit=2, **SMALL))
    assert o["verdict"][:2].tolist() == [K.OK, K.OK] and not o["stats"][:2].any()
    assert not o["views"][:4].any() and o["lm_start"].tolist() == [0] * 5


def test_more_candidates_than_the_cap_keeps_the_largest_counts_ties_to_the_lower_block():
    n = K.MAX_CANDIDATE_VIEWS + 6
    per = [2 + (k % 3) for k in range(n)]                     # counts 2, 3, 4 in turn: the cut falls among the 2s
    tab = K.star_table(n, per, 4, 8)
    o, s = both(tab, [0], S.settings(limit=K.MAX_SLOTS, max_constraints=K.MAX_SLOTS, **SMALL))
    assert o["stats"][0, K.S_CANDIDATES] == K.MAX_CANDIDATE_VIEWS and o["stats"][0, K.S_FLAGS] & K.F_CAPPED
    twos = [k + 1 for k in range(n) if per[k] == 2]
    dropped = set(twos[-6:])
    seen = set(o["views"].reshape(-1).tolist())
    assert not (seen & dropped) and set(twos[:-6]) <= seen
    # exactly the cap: nothing is cut
    tab = K.star_table(K.MAX_CANDIDATE_VIEWS, 2, 4, 8)
    o, s = both(tab, [0], S.settings(limit=4, **SMALL))
    assert o["stats"][0, K.S_CANDIDATES] == K.MAX_CANDIDATE_VIEWS and not o["stats"][0, K.S_FLAGS] & K.F_CAPPED


def test_bad_indices_refuse_the_targets_that_see_them_and_a_broken_start_array_everyone():
    tab = grouped([((1, 2), 5)], 3)
    tab["obs"][2] = (7, 0)                                    # landmark 0 names block 7: every target that sees it is refused
    p = S.settings(limit=2, **SMALL)
    o, s = both(tab, [0, 9, 1], p)
    assert o["verdict"][:3].tolist() == [K.BAD_INDEX, K.BAD_INDEX, K.BAD_INDEX]
    tab = grouped([((1, 2), 5)], 4)
    tab["obs"][2] = (7, 0)
    o, s = both(tab, [0, 3, 2], p)                            # view 3 sees nothing, view 2 no longer sees the bad landmark
    assert o["verdict"][:3].tolist() == [K.BAD_INDEX, K.OK, K.OK]
    tab = grouped([((1, 2), 5)], 3)
    tab["start"][2] = 40                                      # a start beyond n_obs: the table is broken for everyone
    o, s = both(tab, [0, 1], p)
    assert o["verdict"][:2].tolist() == [K.BAD_INDEX, K.BAD_INDEX] and not o["lm_start"].any()


def test_the_record_rule_at_both_of_its_inequalities():
    p = S.settings(limit=6, min_new=4, max_constraints=5)
    st = K.settings(p)

    def one(verdicts, views):
        v = np.array(verdicts, np.uint32)
        rec, n = np.zeros(6, np.uint32), np.zeros(1, np.uint32)
        out = K.lib().cv_record_one(v.ctypes.data, st, views, rec.ctypes.data, n.ctypes.data)
        srec, sver, sn = S.record(verdicts, [0], [S.OK], [0, views], p)
        assert rec.tolist() == srec and [out] == sver and [int(n[0])] == sn
        return out, int(n[0]), rec.tolist()

    three = [0, 1, 0, 2, 0, 1]
    assert one(three, 5) == (K.FEW_CONSTRAINTS, 0, [16, 1, 16, 2, 16, 1])      # 3 < 4 and 3 + 1 < 5
    assert one(three, 4) == (K.OK, 3, three)                                    # 3 + 1 < 4 fails: recorded
    assert one([0, 0, 0, 2, 0, 1], 50) == (K.OK, 4, [0, 0, 0, 2, 0, 1])         # 4 < 4 fails
    assert one([0] * 6, 50) == (K.OK, 5, [0, 0, 0, 0, 0, 16])                   # take(5)
    # the whole call: ranges of the graphs, a target outside every range, a refused target passing through
    targets, gs = [0, 5, 9, 2], [0, 3, 8]
    cv = np.array(three + [0] * 6 + [0] * 6 + [1, 0, 0, 0, 0, 3], np.uint32)
    tv, stats = [K.OK, K.OK, K.OK, K.BAD_INDEX], np.full((4, 8), 7, np.uint32)
    rec, ver, stats2 = K.record(cv, targets, tv, stats, gs, p)
    srec, sver, sn = S.record(cv, targets, tv, gs, p)
    assert rec.tolist() == srec and ver.tolist() == sver == [K.OK, K.OK, K.NO_GRAPH, K.BAD_INDEX]
    assert stats2[:, K.S_RECORDED].tolist() == sn == [3, 5, 0, 0] and (np.delete(stats2, K.S_RECORDED, 1) == 7).all()
    assert rec[18:].tolist() == [1, 16, 16, 16, 16, 3]


def test_rows_are_flatten():
    from cv_amd.pose_graph import flatten
    rng = np.random.default_rng(5)
    for n, n_views in ((0, 4), (1, 3), (40, 9), (300, 17)):
        views = np.sort(np.stack([rng.permutation(n_views)[:3] for _ in range(n)]).reshape(-1, 3), 1).astype(np.uint32) if n else np.zeros((0, 3), np.uint32)
        if n > 2:
            views[1] = 0                                      # an unused slot: all six entries in view 0's row
        rs, re, flag = K.rows(views, n_views)
        fs, fe = flatten(views, n_views)
        assert flag == 0 and rs.tolist() == fs.tolist() and re.tolist() == fe.tolist()
        ss, se, sf = S.rows(views.tolist(), n_views)
        assert (ss, se, sf) == (rs.tolist(), re.tolist(), 0)
    views = np.array([[0, 1, 2], [1, 2, 9], [0, 2, 3]], np.uint32)
    rs, re, flag = K.rows(views, 4)
    fs, fe = flatten(views[[0, 2]], 4)
    assert flag == 1 and rs.tolist() == fs.tolist()
    assert re.tolist() == [e if e < 6 else e + 6 for e in fe.tolist()] + [0] * 6
    assert S.rows(views.tolist(), 4) == (rs.tolist(), re[:12].tolist(), 1)


def test_pairs_are_lexicographic():
    ab = np.zeros(2, np.uint32)
    for n in (2, 3, 5, 127, 128):
        want = [(a, b) for a in range(n) for b in range(a + 1, n)]
        for q in list(range(min(len(want), 300))) + [len(want) - 1]:
            K.lib().cv_pair_from_index(q, n, ab.ctypes.data)
            assert tuple(ab.tolist()) == want[q]


RANDOM = [(seed, kw) for seed in (0, 1, 2) for kw in (dict(limit=8), dict(limit=3, seed=77), dict(max_constraints=2, limit=6), dict())]
_seen = dict(full=0, fewer=0, dropped=0, padded=0)


@pytest.mark.parametrize("seed,kw", RANDOM)
def test_random_tables(seed, kw):
    tab = K.random_table(seed)
    p = S.settings(**kw)
    o, s = both(tab, list(range(12)) + [3, 99], p)
    for d, st in zip(s["detail"], s["stats"]):
        _seen["full"] += st[4] == p["limit"]
        _seen["fewer"] += 0 < st[4] < p["limit"]
        _seen["dropped"] += sum(len(b) < p["min_lm"] for _, b in d["triples"])
        _seen["padded"] += sum(i not in d["unique"] for i in d["emitted"])


def test_the_random_tables_were_not_vacuous():
    if not any(_seen.values()):
        for seed, kw in RANDOM:
            test_random_tables(seed, kw)
    assert all(_seen.values()), _seen
