"""The decisions of the two steps that start a reconstruction (include/akz_bootstrap_table_math.h), on the host:
  1. the host build of the header (tests/bootstrap_table_checker.py) is held to the independent statement
     (tests/bootstrap_table_statement.py) in every byte of every output on designed inputs;
  2. the statement's join is held to cv_amd.three_view.join_pairs with the permutation the key rule gives;
  3. three deliberately broken rules are shown to be caught.
No GPU needed."""
import numpy as np
import pytest

import bootstrap_table_checker as ck
import bootstrap_table_statement as st
from cv_amd.three_view import join_pairs
from landmark_table_checker import table

CAP = 16


def held_join(inp):
    host, stated = ck.join(inp), st.join(inp, ck.join_outputs(inp))
    assert ck.same(host, stated, ck.JOIN_OUTPUT_NAMES) == []
    return host


def held_add(inp):
    host, stated = ck.add(inp), st.add_reconstruction(inp, ck.add_outputs(inp))
    assert ck.same(host, stated, ck.ADD_OUTPUT_NAMES) == []
    return host


# ---- 1. the host build against the statement ----
def test_join_of_empty_lists_and_of_refused_scenes():
    slots = [ck.slot([]), ck.slot([(1, 2), (3, 4)]), ck.slot([(1, 5)], best_id=ck.NONE), ck.slot([(1, 2)], inliers=[1]),
             ck.slot([(1, CAP)]), ck.slot([(CAP, 1)]), ck.slot([(1, 2)], npairs=CAP + 1), ck.slot([(1, 2)], n_inliers=CAP + 1)]
    scenes = [(0, 0), (0, 1), (1, 0), (1, 2), (2, 1), (1, 3), (4, 1), (1, 5), (6, 1), (1, 7), (1, 1)]
    o = held_join(ck.join_inputs(slots, scenes, CAP))
    assert o["verdict"].tolist() == [0, 0, 0, 1, 1, 3, 3, 3, 3, 3, 0]
    assert o["ntriples"].tolist() == [0] * 10 + [2] and o["nfirst"].tolist() == [0, 0, 2] + [0] * 8 and o["nsecond"][1] == 2
    assert (o["triples"][3] == ck.FILL32).all()                           # a refused scene's lists are not written
    o = held_join(ck.join_inputs(slots, scenes, CAP, minimum=2))
    assert o["verdict"].tolist() == [2, 2, 2, 1, 1, 2, 2, 2, 3, 3, 0]       # a count above the capacity comes before the minimum
    assert (o["pose_first"][3] == ck.join_inputs(slots, scenes, CAP)["pose"][1]).all()   # the poses are gathered whatever the verdict


def test_a_centre_feature_twice_keeps_its_last_entry():
    first = ck.slot([(3, 0), (5, 1), (3, 2), (7, 3), (5, 4)])
    second = ck.slot([(5, 10), (9, 11), (5, 12), (3, 13), (8, 14)], inliers=[0, 1, 2, 3])
    o = held_join(ck.join_inputs([first, second], [(0, 1), (1, 0)], CAP))
    # triples follow the first list, duplicates included; the second feature is the LAST entry of the second list
    assert o["triples"][0, :4].tolist() == [[3, 0, 13], [5, 1, 12], [3, 2, 13], [5, 4, 12]] and o["ntriples"][0] == 4
    assert o["first_only"][0, :1].tolist() == [[7, 3]] and o["second_only"][0, :1].tolist() == [[9, 11]]
    assert o["triples"][1, :3].tolist() == [[5, 10, 4], [5, 12, 4], [3, 13, 2]]


@pytest.mark.parametrize("shuffle", [False, True])
def test_drawn_joins(shuffle):
    rng = np.random.default_rng(11)
    slots = [ck.drawn_slot(rng, CAP, n, k, centres=c) for n, k, c in ((16, 16, 16), (16, 9, 7), (12, 12, 5), (1, 1, 16), (16, 0, 16))]
    scenes = [(a, b) for a in range(5) for b in range(5)]
    held_join(ck.join_inputs(slots, scenes, CAP, shuffle=shuffle, seed=0xDEADBEEFCAFEF00D))


def designed_scenes():
    full = ck.scene((0, 1, 2), (6, 5, 7), [(0, 1, 2), (2, 0, 6), (4, 4, 0)], [1, 0, 1], [(1, 2), (3, 3)], [1, 0], [(5, 3)], [1])
    return full


def test_a_rejected_triple_gives_its_centre_feature_neither_observation():
    o = held_add(ck.add_inputs([designed_scenes()], CAP, 3, 4, 1))
    assert o["frame_verdict"][0] == ck.AR_OK and o["stats"][0].tolist() == [2, 1, 1, 6 + (5 - 3) + (7 - 3)]
    start, obs = o["obs_start_out"], o["obs_out"]
    row = lambda r: obs[start[r]:start[r + 1]].tolist()
    assert row(0) == [[1, 0], [2, 1], [3, 2]] and row(2) == [[1, 2]]        # triple (2, 0, 6) was rejected by its mask
    assert row(1) == [[1, 1], [2, 2]] and row(3) == [[1, 3]] and row(4) == [[1, 4], [2, 4], [3, 0]] and row(5) == [[1, 5], [3, 3]]
    # features in no match: the first frame's 0 and 3, then the second frame's 1, 4, 5, 6
    assert [row(r) for r in range(6, 12)] == [[[2, 0]], [[2, 3]], [[3, 1]], [[3, 4]], [[3, 5]], [[3, 6]]]
    assert o["counts_out"].tolist() == [12, 18, 1, 1] and (start[12:] == 18).all()
    assert o["landmarks_out"][2, :5].tolist() == [6, 0, 1, 7, 4] and (o["landmarks_out"][0] == ck.NONE).all()
    assert o["recon_start_out"].tolist() == [0, 12] and o["view_start_out"].tolist() == [1, 4]
    assert (o["kps_dst"][0] == ck.FILL8).all() and o["counts_dst"][1:].tolist() == [6, 5, 7]


def test_empty_lists_and_no_scene():
    held_add(ck.add_inputs([], CAP, 3, 4, 0))
    o = held_add(ck.add_inputs([ck.scene((2, 0, 1), (3, 0, 2))], CAP, 3, 3, 0))
    assert o["counts_out"].tolist() == [5, 5, 1, 1]


@pytest.mark.parametrize("broken", ["centre", "first", "second", "centre_across_lists", "range", "count", "same_block"])
def test_a_refused_scene_is_refused_alone(broken):
    good = ck.scene((3, 4, 5), (4, 4, 4), [(0, 0, 0)])
    bad = dict(centre=ck.scene((0, 1, 2), (4, 4, 4), [(1, 0, 0), (1, 2, 3)]),
               first=ck.scene((0, 1, 2), (4, 4, 4), [(1, 2, 0)], None, [(0, 2)]),
               second=ck.scene((0, 1, 2), (4, 4, 4), [(1, 2, 3)], None, (), None, [(0, 3)]),
               centre_across_lists=ck.scene((0, 1, 2), (4, 4, 4), (), None, [(1, 0)], None, [(1, 0)]),
               range=ck.scene((0, 1, 2), (4, 4, 4), [(1, 4, 0)]),
               count=ck.scene((0, 1, 2), (4, CAP + 1, 4)),
               same_block=ck.scene((0, 1, 0), (4, 4, 4)))[broken]
    o = held_add(ck.add_inputs([bad, good], CAP, 6, 6, 0))
    assert o["frame_verdict"].tolist() == [ck.AR_BAD_INDEX, ck.AR_OK] and o["recon_start_out"].tolist() == [0, 0, 10]
    assert o["constraint_verdict_out"].tolist() == [16, 0]
    # a duplicate that its mask rejects is no duplicate
    if broken == "centre":
        bad["masks"][0] = [1, 0]
        assert held_add(ck.add_inputs([bad, good], CAP, 6, 6, 0))["frame_verdict"].tolist() == [ck.AR_OK, ck.AR_OK]


def test_taken_skipped_and_not_ok_scenes():
    rng = np.random.default_rng(3)
    scenes = [ck.drawn_scene(rng, (0, 1, 2), (9, 8, 7), CAP, (3, 2, 2)),
              ck.drawn_scene(rng, (0, 3, 4), (9, 6, 6), CAP, (2, 1, 1)),                           # shares the centre: TAKEN
              ck.drawn_scene(rng, (5, 6, 7), (5, 5, 5), CAP, (2, 1, 1), skip=1),
              ck.drawn_scene(rng, (5, 6, 7), (5, 5, 5), CAP, (2, 1, 1), verdict=ck.TV_FEW_ROBUST),
              ck.drawn_scene(rng, (7, 3, 5), (5, 6, 5), CAP, (2, 1, 1)),                           # the skipped ones took nothing
              ck.drawn_scene(rng, (6, 4, 2), (5, 6, 7), CAP, (2, 1, 1))]                           # block 2 is the first scene's
    o = held_add(ck.add_inputs(scenes, CAP, 8, 20, 2, extra_room=5))
    assert o["frame_verdict"].tolist() == [ck.AR_OK, ck.AR_TAKEN, ck.AR_NOT_ACCEPTED, ck.AR_NOT_ACCEPTED, ck.AR_OK, ck.AR_TAKEN]
    assert o["counts_out"][3] == 2 and o["view_start_out"].tolist() == [2, 5, 8, 11, 14, 17, 20]


def old_table():
    return table([[(0, 1), (1, 1)], [], [(0, 0), (1, 2), (2, 0)], [(2, 5)]], pad=3)


def test_an_existing_table_in_front():
    scenes = [designed_scenes()]
    inp = ck.add_inputs(scenes, CAP, 3, 7, 3, table=old_table(), recon_start=[0, 2, 4], view_start=[0, 2, 3])
    o = held_add(inp)
    assert o["call_verdict"][0] == ck.AR_OK and o["counts_out"].tolist() == [16, 24, 3, 1]
    assert o["obs_start_out"][:5].tolist() == [0, 2, 2, 5, 6] and o["recon_start_out"].tolist() == [0, 2, 4, 16]
    assert o["view_start_out"].tolist() == [0, 2, 3, 6] and o["landmarks_out"][1, :3].tolist() == [ck.NONE, 0, 2]
    assert o["landmarks_out"][3, 0] == 4 and o["obs_counts_out"][:5].tolist() == [2, 0, 3, 1, 3]
    # without the ranges the table is taken as it is
    held_add(ck.add_inputs(scenes, CAP, 3, 7, 3, table=old_table()))


@pytest.mark.parametrize("what", ["starts", "end", "recon", "recon_end", "views", "view_end"])
def test_bad_table(what):
    start, obs, n_obs = old_table()
    recon, views = [0, 2, 4], [0, 2, 3]
    if what == "starts":
        start = start.copy()
        start[1], start[2] = 5, 2
    elif what == "end":
        n_obs = 5
    elif what == "recon":
        recon = [0, 3, 2, 4]
        views = [0, 1, 2, 3]
    elif what == "recon_end":
        recon = [0, 2, 3]
    elif what == "views":
        views = [2, 0, 3]
    else:
        views = [0, 2, 4]
    o = held_add(ck.add_inputs([designed_scenes()], CAP, 3, 7, 3, table=(start, obs, n_obs), recon_start=recon, view_start=views))
    assert o["call_verdict"][0] == ck.AR_BAD_TABLE and o["frame_verdict"][0] == ck.AR_NOT_ACCEPTED
    assert o["counts_out"].tolist() == [4, n_obs, len(recon), 0] and (o["landmarks_out"] == ck.NONE).all()
    assert (o["obs_start_out"][:5] == start).all() and (o["obs_out"][:n_obs] == obs[:n_obs]).all() and (o["poses"] == ck.FILL64).all()


def test_drawn_calls():
    rng = np.random.default_rng(5)
    for n_scenes in (1, 2, 5):
        scenes = []
        for s in range(n_scenes):
            counts = tuple(int(c) for c in rng.integers(6, CAP + 1, 3))
            lists = tuple(int(v) for v in rng.integers(0, 3, 3))
            scenes.append(ck.drawn_scene(rng, (3 * s + 1, 3 * s, 3 * s + 2), counts, CAP, lists, keep=0.7))
        held_add(ck.add_inputs(scenes, CAP, 3 * n_scenes, 3 * n_scenes + 4, 4, table=old_table(), recon_start=[0, 4], view_start=[0, 4], extra_room=3))


# ---- 2. the statement's join against join_pairs ----
def test_the_statements_join_is_join_pairs():
    rng = np.random.default_rng(17)
    for trial in range(20):
        n1, n2 = int(rng.integers(0, 40)), int(rng.integers(0, 40))
        first = list(zip(rng.integers(0, 24, n1).tolist(), rng.integers(0, 99, n1).tolist()))
        second = list(zip(rng.integers(0, 24, n2).tolist(), rng.integers(0, 99, n2).tolist()))
        triples, first_only, second_only = st.join_lists(first, second)
        perm = st.shuffle_permutation(1234567 + trial, trial, len(triples))
        t, f, g = join_pairs(first, second, permutation=perm)
        assert t.tolist() == [list(triples[j]) for j in perm]
        assert f.tolist() == [list(p) for p in first_only] and g.tolist() == [list(p) for p in second_only]
        assert join_pairs(first, second)[0].tolist() == [list(p) for p in triples]


def test_the_key_rule_is_the_consensus_stages():
    """RS_BATCH_SHUFFLE's keys as the consensus stage's own statement gives them, and as the header computes them"""
    import consensus_statement
    seed = 0x0123456789ABCDEF
    for s in (0, 1, 7):
        keys = st.shuffle_keys(seed, s, 50)
        assert keys == consensus_statement.shuffle_keys(consensus_statement.scene_seed(seed, s), 50)
        assert keys == [ck.lib().bt_shuffle_key(seed, s, j) for j in range(50)]
        assert st.shuffle_permutation(seed, s, 50) == consensus_statement.shuffle_order(consensus_statement.scene_seed(seed, s), 50).tolist()


# ---- 3. broken rules are caught ----
def test_first_wins_is_caught():
    first = ck.slot([(3, 0), (5, 1)])
    second = ck.slot([(5, 10), (5, 12), (3, 13)])
    inp = ck.join_inputs([first, second], [(0, 1)], CAP)
    host = ck.join(inp)
    lists = [st.gathered(inp["pairs"][k], int(inp["npairs"][k]), inp["inliers"][k], int(inp["n_inliers"][k]), CAP) for k in (0, 1)]
    assert host["triples"][0, :2].tolist() == [list(t) for t in st.join_lists(*lists)[0]]
    assert host["triples"][0, :2].tolist() != [list(t) for t in st.join_lists(*lists, last_wins=False)[0]]


def test_the_second_views_rows_before_the_firsts_is_caught():
    inp = ck.add_inputs([designed_scenes()], CAP, 3, 4, 1)
    host = ck.add(inp)
    assert ck.same(host, st.add_reconstruction(inp, ck.add_outputs(inp)), ck.ADD_OUTPUT_NAMES) == []
    differs = ck.same(host, st.add_reconstruction(inp, ck.add_outputs(inp), second_before_first=True), ck.ADD_OUTPUT_NAMES)
    assert "obs_out" in differs and "landmarks_out" in differs


def test_an_unstable_tie_order_is_caught():
    keys = np.array([5, 1, 5, 1, 0x01000005, 5, 0xFFFFFFFF, 1, 0], np.uint32)
    order = np.zeros(len(keys), np.uint32)
    ck.lib().bt_stable_order(keys.ctypes.data, len(keys), order.ctypes.data)
    assert order.tolist() == st.order_of(keys.tolist()) == [8, 1, 3, 7, 0, 2, 5, 4, 6]
    assert order.tolist() != st.order_of(keys.tolist(), stable=False)
