"""The landmark bookkeeping of include/akz_landmark_table_math.h, host build (tests/landmark_table_checker.py), against the
independent statement in dicts and lists (tests/landmark_table_statement.py): add_view / merge_landmarks /
are_landmarks_sharing_view written from the reference's text, and the rule for several frames of one call on top.  For one
frame the statement's sequential add_view is the expectation, with no rule of ours involved.  No GPU."""
import numpy as np
import pytest

import landmark_table_checker as K
import landmark_table_statement as S


def run(inp):
    o = K.add_views(inp)
    st = K.check_against_statement(inp, o)
    if st["call_verdict"] == S.OK:
        assert K.one_observation_per_view(st["rows"])
    return o, st


small_table, designed = K.small_table, K.designed


@pytest.mark.parametrize("name", sorted(K.designed_cases()))
def test_designed_calls(name):
    o, st = run(K.designed_cases()[name])
    if name.startswith("bad:") or name.startswith("a row below n_world"):
        assert st["frame_verdict"] == [S.OK, S.BAD_INDEX, S.OK]
    if name.startswith("starts that") or name.startswith("a last start"):
        assert st["call_verdict"] == S.BAD_TABLE


def test_the_rule_functions():
    L = K.lib()
    assert L.lt_merge_applied(1, 1) == 1
    for a, b in ((2, 1), (1, 2), (0, 1), (3, 3)):
        assert L.lt_merge_applied(a, b) == 0
    obs = np.array([[0, 9], [1, 9], [2, 9], [3, 9], [2, 8]], np.uint32)
    assert L.lt_lists_share(obs.ctypes.data, 0, 2, 2, 4) == 0
    assert L.lt_lists_share(obs.ctypes.data, 0, 3, 3, 5) == 1           # the last element of each only
    assert L.lt_lists_share(obs.ctypes.data, 0, 0, 0, 5) == 0           # an empty list shares nothing


def test_one_frame_is_the_references_add_view():
    """matches to landmarks, a merge, features without a match: the sequential statement is the expectation"""
    slots = [K.slot(5, 6, [(4, 3), (1, 6 + 0 * 8 + 1), (0, 2)])]
    inp = designed(slots, best={(0, 1): (0, 1)}, n_blocks=6)
    o, st = run(inp)
    seq, rec = S.sequential(inp)
    assert K.rows(o) == seq == st["rows"]
    assert seq[0] == [(0, 0), (1, 0), (2, 0), (3, 0), (5, 1)] and seq[1] == []            # a's list, b's list, the new observation; a tombstone
    assert seq[2][-1] == (5, 0) and seq[3] == [(1, 1), (5, 4)]
    assert seq[6:] == [[(5, 2)], [(5, 3)], [(5, 5)]]                                      # add_landmark in feature order
    assert [int(v) for v in o["counts_out"]] == [9, 15, 1, 0]
    # the views' landmark lists are the inverse map
    for view, feats in rec.views.items():
        for feature, key in feats.items():
            assert o["landmarks_out"][view, feature] == key


@pytest.mark.parametrize("seed", range(12))
def test_one_random_frame_is_the_references_add_view(seed):
    inp = K.random_call(seed, n_frames=1, merges=3, split=seed % 3)
    inp["verdict"][:] = 0
    inp["skip"] = None
    o, st = run(inp)
    seq, _ = S.sequential(inp)
    assert K.rows(o) == seq
    assert st["counts"][3] == 0                                                            # one frame: nothing is ever demoted


@pytest.mark.parametrize("seed", range(16))
def test_random_batches(seed):
    inp = K.random_call(100 + seed, n_landmarks=30 + 7 * seed, n_frames=1 + seed % 5, cap=128, collide=seed % 2 == 0, bad_slots=seed % 4 == 3,
                        split=seed % 4, extra_room=seed % 3)
    o, st = run(inp)
    if seed % 2:                                     # no landmark named twice: the frames commute and the reference applies one by one
        assert K.rows(o) == S.sequential(inp)[0]


def test_two_and_three_frames_on_one_landmark_keep_slot_order():
    slots = [K.slot(7, 2, [(1, 2)]), K.slot(5, 3, [(0, 2), (2, 0)]), K.slot(6, 1, [(0, 2)])]
    o, st = run(designed(slots))
    assert K.rows(o)[2] == [(0, 1), (2, 1), (3, 1), (7, 1), (5, 0), (6, 0)]                # ik is not ascending: slot order, not block order
    assert K.rows(o)[0] == [(0, 0), (1, 0), (5, 2)]


def test_demotions():
    # slot 0 merges (0, 1); slot 1 names 1: demoted, the observation goes to 0 alone and 1 keeps its list
    slots = [K.slot(4, 2, [(0, 6 + 0)]), K.slot(5, 2, [(1, 1)])]
    o, st = run(designed(slots, best={(0, 0): (0, 1)}))
    r = K.rows(o)
    assert r[0] == [(0, 0), (1, 0), (4, 0)] and r[1] == [(2, 0), (3, 0), (5, 1)]
    assert st["counts"][2:] == [0, 1] and st["stats"][0][1:3] == [0, 1]
    # two merges chained through landmark 3: (5, 3) and (3, 4) — both demoted
    slots = [K.slot(4, 2, [(0, 6 + 0)]), K.slot(5, 2, [(1, 6 + 8 + 1)])]
    o, st = run(designed(slots, best={(0, 0): (5, 3), (1, 1): (3, 4)}))
    r = K.rows(o)
    assert st["counts"][2:] == [0, 2]
    assert r[5] == [(3, 2), (4, 0)] and r[3] == [(1, 1), (5, 1)] and r[4] == []
    # two merges that touch nothing in common are both applied
    slots = [K.slot(4, 2, [(0, 6 + 0)]), K.slot(5, 2, [(1, 6 + 8 + 1)])]
    o, st = run(designed(slots, best={(0, 0): (5, 3), (1, 1): (1, 0)}))
    assert st["counts"][2:] == [2, 0] and K.rows(o)[1] == [(2, 0), (3, 0), (0, 0), (1, 0), (5, 1)] and K.rows(o)[0] == []


def test_refused_and_skipped_slots_contribute_nothing():
    good = lambda block, lm: K.slot(block, 3, [(1, lm)])
    base, _ = run(designed([good(4, 0), good(6, 2)]))
    cases = [K.slot(5, 2, [(0, 6)]),                                   # a landmark >= n_landmarks
             K.slot(5, 2, [(2, 1)]),                                   # a feature >= count
             K.slot(5, 2, [(0, 6 + 0 * 8 + 0)]),                       # the merged row of another slot
             K.slot(5, 2, [(0, 1), (0, 3)]),                           # a feature in two final matches
             K.slot(5, 9, [(0, 1)]),                                   # a count above the capacity
             K.slot(5, 2, [(0, 1)], nmatches=9)]                       # a match count above the capacity
    for bad in cases:
        o, st = run(designed([good(4, 0), bad, good(6, 2)], best={(1, 0): (0, 1)}))
        assert st["frame_verdict"] == [S.OK, S.BAD_INDEX, S.OK]
        assert K.rows(o) == K.rows(base) and np.array_equal(o["landmarks_out"], base["landmarks_out"])
        assert np.all(o["poses"][5] == -1.0) and np.all(o["stats"][1] == 0)
    # a merged row without d_best
    o, st = run(designed([good(4, 0), K.slot(5, 2, [(0, 6 + 8 + 0)]), good(6, 2)]))
    assert st["frame_verdict"] == [S.OK, S.BAD_INDEX, S.OK] and K.rows(o) == K.rows(base)
    # a verdict that is not RS_SV_OK, and a skip word: not accepted, whatever the matches say
    for s in (K.slot(5, 2, [(0, 99)], verdict=K.SV_FEW_ROBUST), K.slot(5, 2, [(0, 1)], skip=1)):
        o, st = run(designed([good(4, 0), s, good(6, 2)]))
        assert st["frame_verdict"] == [S.OK, S.NOT_ACCEPTED, S.OK] and K.rows(o) == K.rows(base)
    # a match that is not final is no match: its feature gets a landmark of its own
    o, st = run(designed([K.slot(4, 2, [(0, 99), (1, 2)], final=[0, 1])]))
    assert st["frame_verdict"] == [S.OK] and K.rows(o)[6:] == [[(4, 0)]]


def test_split_list_and_empty_calls():
    start, obs, n_obs = K.table(small_table(), pad=1)
    # no frames: the split rows alone; a count above the room is cut to the room
    inp = K.inputs(start, obs, n_obs, 8, 4, [], split=[(0, 5), (1, 5), (2, 5)], split_count=7, split_room=3)
    o, st = run(inp)
    assert K.rows(o)[6:] == [[(0, 5)], [(1, 5)], [(2, 5)]] and st["counts"][0] == 9
    inp = K.inputs(start, obs, n_obs, 8, 4, [], split=[(0, 5), (1, 5), (2, 5)], split_count=1, split_room=3)
    o, st = run(inp)
    assert st["counts"][:2] == [7, 10] and o["landmarks_out"][1, 5] == K.NONE
    # an empty table, nothing to add
    start, obs, n_obs = K.table([], pad=0)
    o, st = run(K.inputs(start, obs, n_obs, 4, 2, []))
    assert st["counts"] == [0, 0, 0, 0] and list(o["start_out"]) == [0]
    # an empty table and a frame of `cap` features and one of none
    o, st = run(K.inputs(start, obs, n_obs, 4, 2, [K.slot(1, 4), K.slot(0, 0)]))
    assert K.rows(o) == [[(1, 0)], [(1, 1)], [(1, 2)], [(1, 3)]] and st["frame_verdict"] == [S.OK, S.OK]


def test_a_table_whose_starts_do_not_ascend_refuses_the_call():
    start, obs, n_obs = K.table(small_table(), pad=2)
    for broken in (np.array([0, 2, 1, 7, 8, 8, 9], np.uint32), np.array([0, 2, 4, 7, 8, 8, 12], np.uint32)):
        inp = K.inputs(broken, obs, n_obs, 8, 8, [K.slot(4, 2, [(0, 1)])], split=[(0, 5)])
        o, st = run(inp)
        assert st["call_verdict"] == S.BAD_TABLE and st["frame_verdict"] == [S.NOT_ACCEPTED]
        assert np.all(o["start_out"] == 0) and np.all(o["obs_counts_out"] == 0) and np.all(o["landmarks_out"] == K.NONE)
        assert np.all(o["obs_out"] == K.FILL32) and np.all(o["poses"] == -1.0)
    # a start array that begins above 0 still ascends: the observations in front of it belong to nobody
    inp = K.inputs(np.array([1, 2, 4, 7, 8, 8, 9], np.uint32), obs, n_obs, 8, 8, [])
    o, st = run(inp)
    assert st["call_verdict"] == S.OK and K.rows(o)[0] == [(1, 0)]


def test_a_feature_listed_twice_gets_its_lowest_key():
    lists = [[(0, 0)], [(1, 1), (0, 0)], [(0, 0), (2, 0)]]
    o, st = run(designed([], lists=lists, n_blocks=3))
    assert o["landmarks_out"][0, 0] == 0 and o["landmarks_out"][1, 1] == 1 and o["landmarks_out"][2, 0] == 2
    # an observation outside the blocks or the capacity is copied and maps nothing
    o, st = run(designed([], lists=[[(9, 0), (0, 99), (1, 1)]], n_blocks=3))
    assert K.rows(o)[0] == [(9, 0), (0, 99), (1, 1)] and (o["landmarks_out"] != K.NONE).sum() == 1


def test_the_mask_is_are_landmarks_sharing_view():
    lists = K.mask_lists()
    start, obs, n_obs, best, decision = K.mask_case(lists, K.MASK_PAIRS, K.MASK_DECISIONS)
    mask = K.sharing_view(start, obs, n_obs, best, decision)
    want = S.sharing_mask(lists, best, decision, len(lists))
    assert mask.tolist() == want and want[0] == K.MASK_WANT
    # the fill below n_obs: a table whose last start lies above n_obs is cut there, and a list that crosses the cut is no list
    start, obs, _, best, decision = K.mask_case(lists, K.MASK_PAIRS, K.MASK_DECISIONS, pad=0)
    cut = int(start[7]) + 3                                  # inside landmark 7
    mask = K.sharing_view(start, obs, cut, best, decision)
    cut_lists = [l if start[k + 1] <= cut else None for k, l in enumerate(lists)]
    assert mask.tolist() == S.sharing_mask(cut_lists, best, decision, len(lists))
    assert mask[0, 9] == 1 and mask[0, 10] == 0 and mask[0, 12] == 0
