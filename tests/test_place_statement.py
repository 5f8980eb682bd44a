"""The decisions of include/akz_place_math.h — the text the place-recognition kernels compile — built with the host compiler
(tests/cpp/place_host.c through host_build.load) and held to tests/place_statement.py, the reference's function line by line, on
the whole catalogue; and the statement held to a literal replay of the reference's sequence.  Integers only: every comparison is
exact, and the entries a call does not write must still hold the fill.  No GPU needed."""
import ctypes as C

import numpy as np
import pytest

import host_build
import place_statement as S

FILL = 0xA5A5A5A5
CASES = S.cases()
ARRAYS = ("found", "views_out", "group_recon", "group_start", "free", "search", "counts", "verdict")


@pytest.fixture(scope="module")
def host():
    L = host_build.load("place_host.c")
    L.pl_find.argtypes = [C.c_void_p] * 5 + [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p] + [C.c_uint32] * 6 + [C.c_void_p] * 8
    L.pl_room.restype = C.c_uint32
    L.pl_room.argtypes = [C.c_uint32, C.c_uint32]
    L.pl_window_slot.argtypes = [C.c_uint32] * 5 + [C.POINTER(C.c_uint32)]
    L.pl_similar_keeps.argtypes = [C.c_uint32] * 8
    L.pl_threshold.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.pl_key.restype = L.pl_group_key.restype = C.c_uint64
    L.pl_key.argtypes = L.pl_group_key.argtypes = [C.c_uint32, C.c_uint32]
    return L


def host_outputs(L, c, pitch=None, search=True):
    t, p, q, vis = c["table"], c["params"], c["queries"], c["visible"]
    o = S.outputs(t, q[:0], None, p, pitch=pitch, fill=FILL, search=search)             # the shapes
    R = S.room(p) if pitch is None else pitch
    o = {k: np.full((len(q),) + a.shape[1:], FILL, np.uint32) for k, a in o.items()}
    ptr = lambda a: a.ctypes.data if a.size else None
    keep = [np.zeros(1, np.uint32)]
    at = lambda a: a.ctypes.data if a.size else keep[0].ctypes.data                     # an empty array still has an address
    assert L.pl_find(at(t["hashes"]), at(t["feed"]), at(t["pos"]), at(t["recon"]), at(t["view"]), len(t["feed"]), t["hashes"].shape[1], at(q),
                     None if vis is None else at(vis), len(q), p["num_similar"], p["num_recent"], p["recent_threshold"], p["search_num"], R,
                     at(o["found"]), at(o["views_out"]), at(o["group_recon"]), at(o["group_start"]), at(o["free"]),
                     ptr(o["search"]) if search else None, at(o["counts"]), at(o["verdict"])) == 0
    return o


def same(got, want, what):
    assert set(got) == set(want)
    for k in want:
        assert got[k].shape == want[k].shape, (what, k)
        bad = np.argwhere(got[k] != want[k])
        assert len(bad) == 0, (what, k, bad[:4].tolist(), got[k][tuple(bad[0])], want[k][tuple(bad[0])])


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_host_build_is_the_statement(host, name):
    c = CASES[name]
    want = S.outputs(c["table"], c["queries"], c["visible"], c["params"], fill=FILL)
    same(host_outputs(host, c), want, name)
    if name in ("growing", "groups_three", "refusals"):               # a wider pitch, and without the search lists
        pitch = S.room(c["params"]) + 5
        same(host_outputs(host, c, pitch=pitch, search=False), S.outputs(c["table"], c["queries"], c["visible"], c["params"], pitch=pitch, fill=FILL, search=False), name)


def test_the_catalogue_holds_what_it_is_designed_for():
    r = lambda name, k=0: S.find_one(CASES[name]["table"], int(CASES[name]["queries"][k]), len(CASES[name]["table"]["feed"]), CASES[name]["params"])
    # the block of equal distances straddles the cut, and its rows are not in row order in the table's neighbourhood
    t = r("ties_at_the_cut")
    assert list(t["search"][1][-3:]) == [5, 5, 5] and sorted(t["search"][0][-3:]) == list(t["search"][0][-3:])
    c = CASES["ties_at_the_cut"]
    d = np.bitwise_count(c["table"]["hashes"] ^ c["table"]["hashes"][c["queries"][0]]).sum(axis=1)
    assert (d == 5).sum() == 6 and set(np.flatnonzero(d == 5)[:3]) == set(t["search"][0][-3:])
    # the query is not in its own list
    t = r("query_outside_its_own_list")
    assert 7 not in t["search"][0] and list(t["search"][1]) == [0, 0, 0, 0]
    # both ends of the feed clip the window
    assert len(r("window_clipped", 0)["recent"]) == 31 and len(r("window_clipped", 1)["recent"]) == 31 and len(r("window_clipped", 2)["recent"]) == 39
    assert r("num_recent_0")["recent"] == [] and r("num_recent_1")["recent"] == [] and len(r("num_recent_256", 1)["recent"]) == 510
    # a near frame that is recent is dropped and does not use up the take
    t = r("near_and_recent")
    assert set(t["search"][0][1:7]) == set(t["recent"]) and len(t["similar"]) == 3 and not set(t["similar"]) & set(t["recent"])
    # the threshold drops the query's feed only
    t, c = r("recent_threshold"), CASES["recent_threshold"]
    feed, pos = c["table"]["feed"], c["table"]["pos"]
    assert all(feed[s] != feed[20] or abs(int(pos[s]) - int(pos[20])) >= 10 for s in t["similar"])
    assert any(feed[s] != feed[20] and abs(int(pos[s]) - int(pos[20])) < 10 for s in t["similar"])
    # the groups
    assert r("groups_free")["groups"] == [] and [(k, len(v)) for k, v in r("groups_three")["groups"]] == [(5, 4), (9, 4), (30, 2)]
    assert CASES["groups_own"]["table"]["recon"][12] == 9
    # the widest case reaches every limit
    t = r("widest", 1)
    assert len(t["search"][0]) == 2048 and len(t["recent"]) == 510 and len(t["similar"]) >= 2048 - 510 - 1
    assert [S.find_one(CASES["refusals"]["table"], int(q), int(v), CASES["refusals"]["params"])["verdict"]
            for q, v in zip(CASES["refusals"]["queries"], CASES["refusals"]["visible"])] == [S.OK, S.BAD_INDEX, S.BAD_INDEX, S.OK, S.BAD_INDEX, S.BAD_TABLE]


def test_visible_query_plus_one_is_the_growing_table():
    """the statement with visible = query + 1 over the whole table == one query at a time over the table so far"""
    for name, kw in (("growing", {}), ("growing", dict(num_recent=0)), ("growing", dict(num_similar=0, search_num=3))):
        c = S.growing_case(**kw)
        literal = S.replay(c["table"], c["params"])
        n = len(c["table"]["feed"])
        for k in range(n):
            batched = S.find_one(c["table"], k, k + 1, c["params"])
            assert batched["verdict"] == literal[k]["verdict"] == S.OK
            for key in ("recent", "similar", "groups", "free"):
                assert batched[key] == literal[k][key], (kw, k, key)
            assert all(np.array_equal(a, b) for a, b in zip(batched["search"], literal[k]["search"]))
        # and a later frame changes an earlier frame's answer once it is visible
        assert any(S.find_one(c["table"], k, n, c["params"])["recent"] != literal[k]["recent"] for k in range(n)) or c["params"]["num_recent"] == 0


def test_the_pieces(host):
    assert host.pl_room(0, 32) == 62 == S.room(S.params()) and host.pl_room(8, 0) == 8 and host.pl_room(2048, 256) == 2558 and host.pl_room(3, 1) == 3
    slot = C.c_uint32(99)
    assert host.pl_window_slot(1, 10, 1, 12, 4, C.byref(slot)) == 1 and slot.value == 1
    assert host.pl_window_slot(1, 15, 1, 12, 4, C.byref(slot)) == 1 and slot.value == 6
    assert host.pl_window_slot(1, 12, 1, 12, 4, C.byref(slot)) == 1 and slot.value == 3            # the query's own slot
    assert host.pl_window_slot(1, 16, 1, 12, 4, C.byref(slot)) == 0 and host.pl_window_slot(2, 12, 1, 12, 4, C.byref(slot)) == 0
    assert host.pl_window_slot(1, 0xFFFFFFFF, 1, 0, 4, C.byref(slot)) == 0 and host.pl_window_slot(1, 12, 1, 12, 0, C.byref(slot)) == 0
    assert host.pl_similar_keeps(5, 1, 10, 5, 1, 10, 0, 0) == 0                                    # the query itself
    assert host.pl_similar_keeps(6, 1, 13, 5, 1, 10, 4, 0) == 0 and host.pl_similar_keeps(6, 1, 14, 5, 1, 10, 4, 0) == 1
    assert host.pl_similar_keeps(6, 1, 14, 5, 1, 10, 4, 5) == 0 and host.pl_similar_keeps(6, 2, 14, 5, 1, 10, 4, 5) == 1
    hist = np.array([0, 3, 0, 2, 5], np.uint32)
    t, quota = C.c_uint32(), C.c_uint32()
    for wanted, want in ((1, (1, 1)), (3, (1, 3)), (4, (3, 1)), (5, (3, 2)), (6, (4, 1)), (10, (4, 5))):
        assert host.pl_threshold(hist.ctypes.data, 5, wanted, C.byref(t), C.byref(quota)) == 1 and (t.value, quota.value) == want
    assert host.pl_threshold(hist.ctypes.data, 5, 11, C.byref(t), C.byref(quota)) == 0
    assert host.pl_key(3, 9) < host.pl_key(4, 0) and host.pl_key(3, 9) > host.pl_key(3, 8)
    assert host.pl_group_key(4, 9) < host.pl_group_key(3, 1) and host.pl_group_key(4, 5) < host.pl_group_key(4, 9)
