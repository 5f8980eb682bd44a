"""The decisions of include/akz_view_plan_math.h — the text the view-plan kernels compile — built with the host compiler
(tests/cpp/view_plan_host.c through host_build.load) and held to tests/view_plan_statement.py, the reference's text in plain
Python, on the whole catalogue.  The find's outputs the host build reads are place_statement's, laid out as the ABI lays them out,
with a fill wherever a find does not write: a refused query's rows are never read.  Integers only: every comparison is exact.
No GPU needed."""
import ctypes as C

import numpy as np
import pytest

import host_build
import place_statement as P
import view_plan_statement as S

FILL = 0xA5A5A5A5
CASES = S.cases()


@pytest.fixture(scope="module")
def host():
    L = host_build.load("view_plan_host.c")
    L.vp_plan.argtypes = [C.c_void_p] * 5 + [C.c_uint32, C.c_void_p] + [C.c_uint32] * 5 + [C.c_void_p] * 4
    for name in ("vp_group_by_ordinal", "vp_taken", "vp_list_verdict", "vp_call_verdict"):
        getattr(L, name).restype = C.c_uint32
    L.vp_group_by_ordinal.argtypes = [C.c_int, C.c_uint32, C.c_uint32]
    L.vp_taken.argtypes = L.vp_list_verdict.argtypes = L.vp_call_verdict.argtypes = [C.c_uint32, C.c_uint32]
    L.vp_group_span.restype = C.c_uint32
    L.vp_group_span.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]
    L.vp_live.argtypes = [C.c_uint32] * 5
    return L


def host_outputs(L, c, pitch=None):
    find = P.outputs(c["table"], c["queries"], c["visible"], c["params"], pitch=pitch, fill=FILL, search=False)
    room = P.room(c["params"]) if pitch is None else pitch
    F, V = len(c["queries"]), c["V"]
    o = dict(view_idx=np.full((F, V), FILL, np.uint32), n_views=np.full(F, FILL, np.uint32), verdict=np.full(F, FILL, np.uint32),
             counts=np.full(S.COUNTS, FILL, np.uint32))
    at = lambda a: a.ctypes.data
    pick = c["pick"]
    assert L.vp_plan(at(find["views_out"]), at(find["group_recon"]), at(find["group_start"]), at(find["counts"]), at(find["verdict"]), room,
                     None if pick is None else at(pick), S.PICK_RECON if c["by_recon"] else 0, F, V, c["n_blocks"], c["exp_blocks"],
                     at(o["view_idx"]), at(o["n_views"]), at(o["verdict"]), at(o["counts"])) == 0
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
    same(host_outputs(host, c), S.outputs(c, fill=FILL), name)
    if name in ("growing", "three_first", "refusals"):                 # a wider pitch of the find's rows
        same(host_outputs(host, c, pitch=P.room(c["params"]) + 5), S.outputs(c, fill=FILL), name)


def test_the_catalogue_holds_what_it_is_designed_for():
    r = {name: S.outputs(c) for name, c in CASES.items()}
    verdicts = set(int(v) for o in r.values() for v in o["verdict"])
    assert verdicts == {S.OK, S.CUT, S.NO_GROUP, S.FIND_REFUSED, S.BAD_VIEW}            # every frame verdict
    calls = {name: int(o["counts"][S.C_VERDICT]) for name, o in r.items()}
    assert set(calls.values()) == {S.OK, S.NO_ROOM}                                     # every call verdict
    # both sides of exp_blocks: the count equal to it, and one above
    assert r["room_exact"]["counts"].tolist() == [5, 7, S.OK, 3] and CASES["room_exact"]["exp_blocks"] == 5
    assert r["room_short"]["counts"].tolist() == [5, 0, S.NO_ROOM, 0] and CASES["room_short"]["exp_blocks"] == 4
    assert (r["room_short"]["view_idx"] == S.NONE).all() and (r["room_short"]["n_views"] == 0).all() and (r["room_short"]["verdict"] == S.OK).all()
    # a pick beyond n_groups, a key no group has
    assert r["three_turn_3"]["verdict"].tolist() == [S.NO_GROUP] and r["three_key_77"]["verdict"].tolist() == [S.NO_GROUP]
    assert r["three_turn_2"]["n_views"].tolist() == [2] and r["three_key_30"]["view_idx"].tolist() == r["three_turn_2"]["view_idx"].tolist()
    assert r["three_first"]["view_idx"].tolist() == r["three_key_5"]["view_idx"].tolist() != r["three_key_9"]["view_idx"].tolist()
    assert r["free"]["verdict"].tolist() == [S.NO_GROUP]
    # a group of exactly V, V - 1 and V + 1 views
    assert r["lengths"]["verdict"].tolist() == [S.OK, S.OK, S.CUT, S.OK] and r["lengths"]["n_views"].tolist() == [4, 3, 4, 1]
    # a key equal to n_blocks - 1 is a block, one equal to n_blocks is none; behind the cut it is not looked at
    assert r["last_block"]["verdict"].tolist() == [S.OK, S.BAD_VIEW, S.OK, S.BAD_VIEW, S.CUT] and r["last_block"]["view_idx"][0].tolist() == [3, 39, S.NONE]
    assert r["last_block"]["counts"].tolist() == [6, 6, S.OK, 3]
    # every frame naming the same views: the distinct count is the group's length
    assert r["same_views"]["counts"].tolist() == [3, 15, S.OK, 5]
    assert r["refusals"]["verdict"].tolist().count(S.FIND_REFUSED) == 4
    assert [len(CASES[f"frames_{F}"]["queries"]) for F in (1, 63, 64, 65)] == [1, 63, 64, 65]
    assert r["two_groups_each"]["view_idx"][:, :3].tolist() == [[2, 4, S.NONE], [5, S.NONE, S.NONE], [S.NONE] * 3]
    assert S.CUT in r["growing"]["verdict"] and S.NO_GROUP in r["growing"]["verdict"] and S.OK in r["growing"]["verdict"]


def test_the_pieces(host):
    NONE = S.NONE
    assert host.vp_group_by_ordinal(0, 9, 3) == 0 and host.vp_group_by_ordinal(1, 2, 3) == 2 and host.vp_group_by_ordinal(1, 3, 3) == NONE
    assert host.vp_group_by_ordinal(0, 0, 0) == NONE
    assert (host.vp_taken(3, 4), host.vp_taken(4, 4), host.vp_taken(5, 4)) == (3, 4, 4)
    assert (host.vp_list_verdict(3, 4), host.vp_list_verdict(4, 4), host.vp_list_verdict(5, 4)) == (S.OK, S.OK, S.CUT)
    assert (host.vp_call_verdict(5, 5), host.vp_call_verdict(6, 5), host.vp_call_verdict(0, 1)) == (S.OK, S.NO_ROOM, S.OK)
    start = C.c_uint32(99)
    assert host.vp_group_span(2, 6, 10, C.byref(start)) == 4 and start.value == 2
    assert host.vp_group_span(8, 14, 10, C.byref(start)) == 2 and start.value == 8           # held inside the row
    assert host.vp_group_span(7, 3, 10, C.byref(start)) == 0 and host.vp_group_span(NONE, NONE, 10, C.byref(start)) == 0 and start.value == 10
    assert host.vp_live(0, 1, 4, 7, 8) == 1 and host.vp_live(1, 1, 4, 7, 8) == 0 and host.vp_live(0, 1, 4, 8, 8) == 0
    assert host.vp_live(4, 9, 4, 0, 8) == 0 and host.vp_live(3, 9, 4, 0, 8) == 1             # a count above n_views is n_views
