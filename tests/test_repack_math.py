"""include/akz_repack_math.h in its host build (tests/cpp/repack_host.c) against the statement of the reference's remove_view
(tests/repack_statement.py) over the designed tables of tests/repack_catalogue.py: every output word.  No GPU needed; the
device is held to the same host build in tests/test_gpu_repack.py."""
import math

import numpy as np
import pytest

import repack_catalogue as cat
import repack_statement as stmt

CASES = cat.table_cases()
BY_NAME = {c.name: c for c in CASES}


@pytest.fixture(scope="module")
def host():
    return {c.name: cat.host_table(c) for c in CASES}


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_host_build_is_the_statement_or_the_specified_refusal(case, host):
    got = host[case.name]
    assert int(got["call_verdict"][0]) == case.expect
    if case.expect == cat.NO_ROOM:
        rows, observations = cat.kept_counts(case)
        lens = case.start[1:].astype(np.int64) - case.start[:-1]
        empty = int(np.count_nonzero(lens == 0))
        counts = (rows, observations, empty, case.n_landmarks - rows - empty, int(lens.sum()) - observations)
        assert rows > case.lm_room or observations > case.obs_room
        assert cat.same(got, cat.refused_table(case, cat.NO_ROOM, counts)) is None
    elif case.expect != cat.OK:
        assert cat.same(got, cat.refused_table(case, case.expect)) is None
    elif case.statement:
        assert cat.same(got, cat.statement_table(case)) is None


def test_the_catalogue_holds_what_it_names():
    """the shapes the kernels can go wrong at are in the tables, not only in their names"""
    big = BY_NAME["rows_2049"]
    lens = set((big.start[1:] - big.start[:-1]).tolist())
    assert {0, 1, 63, 64, 65, 129} <= lens
    assert sorted(c.n_landmarks for c in CASES if c.name.startswith("rows_")) == [0, 1, 1023, 1024, 1025, 2049]
    key = lambda name: cat.host_table(BY_NAME[name])["key_out"]
    k = key("drop_first_of_tile")
    assert k[0] == cat.NONE and k[cat.TILE] == cat.NONE and k[2 * cat.TILE] == cat.NONE and k[1] == 0
    k = key("drop_last_of_tile")
    assert k[cat.TILE - 1] == cat.NONE and k[2 * cat.TILE - 1] == cat.NONE and k[cat.TILE] != cat.NONE
    k = key("drop_whole_tile")
    assert np.all(k[cat.TILE:2 * cat.TILE] == cat.NONE) and k[2 * cat.TILE] != cat.NONE and k[cat.TILE - 2] != cat.NONE
    assert np.all(key("drop_every_row") == cat.NONE)
    assert np.array_equal(key("drop_no_row_identity"), np.arange(2 * cat.TILE + 1))
    # a wide row that keeps a part: 129 observations, those in live views stay
    o = cat.host_table(big)
    live = sum(1 for i in range(129) if (6 + i) % cat.BIG_BLOCKS < cat.BIG_LIVE)
    assert 64 < live < 129 and int(o["obs_counts_out"][o["key_out"][6]]) == live
    # three ranges: one loses every row, one is empty
    r = cat.host_table(BY_NAME["ranges_three"])["recon_start_out"]
    assert r[0] == 0 and r[1] == 0 and r[2] == 0 and r[3] > 0


def test_a_feature_in_two_rows_gets_its_lowest_key():
    case = BY_NAME["feature_in_two_rows"]
    o = cat.host_table(case)
    assert int(o["call_verdict"][0]) == cat.OK
    m = case.list_map()
    for row in (0, 1):
        blk, feat = case.obs[case.start[row]]
        assert o["landmarks_out"][m[blk], feat] == o["key_out"][row] == row
    assert o["key_out"][40] != cat.NONE and o["key_out"][41] != cat.NONE          # the second listings are rows all the same


def test_a_dropped_observation_may_name_any_feature():
    """only a KEPT feature >= cap is a bad index: a removed view's observations are never placed"""
    o = cat.host_table(BY_NAME["dropped_feature_is_cap"])
    ref = cat.host_table(BY_NAME["b9_first_removed"])
    assert cat.same(o, ref) is None


@pytest.mark.parametrize("name", ["rows_2049", "drop_first_of_tile", "b9_below_removed", "ranges_three", "drop_every_row"])
def test_the_order_of_removal_does_not_matter(name):
    case = BY_NAME[name]
    gone = case.removed()
    orders = [gone, gone[::-1], gone[1::2] + gone[0::2], gone[len(gone) // 2:] + gone[:len(gone) // 2]]
    first = cat.statement_table(case, orders[0])
    for order in orders[1:]:
        assert cat.same(first, cat.statement_table(case, order)) is None
    assert len({tuple(o) for o in orders}) >= min(3, math.factorial(len(gone)))       # three orders wherever the set has three
    assert cat.same(first, cat.host_table(case)) is None


@pytest.mark.parametrize("name", ["rows_2049", "drop_whole_tile", "b5_middle_removed", "empty_tail_3000", "ranges_three"])
def test_repacking_a_repacked_table_changes_nothing(name):
    case = BY_NAME[name]
    once = cat.host_table(case)
    rows, total = int(once["counts_out"][0]), int(once["counts_out"][1])
    again = cat.Case("again", [], case.n_blocks_out, None, case.n_blocks_out, start=once["obs_start_out"][:rows + 1],
                     recon_start=once.get("recon_start_out"))
    again.obs, again.n_obs = once["obs_out"][:max(total, 1)].copy(), total
    twice = cat.host_table(again)
    assert np.array_equal(twice["key_out"][:rows], np.arange(rows))
    assert tuple(twice["counts_out"]) == (rows, total, 0, 0, 0)
    for k in ("obs_start_out", "obs_counts_out", "landmarks_out", "call_verdict"):
        assert np.array_equal(twice[k], once[k]), k
    assert np.array_equal(twice["obs_out"][:total], once["obs_out"][:total])
    if "recon_start_out" in once:
        assert np.array_equal(twice["recon_start_out"], once["recon_start_out"])


def test_rooms_one_short_keep_the_true_counts():
    for size in ("small", "big"):
        exact = cat.host_table(BY_NAME[f"rooms_{size}_exact"])
        assert int(exact["call_verdict"][0]) == cat.OK
        for short in ("one_row_short", "one_observation_short"):
            o = cat.host_table(BY_NAME[f"rooms_{size}_{short}"])
            assert int(o["call_verdict"][0]) == cat.NO_ROOM and np.array_equal(o["counts_out"], exact["counts_out"])
            assert np.all(o["obs_start_out"] == 0) and np.all(o["key_out"] == cat.NONE) and np.all(o["landmarks_out"] == cat.NONE)
            assert np.all(o["obs_out"] == cat.POISON)


# ---- the pools ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row_bytes", cat.GATHER_ROW_BYTES)
@pytest.mark.parametrize("case", cat.gather_cases(), ids=lambda c: c[0])
def test_gather_moves_rows_and_zeroes_the_rest(case, row_bytes):
    name, nb, block_map, out, expect = case
    src = cat.pool(nb, row_bytes)
    dst, verdict = cat.host_gather(src, row_bytes, nb, block_map, out)
    assert int(verdict[0]) == expect
    want = np.zeros((out, row_bytes), np.uint8)
    if expect == cat.OK:
        for b in range(nb):
            m = b if block_map is None else block_map[b]
            if m != cat.NONE:
                want[m] = src[b]
    assert np.array_equal(dst[:out], want)


# ---- the constraints -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 513])
@pytest.mark.parametrize("gone", [(), (0,), (4,), (8,), (1, 7), tuple(range(9))])
def test_constraints_are_the_statements_retain(n, gone):
    nb = 9
    views, poses, verdict = cat.constraint_case(n, nb)
    block_map, out = cat.compact(nb, set(gone))
    start = [0, n // 3, n // 3, n]
    o = cat.host_constraints(views, poses, verdict, block_map, nb, out, start)
    table = ([0], np.zeros((0, 2), np.uint32))
    r = stmt.repack(table[0], table[1], 0, nb, cat.CAP, block_map, list(gone), constraints=[(v, c) for c, v in enumerate(views)])
    kept = [c for _, c in r["constraints"]]
    k = len(kept)
    assert int(o["count"][0]) == k
    assert np.array_equal(o["views_out"][:k], np.array([v for v, _ in r["constraints"]], np.uint32).reshape(k, 3))
    assert np.array_equal(o["poses_out"][:k], poses[kept]) and np.array_equal(o["verdict_out"][:k], verdict[kept])
    assert np.all(o["views_out"][k:n] == cat.NONE) and np.all(o["verdict_out"][k:n] == 3) and np.all(o["poses_out"][k:n] == 0.0)
    assert list(o["start_out"]) == [sum(1 for c in kept if c < s) for s in start]
    if n >= 255 and len(gone) == 1:
        lost = {int(np.where(views[c] == gone[0])[0][0]) for c in range(n) if gone[0] in views[c]}
        assert lost == {0, 1, 2}                       # constraints that lose their first, their second, their third view
        assert any(np.array_equal(views[c], views[c - 1]) for c in kept if c)                          # duplicates survive as two


def test_constraints_outside_the_map_are_dropped():
    views = np.array([[0, 1, 2], [0, 9, 2], [3, 4, 5], [3, 4, 0xFFFFFFFF]], np.uint32)
    poses, verdict = np.ones((4, 2, 12)), np.zeros(4, np.uint32)
    o = cat.host_constraints(views, poses, verdict, [0, 1, 2, 3, 9, 5, 6, 7, 8], 9, 9)          # 4 -> 9: no block of the output
    assert int(o["count"][0]) == 1 and list(o["views_out"][0]) == [0, 1, 2]
    o = cat.host_constraints(views, poses, verdict, None, 9, 9)
    assert int(o["count"][0]) == 2


# ---- the frame table -----------------------------------------------------------------------------------------------------------
def test_frames_follow_their_views():
    nb = 9
    block_map, _ = cat.compact(nb, {2, 5})
    recon = np.array([0, 0, 1, 0, cat.NONE, 0, 0, 1], np.uint32)
    view = np.array([0, 2, 2, 5, 2, 8, 9, 5], np.uint32)
    frames = [[None, None] if r == cat.NONE else [int(r), int(v)] for r, v in zip(recon, view)]
    ok = [f for f in frames if f[1] is None or f[1] < nb]
    table = ([0], np.zeros((0, 2), np.uint32))
    want = stmt.repack(table[0], table[1], 0, nb, cat.CAP, block_map, [5, 2], frames=ok, reconstruction=0)["frames"]
    got_recon, got_view, flags = cat.host_frames(recon, view, 0, block_map, nb)
    assert int(flags[0]) == 1 and got_recon[6] == 0 and got_view[6] == 9               # a view outside the blocks: untouched, flagged
    got = [[None, None] if r == cat.NONE else [int(r), int(v)] for r, v in zip(got_recon, got_view)]
    del got[6]
    # a frame of another reconstruction, or without a view, keeps what it had; a removed view leaves the frame without one
    assert [g[0] for g in got] == [w[0] for w in want]
    assert [g[1] for g in got if g[0] is not None] == [w[1] for w in want if w[0] is not None]
    assert int(cat.host_frames(recon[:6], view[:6], 0, block_map, nb)[2][0]) == 0


def test_the_direct_answer_of_a_one_observation_table_is_the_host_builds_and_the_statements():
    """cat.direct_table (numpy alone) is what the GPU test holds the tables beyond one pass of the tile sums to next to the host
    build: here the three are tied together on a table small enough for the statement — three tiles, rows removed at the first
    and last place of a tile — and the direct answer and the host build on the large tables themselves."""
    small = cat.tile_sums_case("three_tiles", 2 * cat.TILE + 1, {0, 5, cat.TILE - 1, cat.TILE, 2 * cat.TILE})
    direct = cat.direct_table(small)
    assert cat.same(direct, cat.host_table(small)) is None
    assert cat.same(direct, cat.statement_table(small)) is None
    assert int(direct["counts_out"][0]) == 2 * cat.TILE + 1 - 5
    for case in cat.tile_sums_cases():
        direct = cat.direct_table(case)
        assert cat.same(direct, cat.host_table(case)) is None, case.name
        edge = cat.SUMS_PASS * cat.TILE
        k = direct["key_out"]
        assert k[edge - 1] == cat.NONE and k[edge - 2] != cat.NONE                  # removed below the boundary of the trips
        tiles = np.add.reduceat((k[:case.n_landmarks] != cat.NONE).astype(np.int64), np.arange(0, case.n_landmarks, cat.TILE))
        assert np.all(tiles > 0) and np.count_nonzero(tiles[:cat.SUMS_PASS] < cat.TILE) > 250    # every tile keeps rows, most lose one
        if case.n_landmarks > edge:
            assert k[edge] == edge - len(case.doomed[case.doomed < edge])           # the carry of the first trip
        if case.n_landmarks == edge + 3:
            assert k[edge + 1] == cat.NONE and k[edge + 2] == k[edge] + 1           # removed above it, between two kept rows


def test_the_direct_answer_of_a_gather_is_the_host_builds():
    """cat.direct_gather (numpy alone) stands in for the host build at the rows of megabytes tests/test_gpu_repack.py moves: here
    the two agree on every accepted case of the catalogue, at every row length of the small table"""
    for row_bytes in cat.GATHER_ROW_BYTES:
        for name, nb, block_map, out, expect in cat.gather_cases():
            if expect != cat.OK:
                continue
            src = cat.pool(nb, row_bytes)
            host, verdict = cat.host_gather(src, row_bytes, nb, block_map, out)
            assert int(verdict[0]) == cat.OK and np.array_equal(host[:out], cat.direct_gather(src, block_map, out)), (name, row_bytes)
    for row_bytes, _, nb in cat.GATHER_LONG_ROWS:                                  # and at the long rows the host build still takes in a moment
        if row_bytes > 16 * 1025:
            continue
        m, out = cat.compact(nb, {nb // 2})
        src = cat.pool(nb, row_bytes)
        host, _ = cat.host_gather(src, row_bytes, nb, m, out)
        assert np.array_equal(host, cat.direct_gather(src, m, out)), row_bytes
