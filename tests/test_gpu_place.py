"""hm_find_frames_batch_device (cv_amd/csrc/hm_place.hip) through cv_amd.place_recognition, held to tests/place_statement.py — the
reference's function line by line — byte for byte, the entries a call does not write still holding the fill.  The catalogue is
test_place_statement.py's, where the host build of the kernels' decisions is held to the same statement.  The distance kernel's
tile is 64 queries x 64 stored rows: the sizes of the catalogue stand on either side of both."""
import ctypes as C

import numpy as np
import pytest

import matching_statement as M
import place_statement as S
from test_gpu_parity import gpu  # noqa: F401  (gpu: the module fixture that builds the library)

pytestmark = pytest.mark.gpu

FILL = 0xA5A5A5A5
CASES = S.cases()
TILE_Q = TILE_S = 64


def _torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def matcher(gpu):
    _, knn = gpu
    m = knn.Matcher(256)
    yield m
    m.close()


def index_of(matcher, t, capacity=None):
    from cv_amd.place_recognition import FrameIndex
    n = len(t["feed"])
    idx = FrameIndex(_torch(), matcher, n if capacity is None else capacity, hash_bytes=t["hashes"].shape[1])
    idx.append_rows(t["feed"], t["pos"], t["hashes"])
    idx.set_views(np.arange(n), t["recon"], t["view"])
    return idx


def device_outputs(matcher, c, pitch=None, search=True, idx=None):
    from cv_amd import _lib, place_recognition as P
    idx = idx or index_of(matcher, c["table"])
    r = idx.find(c["queries"], P.params(**c["params"]), c["visible"], search=search, row_pitch=pitch, fill=FILL - (1 << 32))
    _lib.check(_lib.lib().hm_sync(matcher.handle), "hm_sync")
    u = lambda t: t.cpu().numpy().view(np.uint32)
    o = dict(found=u(r.found), views_out=u(r.views_out), group_recon=u(r.group_recon), group_start=u(r.group_start), free=u(r.free),
             counts=u(r.counts), verdict=u(r.verdict))
    if search:
        o["search"] = u(r.search)[:, :c["params"]["search_num"]]
    return o


def same(got, want, what):
    assert set(got) == set(want)
    for k in want:
        assert got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
        bad = np.argwhere(got[k] != want[k])
        assert len(bad) == 0, (what, k, len(bad), bad[:4].tolist(), got[k][tuple(bad[0])], want[k][tuple(bad[0])])


def held(matcher, c, what, **kw):
    same(device_outputs(matcher, c, **kw), S.outputs(c["table"], c["queries"], c["visible"], c["params"], fill=FILL, **kw), what)


def test_the_catalogue_stands_on_both_sides_of_the_tiles():
    for n in (1, TILE_S - 1, TILE_S, TILE_S + 1, 3 * TILE_S + 5):
        for nq in (1, TILE_Q + 1):
            c = CASES[f"size_n{n}_q{nq}"]
            assert len(c["table"]["feed"]) == n and len(c["queries"]) == nq


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_device_is_the_statement(matcher, name):
    held(matcher, CASES[name], name)


@pytest.mark.parametrize("name", ["growing", "groups_three", "refusals", "widest"])
def test_a_wider_pitch_and_no_search_lists(matcher, name):
    c = CASES[name]
    held(matcher, c, name, pitch=S.room(c["params"]) + 5, search=False)


def test_the_search_is_left_out_when_nothing_reads_it(matcher):
    """num_similar = 0 and no d_search: the recent frames, their groups and n_searched all the same"""
    c = CASES["num_similar_0"]
    held(matcher, c, "no search", search=False)
    c = S.window_case(600, 1, 256, [0, 300, 599], num_similar=0)
    held(matcher, c, "no search, widest window", search=False)


def test_sees_newer_rows_only_without_visible(matcher):
    c = CASES["sees_newer_rows"]
    capped = dict(c, visible=c["queries"] + 1)
    a, b = device_outputs(matcher, c), device_outputs(matcher, capped)
    same(b, S.outputs(c["table"], c["queries"], capped["visible"], c["params"], fill=FILL), "visible = query + 1")
    assert not np.array_equal(a["found"], b["found"]) and (a["counts"][:, S.C_SEARCHED] >= b["counts"][:, S.C_SEARCHED]).all()


def test_growing_equals_the_replay(matcher):
    """visible = query + 1 over one batch == the table grown one frame at a time (the reference's sequence)"""
    c = CASES["growing"]
    got = device_outputs(matcher, c)
    literal = S.replay(c["table"], c["params"])
    for k, r in enumerate(literal):
        nr, ns = len(r["recent"]), len(r["similar"])
        assert got["verdict"][k] == S.OK and list(got["found"][k, :nr + ns]) == r["recent"] + r["similar"], k
        assert list(got["free"][k, :len(r["free"])]) == r["free"] and list(got["group_recon"][k, :len(r["groups"])]) == [g for g, _ in r["groups"]], k
        assert list(got["views_out"][k, :nr + ns - len(r["free"])]) == [v for _, views in r["groups"] for v in views], k


@pytest.mark.parametrize("name", ["ties_at_the_cut", "query_outside_its_own_list", "hash_bytes_512", "hash_bytes_4096", "growing", "search_num_above_visible"])
def test_the_search_list_is_hm_hash_knn(matcher, name):
    from cv_amd import _lib
    L = _lib.lib()
    c = CASES[name]
    t, k = c["table"], c["params"]["search_num"]
    got = device_outputs(matcher, c)
    for j, q in enumerate(c["queries"]):
        vis = len(t["feed"]) if c["visible"] is None else int(c["visible"][j])
        out = np.zeros(k, M.NB)
        n_out = C.c_uint32(0)
        query, stored = np.ascontiguousarray(t["hashes"][q]), np.ascontiguousarray(t["hashes"][:vis])
        _lib.check(L.hm_hash_knn(matcher.handle, query.ctypes.data, stored.ctypes.data, vis, stored.shape[1], k, out.ctypes.data, C.byref(n_out)),
                   "hm_hash_knn")
        m = n_out.value
        assert m == got["counts"][j, S.C_SEARCHED] == min(k, vis)
        assert np.array_equal(got["search"][j, :m, 0], out["index"][:m]) and np.array_equal(got["search"][j, :m, 1], out["distance"][:m]), (name, j)
        assert (got["search"][j, m:] == FILL).all()


def test_more_queries_than_one_pass(matcher):
    held(matcher, S.many_queries_case(), "many queries", search=False)
    c = S.many_queries_case(n=3000, nq=300)
    held(matcher, c, "many queries, one pass")


def test_one_larger_table(matcher):
    held(matcher, S.largest_case(), "20 000 x 512 bytes, 64 queries")


def test_refusals_of_a_query_leave_the_others(matcher):
    c = CASES["refusals"]
    got = device_outputs(matcher, c)
    assert list(got["verdict"]) == [S.OK, S.BAD_INDEX, S.BAD_INDEX, S.OK, S.BAD_INDEX, S.BAD_TABLE]
    for k in (1, 2, 4, 5):
        assert (got["counts"][k] == 0).all() and (got["found"][k] == FILL).all() and (got["search"][k] == FILL).all() and (got["group_start"][k] == FILL).all()
    for k in (0, 3):
        assert got["counts"][k, S.C_RECENT] > 0 and got["counts"][k, S.C_SEARCHED] == 8


@pytest.mark.parametrize("name", ["refusals", "groups_three"])
def test_the_cpp_mirror_answers_the_same(gpu, tmp_path, name):
    """cv_sfm::FrameIndex of include/akaze.hpp from a native process (tests/cpp/place.cpp): verdicts and counts of a case"""
    import subprocess
    import host_build
    c = CASES[name]
    t, p, q, vis = c["table"], c["params"], c["queries"], c["visible"]
    exe = host_build.native(tmp_path, "place.cpp", hip=True)
    path = tmp_path / "call.bin"
    with open(path, "wb") as fp:
        fp.write(np.array([len(t["feed"]), t["hashes"].shape[1], len(q), p["num_similar"], p["num_recent"], p["recent_threshold"], p["search_num"],
                           0 if vis is None else 1], np.uint32).tobytes())
        for a in (t["hashes"], t["feed"], t["pos"], t["recon"], t["view"], q) + (() if vis is None else (vis,)):
            fp.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.endswith("place ok\n"), (r.returncode, r.stdout[-300:], r.stderr[-300:])
    want = S.outputs(t, q, vis, p, search=False)
    lines = [line.split() for line in r.stdout.splitlines() if line.startswith("query ")]
    assert len(lines) == len(q)
    for k, w in enumerate(lines):
        assert int(w[1]) == k and int(w[3]) == want["verdict"][k] and [int(v) for v in w[5:10]] == list(want["counts"][k]), (name, k, w)


def test_hash_bag_into_the_tail_then_find_then_match_views(gpu):
    """The chain: hm_hash_bag_device writes the hashes of a batch of descriptor blocks into the index's tail, find runs behind it
    on the matcher's stream with one wait at the end, and view_blocks of its result is what Registration.match_views takes."""
    torch = _torch()
    from cv_amd import _device, _lib, place_recognition as P
    from cv_amd.registration import Registration
    rng = np.random.default_rng(0x504C)
    cap, n_stored, F, V, n_codewords = 96, 10, 3, 3, 256
    nb = n_stored + F
    codewords = rng.integers(0, 256, (n_codewords, 64), dtype=np.uint8)
    counts = rng.integers(40, cap + 1, nb).astype(np.int32)
    descs = rng.integers(0, 256, (nb, cap, 64), dtype=np.uint8)
    for b in range(1, nb):                                        # frames that resemble the one before: near hashes
        keep = rng.random(cap) < 0.7
        descs[b, keep] = descs[b - 1, keep]
    dev = torch.device("cuda", 0)
    reg = Registration(torch, cap, F, V, codewords, (1000.0, 1000.0, 320.0, 240.0, 0.0, None), n_hypotheses=256, max_candidates=64,
                       estimations_per_block=16, block_size=32)
    try:
        d_descs, d_counts = torch.from_numpy(descs).to(dev), torch.from_numpy(counts).to(dev)
        d_landmarks = torch.from_numpy(rng.integers(0, 500, (nb, cap)).astype(np.int32)).to(dev)
        d_words = torch.zeros((nb, cap, 2), dtype=torch.int32, device=dev)
        idx = P.FrameIndex(torch, reg.matcher, nb, hash_bytes=n_codewords // 8)
        feed, pos = np.zeros(nb, np.uint32), np.arange(nb, dtype=np.uint32)
        recon = np.where(np.arange(nb) < n_stored, 3 + np.arange(nb) % 2, S.NONE).astype(np.uint32)
        view = np.arange(nb, dtype=np.uint32)                    # a stored frame's view key is its block
        prm = dict(num_similar=2, num_recent=3, recent_threshold=0, search_num=6)
        for b0, b1 in ((0, n_stored), (n_stored, nb)):           # the stored frames, then the batch: both through hash_bag
            tail = idx.append_rows(feed[b0:b1], pos[b0:b1])
            _device.call("hm_hash_bag_device", reg.matcher.handle, d_descs[b0:b1], d_counts[b0:b1], cap, b1 - b0, reg.d_codewords, n_codewords, tail,
                         d_words[b0:b1], _device.wait(torch.cuda.current_stream(dev)))
            if b0 == 0:
                idx.set_views(np.arange(n_stored), recon[:n_stored], view[:n_stored])
        queries = np.arange(n_stored, nb)
        r = idx.find(queries, P.params(**prm), visible=queries + 1, search=True, fill=FILL - (1 << 32))
        _lib.check(_lib.lib().hm_sync(reg.matcher.handle), "hm_sync")          # the one wait
        hashes = np.stack([M.hash_bag(descs[b, :counts[b]], codewords)[0] for b in range(nb)])
        assert np.array_equal(idx.hashes.cpu().numpy(), hashes)
        t = S.table(hashes, feed, pos, recon, view)
        want = S.outputs(t, queries, queries + 1, prm, fill=FILL)
        u = lambda a: a.cpu().numpy().view(np.uint32)
        same(dict(found=u(r.found), views_out=u(r.views_out), group_recon=u(r.group_recon), group_start=u(r.group_start), free=u(r.free),
                  counts=u(r.counts), verdict=u(r.verdict), search=u(r.search)), want, "the chain")
        vb = P.view_blocks(r, V, pad=0)
        for k in range(F):
            have = int(want["group_start"][k, want["counts"][k, S.C_GROUPS]])
            assert have >= 1 and list(vb[k, :min(have, V)]) == list(want["views_out"][k, :min(have, V)]) and (vb[k, have:] == 0).all()
            assert (vb[k] < n_stored).all()
        reg.match_views(d_descs, d_counts, list(queries), vb.tolist(), d_landmarks, stream_to_wait=torch.cuda.current_stream(dev))
        reg.sync()
        assert np.array_equal(reg.hash[:F].cpu().numpy(), hashes[n_stored:])          # the registration hashed the same frames
    finally:
        reg.close()
