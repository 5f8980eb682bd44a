"""From the frames found to the searches on the device (cv_amd/csrc/hm_view_plan.hip): hm_view_plan_device held to
tests/view_plan_statement.py behind a real FrameIndex.find, byte for byte; hm_knn_planned_batch_device and
hm_best_of_views_planned_batch_device held to tests/matching_statement.py and to the bytes of the host-planned entry points on the
same problems; Registration.match_found held to match_views where both mean the same.  Every comparison is equality.

The descriptor blocks are matching_statement.aliased_blocks(cap=320) of several seeds side by side: 42 blocks whose query and target
counts differ and stand on both sides of the search's 256-query workgroup and 64-query wave (0, 1, 255, 256, 257, 320)."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest

import matching_statement as M
import place_statement as PS
import view_plan_statement as S
from test_gpu_parity import gpu  # noqa: F401  (gpu: the module fixture that builds the library)

pytestmark = pytest.mark.gpu

FILL = 0xA5A5A5A5
CASES = S.cases()
CAP, N_BLOCKS, N_VIEW_BLOCKS = 320, 42, 36
NT = np.array(([300, 0, 1, 255, 256, 257, 320, 33, 40] * 5)[:N_BLOCKS], np.int32)          # as targets
NQ = np.array(([5, 320, 40, 64, 65] * 8)[:N_VIEW_BLOCKS] + [320, 257, 0, 1, 255, 256], np.int32)      # as queries
FRAME_BLOCKS = {1: [36], 5: [37, 38, 39, 40, 41]}
BETTER_BY = 3
KERNELS = [("fp4", 3), ("fp4_regs", 3), ("int8", 3), ("valu", 2)]


def _dev():
    import torch
    return torch, torch.device("cuda", 0)


def _up(a):
    torch, dev = _dev()
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)


def _filled(nbytes, value=0xFF):
    torch, dev = _dev()
    return torch.full((nbytes,), value, dtype=torch.uint8, device=dev)


def _u32p(a):
    return np.ascontiguousarray(a, np.uint32).ctypes.data_as(C.c_void_p)


def _wait():
    from cv_amd import _lib
    torch, _ = _dev()
    return _lib.wait_handle(torch.cuda.current_stream())


def _sync(m):
    from cv_amd import _lib
    _lib.check(_lib.lib().hm_sync(m.handle), "hm_sync")


# ------------------------------------------------------------------------------------------------ the blocks and their answers
@lru_cache(maxsize=None)
def blocks():
    buf = np.concatenate([M.aliased_blocks(seed=s, cap=CAP)["buf"] for s in range(N_BLOCKS // 3)])
    rng = np.random.default_rng(0x5650)
    for b in range(1, N_BLOCKS, 2):                             # near copies across blocks: distances that decide something
        rows = rng.random(CAP) < 0.3
        buf[b, rows] = buf[b - 1, rows]
        buf[b, rows, 0] ^= rng.integers(0, 4, int(rows.sum())).astype(np.uint8)
    landmarks = rng.integers(0, 200, (N_BLOCKS, CAP)).astype(np.uint32)
    buf.setflags(write=False)
    return buf, landmarks


@lru_cache(maxsize=None)
def knn3(qb, tb):
    """the statement's three neighbours of query block qb's features in target block tb: computed once"""
    buf, _ = blocks()
    return M.knn(buf[qb, :NQ[qb]], buf[tb, :NT[tb]], 3)


def lists_for(F, V, seed=0):
    """view lists a kernel other than the plan's might have written: frame f's first nvs[f] entries are its views; behind them NONE
    or a block number that must not be searched"""
    rng = np.random.default_rng([0x5650, F, V, seed])
    nvs = np.array([V, 0, (V + 1) // 2, 1, V][:F] if F > 1 else [V], np.uint32)
    view_idx = np.full((F, V), S.NONE, np.uint32)
    for f in range(F):
        view_idx[f, :nvs[f]] = rng.choice(N_VIEW_BLOCKS, nvs[f], replace=False)
        if f % 2 == 0:
            view_idx[f, nvs[f]:] = 7                            # behind the count: not a view of this frame
    return view_idx, nvs


def padded(view_idx, nvs):
    """place_recognition.view_blocks' lists: a frame with fewer views repeats its last one (none: block 0)"""
    out = view_idx.copy()
    for f, nv in enumerate(nvs):
        out[f, nv:] = out[f, nv - 1] if nv else 0
    return out


class Device:
    """the table on the device, and the calls"""

    def __init__(self, m):
        buf, landmarks = blocks()
        self.m = m
        self.d_buf, self.d_nq, self.d_nt, self.d_lm = _up(buf), _up(NQ), _up(NT), _up(landmarks)

    def planned(self, fb, view_idx, nvs, k, exp_blocks=None, d_view_idx=None, d_nvs=None):
        """-> (knn [F][V][cap][k] NB, best [F][cap][3][2], decision [F][cap]) with the fill where nothing was written"""
        from cv_amd import _lib
        L = _lib.lib()
        F, V = view_idx.shape
        d_vi = _up(view_idx) if d_view_idx is None else d_view_idx
        d_nv = _up(nvs) if d_nvs is None else d_nvs
        d_out, d_best, d_dec = _filled(F * V * CAP * k * 8), _filled(F * CAP * 24), _filled(F * CAP * 4)
        exp_blocks = min(F * V, N_BLOCKS) if exp_blocks is None else exp_blocks
        _lib.check(L.hm_knn_planned_batch_device(self.m.handle, self.d_buf.data_ptr(), self.d_nq.data_ptr(), self.d_buf.data_ptr(), self.d_nt.data_ptr(),
                                                 CAP, _u32p(fb), d_vi.data_ptr(), d_nv.data_ptr(), F, V, N_BLOCKS, exp_blocks, k, d_out.data_ptr(),
                                                 _wait()), "knn_planned")
        _lib.check(L.hm_best_of_views_planned_batch_device(self.m.handle, d_out.data_ptr(), self.d_nq.data_ptr(), _u32p(fb), CAP, d_vi.data_ptr(),
                                                           d_nv.data_ptr(), F, V, N_BLOCKS, k, self.d_lm.data_ptr(), self.d_nt.data_ptr(), BETTER_BY,
                                                           d_best.data_ptr(), d_dec.data_ptr(), None), "best_planned")
        _sync(self.m)
        return (d_out.cpu().numpy().view(M.NB).reshape(F, V, CAP, k), d_best.cpu().numpy().view(np.uint32).reshape(F, CAP, 3, 2),
                d_dec.cpu().numpy().view(np.uint32).reshape(F, CAP))

    def host_planned(self, fb, lists, k):
        """hm_knn_batch_device + hm_best_of_views_batch_device on host lists [F][V]"""
        from cv_amd import _lib
        L = _lib.lib()
        F, V = lists.shape
        d_out, d_best, d_dec = _filled(F * V * CAP * k * 8), _filled(F * CAP * 24), _filled(F * CAP * 4)
        _lib.check(L.hm_knn_batch_device(self.m.handle, self.d_buf.data_ptr(), self.d_nq.data_ptr(), self.d_buf.data_ptr(), self.d_nt.data_ptr(), CAP,
                                         _u32p(np.repeat(fb, V)), _u32p(lists), F * V, k, d_out.data_ptr(), _wait()), "knn_batch")
        _lib.check(L.hm_best_of_views_batch_device(self.m.handle, d_out.data_ptr(), self.d_nq.data_ptr(), _u32p(fb), CAP, _u32p(lists), F, V, k,
                                                   self.d_lm.data_ptr(), self.d_nt.data_ptr(), BETTER_BY, d_best.data_ptr(), d_dec.data_ptr(), None),
                   "best_batch")
        _sync(self.m)
        return (d_out.cpu().numpy().view(M.NB).reshape(F, V, CAP, k), d_best.cpu().numpy().view(np.uint32).reshape(F, CAP, 3, 2),
                d_dec.cpu().numpy().view(np.uint32).reshape(F, CAP))


def unwritten(a):
    return (np.ascontiguousarray(a).view(np.uint8) == 0xFF).all()


def held(dev, F, V, k, what):
    """one planned call against the statement and against the host-planned entry points"""
    _, landmarks = blocks()
    fb = np.array(FRAME_BLOCKS[F], np.uint32)
    view_idx, nvs = lists_for(F, V)
    got, best, dec = dev.planned(fb, view_idx, nvs, k)
    ref, rbest, rdec = dev.host_planned(fb, padded(view_idx, nvs), k)
    for f in range(F):
        nq, nv = int(NQ[fb[f]]), int(nvs[f])
        for v in range(V):
            if v >= nv:
                assert unwritten(got[f, v]), (what, f, v, "a dead slab was written")
                continue
            idx, dist = knn3(int(fb[f]), int(view_idx[f, v]))
            M.check_neighbors(got[f, v, :nq], idx[:, :k], dist[:, :k], M.ABI_ABSENT, f"{what}: frame {f} view {v}")
            assert got[f, v, :nq].tobytes() == ref[f, v, :nq].tobytes(), (what, f, v, "not hm_knn_batch_device's bytes")
            assert unwritten(got[f, v, nq:]), (what, f, v)
        wbest, wdec = M.best_of_views(got[f, :nv], nq, landmarks, view_idx[f, :nv], NT, BETTER_BY)
        assert np.array_equal(best[f, :nq], wbest) and np.array_equal(dec[f, :nq], wdec), (what, f)
        assert unwritten(best[f, nq:]) and unwritten(dec[f, nq:]), (what, f)
        if nv:
            assert np.array_equal(best[f, :nq], rbest[f, :nq]) and np.array_equal(dec[f, :nq], rdec[f, :nq]), (what, f, "not hm_best_of_views_batch_device's")
        else:
            assert (best[f, :nq] == S.NONE).all() and (dec[f, :nq] == 0).all(), (what, f)
    return dec


@pytest.fixture(scope="module")
def device(gpu):
    _, knn = gpu
    m = knn.Matcher(CAP)
    yield Device(m)
    m.close()


def test_the_table_stands_on_both_sides_of_the_workgroup_and_the_wave():
    assert set(NT) >= {0, 1, 255, 256, 257, CAP} and set(NQ) >= {0, 1, 255, 256, 257, CAP} and set(NQ) >= {64, 65}
    assert {int(NQ[b]) for b in FRAME_BLOCKS[5]} == {257, 0, 1, 255, 256} and NQ[FRAME_BLOCKS[1][0]] == CAP
    view_idx, nvs = lists_for(5, 32)
    assert {int(NT[b]) for f in range(5) for b in view_idx[f, :nvs[f]]} >= {0, 1, 255, 256, 257, CAP}
    assert list(nvs) == [32, 0, 16, 1, 32] and (view_idx[0, :32] < N_VIEW_BLOCKS).all() and (view_idx[1] == S.NONE).all() and (view_idx[2, 16:] == 7).all()


# ------------------------------------------------------------------------------------------------ the plan
def plan_outputs(matcher, c):
    from cv_amd import place_recognition as P
    from test_gpu_place import index_of
    idx = index_of(matcher, c["table"])
    found = idx.find(c["queries"], P.params(**c["params"]), c["visible"], fill=FILL - (1 << 32))
    plan = P.plan_views(found, c["V"], c["n_blocks"], pick=c["pick"], by_recon=c["by_recon"], exp_blocks=c["exp_blocks"])
    _sync(matcher)
    u = lambda t: t.cpu().numpy().view(np.uint32)
    return dict(view_idx=u(plan.view_idx), n_views=u(plan.n_views), verdict=u(plan.verdict), counts=u(plan.counts))


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_plan_is_the_statement(device, name):
    """behind a real find on the matcher's stream, no wait between the two; the plan writes every word of its outputs"""
    c = CASES[name]
    got, want = plan_outputs(device.m, c), S.outputs(c, fill=FILL)
    assert set(got) == set(want)
    for k in want:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (name, k, got[k].tolist(), want[k].tolist())


# ------------------------------------------------------------------------------------------------ the search
@pytest.mark.parametrize("F", [1, 5])
@pytest.mark.parametrize("V", [1, 3, 32])
def test_the_planned_search_is_the_statement_and_the_host_planned_bytes(device, F, V):
    decisions = set()
    for k in (1, 2, 3):
        decisions |= set(held(device, F, V, k, f"F {F} V {V} k {k}").reshape(-1).tolist())
    if V == 32:
        assert {0, 1, 2} <= decisions                           # the three decisions all occur


@pytest.mark.parametrize("kernel,k", KERNELS, ids=[name for name, _ in KERNELS])
def test_every_family_a_context_can_be_created_with(gpu, kernel, k):
    _, knn = gpu
    m = knn.Matcher(CAP, kernel=kernel)
    try:
        held(Device(m), 5, 3, k, kernel)
    finally:
        m.close()


def test_a_key_that_is_no_block_is_a_dead_problem(device):
    fb = np.array(FRAME_BLOCKS[5], np.uint32)
    view_idx, nvs = lists_for(5, 3)
    bad = view_idx.copy()
    bad[0, 1] = N_BLOCKS                                        # frame 0: 3 views, the middle one no block
    bad[4, 0] = S.NONE
    got, best, dec = device.planned(fb, bad, nvs, 3)
    ref, _, _ = device.planned(fb, view_idx, nvs, 3)
    _, landmarks = blocks()
    assert unwritten(got[0, 1]) and unwritten(got[4, 0])
    for f, v in ((0, 0), (0, 2), (4, 1), (4, 2), (2, 0), (3, 0)):
        assert got[f, v].tobytes() == ref[f, v].tobytes(), (f, v)
    for f, keep in ((0, [0, 2]), (4, [1, 2])):
        nq = int(NQ[fb[f]])
        wbest, wdec = M.best_of_views(ref[f][keep], nq, landmarks, view_idx[f][keep], NT, BETTER_BY)
        assert np.array_equal(best[f, :nq], wbest) and np.array_equal(dec[f, :nq], wdec), f


def test_exp_blocks_exact_and_one_short_behind_a_find(device):
    """the plan of the catalogue's five distinct blocks with room for five and for four, searched over the table's blocks"""
    from cv_amd import _lib, place_recognition as P
    from test_gpu_place import index_of
    _, landmarks = blocks()
    fb = np.array([39, 40, 41], np.uint32)
    for name, call, live in (("room_exact", S.OK, 7), ("room_short", S.NO_ROOM, 0)):
        c = CASES[name]
        want = S.outputs(c)
        idx = index_of(device.m, c["table"])
        found = idx.find(c["queries"], P.params(**c["params"]), c["visible"])
        plan = P.plan_views(found, c["V"], c["n_blocks"], exp_blocks=c["exp_blocks"])
        got, best, dec = device.planned(fb, want["view_idx"], want["n_views"], 3, exp_blocks=c["exp_blocks"], d_view_idx=plan.view_idx, d_nvs=plan.n_views)
        counts = plan.counts.cpu().numpy().view(np.uint32)
        assert counts.tolist() == [5, live, call, 3 if live else 0] == want["counts"].tolist()
        assert np.array_equal(plan.view_idx.cpu().numpy().view(np.uint32), want["view_idx"])
        for f in range(3):
            nq, nv = int(NQ[fb[f]]), int(want["n_views"][f])
            assert nv == (0 if call == S.NO_ROOM else [2, 2, 3][f])
            for v in range(c["V"]):
                if v >= nv:
                    assert unwritten(got[f, v]), (name, f, v)
                    continue
                idx3, dist3 = knn3(int(fb[f]), int(want["view_idx"][f, v]))
                M.check_neighbors(got[f, v, :nq], idx3, dist3, M.ABI_ABSENT, f"{name}: frame {f} view {v}")
            wbest, wdec = M.best_of_views(got[f, :nv], nq, landmarks, want["view_idx"][f, :nv], NT, BETTER_BY)
            assert np.array_equal(best[f, :nq], wbest) and np.array_equal(dec[f, :nq], wdec) and unwritten(best[f, nq:]), (name, f)
            if call == S.NO_ROOM:
                assert (best[f, :nq] == S.NONE).all() and (dec[f, :nq] == 0).all()
    # a list of the caller's own with more distinct blocks than the room: nothing is searched
    view_idx, nvs = lists_for(5, 3)
    distinct = len({int(b) for f in range(5) for b in view_idx[f, :nvs[f]]})
    fb5 = np.array(FRAME_BLOCKS[5], np.uint32)
    exact, _, _ = device.planned(fb5, view_idx, nvs, 3, exp_blocks=distinct)
    full, _, _ = device.planned(fb5, view_idx, nvs, 3)
    assert exact.tobytes() == full.tobytes() and not unwritten(exact)
    from cv_amd import _lib as lib_
    d_out = _filled(5 * 3 * CAP * 3 * 8)
    lib_.check(lib_.lib().hm_knn_planned_batch_device(device.m.handle, device.d_buf.data_ptr(), device.d_nq.data_ptr(), device.d_buf.data_ptr(),
                                                      device.d_nt.data_ptr(), CAP, _u32p(fb5), _up(view_idx).data_ptr(), _up(nvs).data_ptr(), 5, 3, N_BLOCKS,
                                                      distinct - 1, 3, d_out.data_ptr(), _wait()), "knn_planned, one short")
    _sync(device.m)
    assert unwritten(d_out.cpu().numpy())


def test_two_calls_and_permuted_frames_give_the_same_bytes_per_frame(device):
    fb = np.array(FRAME_BLOCKS[5], np.uint32)
    view_idx, nvs = lists_for(5, 32)
    a, abest, adec = device.planned(fb, view_idx, nvs, 3)
    b, bbest, bdec = device.planned(fb, view_idx, nvs, 3)
    assert a.tobytes() == b.tobytes() and abest.tobytes() == bbest.tobytes() and adec.tobytes() == bdec.tobytes()
    perm = np.array([3, 0, 4, 2, 1])
    p, pbest, pdec = device.planned(fb[perm], view_idx[perm], nvs[perm], 3)
    for at, f in enumerate(perm):
        assert p[at].tobytes() == a[f].tobytes() and pbest[at].tobytes() == abest[f].tobytes() and pdec[at].tobytes() == adec[f].tobytes(), (at, f)


# ------------------------------------------------------------------------------------------------ the chain
def test_match_found_is_match_views_on_a_one_group_table_behind_a_busy_producer(gpu):
    """The small scene of test_gpu_registration.py; every new frame's window holds views of ONE reconstruction, so that "the
    first V keys in group order" and "the first V keys of group 0" are the same list.  The parent's way (find, hm_sync,
    view_blocks, match_views, consensus) on settled inputs gives WANT; then the descriptor blocks hold zeros, a side stream
    stays busy and copies the true ones behind its delay, and hash_bag -> find -> match_found -> consensus are enqueued behind
    it with no hm_sync in between."""
    import torch
    import enqueue_contract as EC
    from cv_amd import _device, _lib, place_recognition as P
    from cv_amd.akaze import Akaze
    from cv_amd.registration import Registration
    from test_gpu_registration import landmark_keys, pan_world, world_table
    W, H, DX, DY, V, F, CAP2, CELL = 640, 360, 4, 2, 4, 8, 2048, 6
    NB = V + F
    dev = torch.device("cuda", 0)
    frames = pan_world(0x2E61, W, H, NB, DX, DY)
    ak = Akaze.default()
    ak.max_keypoints = CAP2
    ctx = ak.context(W, H, NB)
    L = _lib.lib()
    d_frames = torch.from_numpy(frames).to(dev)
    d_kps = torch.zeros((NB, CAP2, 28), dtype=torch.uint8, device=dev)
    d_true = torch.zeros((NB, CAP2, 64), dtype=torch.uint8, device=dev)
    d_counts = torch.zeros((NB,), dtype=torch.int32, device=dev)
    _lib.check(L.akz_extract_batch_device(ctx.handle, d_frames.data_ptr(), 0, NB, W, H, d_kps.data_ptr(), d_true.data_ptr(), CAP2,
                                          d_counts.data_ptr(), _lib.wait_handle(torch.cuda.current_stream())), "extract")
    _lib.check(L.akz_sync(ctx.handle), "akz_sync")
    counts = d_counts.cpu().numpy()
    kps = d_kps.cpu().numpy().view(_lib.KP_DTYPE).reshape(NB, CAP2)
    f_cam, z0 = 700.0, 5.0
    cam = (f_cam, f_cam, W / 2.0, H / 2.0, 0.0, None)
    wc, hc = (W + DX * NB) // CELL + 2, (H + DY * NB) // CELL + 2
    landmarks = np.zeros((NB, CAP2), np.uint32)
    for g in range(NB):
        landmarks[g, :counts[g]] = landmark_keys(kps[g, :counts[g]], g, DX, DY, CELL, wc)
    world = world_table(wc, hc, CELL, f_cam, W / 2.0, H / 2.0, z0)
    d_lm, d_world = torch.from_numpy(landmarks.view(np.int32)).to(dev), torch.from_numpy(world).to(dev)
    codewords = np.random.default_rng(5).integers(0, 256, (256, 64), dtype=np.uint8)
    reg = Registration(torch, CAP2, F, V, codewords, cam, threshold=2e-5, n_hypotheses=256, seed=11, block_size=32, max_candidates=64,
                       estimations_per_block=16)
    try:
        queries = np.arange(V, NB)
        prm = P.params(num_recent=9)                               # frame at position p sees the stored views above p - 9: 4, 4, 4, 4, 4, 3, 2, 1
        d_words = torch.zeros((NB, CAP2, 2), dtype=torch.int32, device=dev)

        def table():
            """the frame table's rows, written on the current torch stream: settled before anything is enqueued behind them"""
            idx = P.FrameIndex(torch, reg.matcher, NB, hash_bytes=32)
            tail = idx.append_rows(np.zeros(NB, np.uint32), np.arange(NB, dtype=np.uint32))
            idx.set_views(np.arange(V), np.full(V, 3, np.uint32), np.arange(V, dtype=np.uint32))
            torch.cuda.synchronize()
            return idx, tail

        def hash_into(tail, d_descs, wait):
            _device.call("hm_hash_bag_device", reg.matcher.handle, d_descs, d_counts, CAP2, NB, reg.d_codewords, 256, tail, d_words, wait)

        def outputs():
            reg.sync()
            return {k: getattr(reg, k).cpu().numpy().tobytes() for k in ("hash", "best", "decision", "pairs", "npairs", "pose", "best_id", "n_inliers")}

        # the parent's way, settled
        idx, tail = table()
        hash_into(tail, d_true, _wait())
        found = idx.find(queries, prm)
        _lib.check(L.hm_sync(reg.matcher.handle), "hm_sync")
        vb = P.view_blocks(found, V)
        assert [len(set(row)) for row in vb.tolist()] == [4, 4, 4, 4, 4, 3, 2, 1]
        reg.match_views(d_true, d_counts, list(queries), vb.tolist(), d_lm, stream_to_wait=torch.cuda.current_stream(dev))
        reg.consensus(d_kps, d_counts, d_world, len(world))
        want = outputs()
        assert int(reg.npairs.min()) > 40 and int((reg.best_id.cpu() != -1).sum()) >= F - 1
        # the new chain behind a busy producer of its descriptors
        cycles, ms = EC.calibrate(torch, want_ms=60.0)
        d_descs = torch.zeros_like(d_true)
        idx, tail = table()
        producer = EC.Producer(torch, cycles)
        producer.start([(d_descs, d_true)])
        assert not producer.done.query(), "the producer finished before the calls were made: the test shows nothing"
        hash_into(tail, d_descs, producer.wait_handle())
        found = idx.find(queries, prm)                             # (behind the hash_bag on the matcher's stream)
        reg.match_found(d_descs, d_counts, list(queries), found, d_lm, stream_to_wait=producer.wait_handle())
        reg.consensus(d_kps, d_counts, d_world, len(world))
        got = outputs()
        assert [k for k in want if got[k] != want[k]] == []
        assert reg.plan.n_views.cpu().tolist() == [4, 4, 4, 4, 4, 3, 2, 1] and reg.plan.counts.cpu().tolist() == [4, 26, S.OK, 8]
        assert (reg.plan.verdict.cpu() == S.OK).all()
    finally:
        reg.close()
