"""The HIP matcher stage (cv_amd/csrc/hm_match.hip) held to the independent numpy / Python statement of the reference
(tests/matching_statement.py) on its catalogue of designed inputs: every index, distance, pair, decision and hash byte equal,
and equal to the closed form where the input has one.  The catalogue and its "reaches what it was built for" checks are those
of test_matching_statement.py, where the C oracle is held to the same statement."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest

import matching_statement as S
import test_matching_statement as T
from test_gpu_parity import gpu  # noqa: F401  (gpu: the module fixture that builds the library)

pytestmark = pytest.mark.gpu

KERNELS = [("fp4", (1, 2, 3)), ("fp4_regs", (1, 2, 3)), ("int8", (1, 2, 3)), ("valu", (2,))]     # the VALU kernel exists for k = 2
KNN_CASES = T.KNN_CASES


def _u32p(a):
    return np.ascontiguousarray(a, np.uint32).ctypes.data_as(C.c_void_p)


def _dev():
    import torch
    return torch, torch.device("cuda", 0)


def _up(a):
    """A host array as a flat uint8 tensor on the device."""
    torch, dev = _dev()
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)


def _filled(nbytes, value=0xFF):
    torch, dev = _dev()
    return torch.full((nbytes,), value, dtype=torch.uint8, device=dev)


def _down(t, dtype, shape):
    return t.cpu().numpy().view(dtype).reshape(shape)


def _wait():
    from cv_amd import _lib
    torch, _ = _dev()
    return _lib.wait_handle(torch.cuda.current_stream())


def _check_case(got, q, t, k, closed, what):
    idx, dist = S.knn(q, t, k)
    S.check_neighbors(got, idx, dist, S.ABI_ABSENT, what)                         # the statement, every entry
    if closed is not None:
        cidx, cdist, mask = closed(k)
        S.check_neighbors(got, cidx, cdist, S.ABI_ABSENT, what + " (closed form)", mask)


@pytest.mark.parametrize("kernel,ks", KERNELS, ids=[k for k, _ in KERNELS])
def test_knn_catalogue_through_every_kernel(gpu, kernel, ks):
    _, knn = gpu
    m = knn.Matcher(1024, kernel=kernel)
    try:
        for name, q, t, closed in KNN_CASES:
            for k in ks:
                _check_case(m.knn(q, t, k), q, t, k, closed, f"{kernel}: {name}, k {k}")
            if len(t) >= 2:
                _check_case(m.knn2(q, t), q, t, 2, closed, f"{kernel}: {name}, knn2")
    finally:
        m.close()


def test_knn_catalogue_through_the_resident_and_the_batched_entry_points(gpu):
    """hm_set_targets / hm_knn_targets case by case, and hm_knn_batch_device with every case a problem of ONE call."""
    _, knn = gpu
    from cv_amd import _lib
    L = _lib.lib()
    cap = max(max(len(q), len(t)) for _, q, t, _ in KNN_CASES)
    assert cap == 513
    m = knn.Matcher(cap)
    try:
        for name, q, t, closed in KNN_CASES:
            m.set_targets(t)
            for k in (1, 2, 3):
                _check_case(m.knn_targets(q, k), q, t, k, closed, f"knn_targets: {name}, k {k}")
        n = len(KNN_CASES)
        qs = np.full((n, cap, 64), 0x5A, np.uint8); ts = np.full((n, cap, 64), 0xA5, np.uint8)
        for p, (_, q, t, _) in enumerate(KNN_CASES):
            qs[p, :len(q)] = q; ts[p, :len(t)] = t
        d_q, d_t = _up(qs), _up(ts)
        d_nq = _up(np.array([len(c[1]) for c in KNN_CASES], np.int32)); d_nt = _up(np.array([len(c[2]) for c in KNN_CASES], np.int32))
        order = np.arange(n, dtype=np.uint32)
        for k in (1, 2, 3):
            d_out = _filled(n * cap * k * 8)
            _lib.check(L.hm_knn_batch_device(m.handle, d_q.data_ptr(), d_nq.data_ptr(), d_t.data_ptr(), d_nt.data_ptr(), cap, _u32p(order),
                                             _u32p(order), n, k, d_out.data_ptr(), _wait()), "knn_batch")
            _lib.check(L.hm_sync(m.handle), "hm_sync")
            got = _down(d_out, S.NB, (n, cap, k))
            for p, (name, q, t, closed) in enumerate(KNN_CASES):
                _check_case(got[p, :len(q)], q, t, k, closed, f"knn_batch: {name}, k {k}")
                assert (got[p, len(q):]["index"] == 0xFFFFFFFF).all()             # nothing written past the query count
    finally:
        m.close()


@pytest.mark.parametrize("kernel,ks", KERNELS, ids=[k for k, _ in KERNELS])
def test_largest_admitted_target_set(gpu, kernel, ks):
    """2^21 - 1 targets — the key's row field at its last values — with distance 0, 1, 1, 2 planted at 2^21 - 2, 0, 2^21 - 3 and
    2^20 - 1; four queries, one search per kernel (k = 3, the VALU kernel k = 2)."""
    _, knn = gpu
    c = S.largest_target_set()
    k = max(ks)
    m = knn.Matcher(S.LARGEST_NT, kernel=kernel)
    try:
        got = m.knn(c["q"], c["t"], k)
    finally:
        m.close()
    assert got["index"][0].tolist() == [p for p, _ in S.LARGEST_PLANTS[:k]] and got["distance"][0].tolist() == [0, 1, 1][:k]
    S.check_neighbors(got, c["idx"][:, :k], c["dist"][:, :k], S.ABI_ABSENT, f"{kernel}: 2^21 - 1 targets")


@pytest.mark.parametrize("kernel", ["fp4", "fp4_regs", "int8", "valu"])
def test_one_buffer_as_queries_and_as_targets_with_different_counts(gpu, kernel):
    """hm_knn_batch_device with d_q == d_t and d_nq != d_nt, and hm_hash_bag_device with a frame block at the codebook's
    address: every problem equals the statement (a recoding made for the one count must not serve the other)."""
    _, knn = gpu
    from cv_amd import _lib
    L = _lib.lib()
    c = S.aliased_blocks()
    cap, n = c["cap"], len(c["iq"])
    m = knn.Matcher(cap, kernel=kernel)
    try:
        d_buf, d_nq, d_nt = _up(c["buf"]), _up(c["nq"]), _up(c["nt"])
        for k in ((2,) if kernel == "valu" else (1, 3)):
            d_out = _filled(n * cap * k * 8)
            _lib.check(L.hm_knn_batch_device(m.handle, d_buf.data_ptr(), d_nq.data_ptr(), d_buf.data_ptr(), d_nt.data_ptr(), cap,
                                             _u32p(c["iq"]), _u32p(c["it"]), n, k, d_out.data_ptr(), _wait()), "knn_batch, aliased")
            _lib.check(L.hm_sync(m.handle), "hm_sync")
            got = _down(d_out, S.NB, (n, cap, k))
            for p, (a, b) in enumerate(zip(c["iq"], c["it"])):
                q, t = c["buf"][a, :c["nq"][a]], c["buf"][b, :c["nt"][b]]
                _check_case(got[p, :len(q)], q, t, k, None, f"{kernel}: block {a} ({len(q)} queries) -> block {b} ({len(t)} targets), k {k}")
        h = S.aliased_codebook()
        cap, ncw = h["cap"], h["n_codewords"]
        d_buf, d_counts = _up(h["buf"]), _up(h["counts"])
        d_hash, d_words = _filled(2 * ncw // 8), _filled(2 * cap * 8)
        _lib.check(L.hm_hash_bag_device(m.handle, d_buf.data_ptr(), d_counts.data_ptr(), cap, 2, d_buf.data_ptr(), ncw, d_hash.data_ptr(),
                                        d_words.data_ptr(), _wait()), "hash_bag_device, aliased")
        _lib.check(L.hm_sync(m.handle), "hm_sync")
        gh, gw = _down(d_hash, np.uint8, (2, ncw // 8)), _down(d_words, S.NB, (2, cap))
        for f in range(2):
            nf = int(h["counts"][f])
            wh, wi, wd = S.hash_bag(h["buf"][f, :nf], h["buf"][0, :ncw])
            assert np.array_equal(gh[f], wh), (kernel, f)
            assert np.array_equal(gw[f, :nf]["index"], wi) and np.array_equal(gw[f, :nf]["distance"], wd), (kernel, f)
    finally:
        m.close()


@lru_cache(maxsize=None)
def _pair_answer(*case):
    return T.pair_case_answer(*case)


@pytest.mark.parametrize("na,kind,rule,pu,pf,sym", T.PAIR_CASES)
def test_pairs_catalogue_through_hm_match(gpu, na, kind, rule, pu, pf, sym):
    _, knn = gpu
    from cv_amd import _lib
    c, want = _pair_answer(na, kind, rule, pu, pf, sym)
    m = knn.Matcher(na)
    try:
        got = m.match(c["a"], c["b"], rule, pu, pf, sym)
        assert np.array_equal(got, want), (len(got), len(want))
        # a list shorter than the answer: the status says so, n_out is the full count, the first cap pairs are the answer's
        for cap in (1, len(want) - 1, 1023 if len(want) > 1024 else len(want) // 2):
            pairs = np.full((cap + 4, 2), 0xFFFFFFFF, np.uint32)
            n = C.c_uint32(77)
            st = _lib.lib().hm_match(m.handle, c["a"].ctypes.data, na, c["b"].ctypes.data, len(c["b"]), rule, pu, pf, int(sym),
                                     pairs.ctypes.data, cap, C.byref(n))
            assert st == -4 and n.value == len(want), (cap, st, n.value)          # AKZ_E_CAPACITY
            assert np.array_equal(pairs[:cap], want[:cap]) and (pairs[cap:] == 0xFFFFFFFF).all(), cap
    finally:
        m.close()


RULE_SETS = sorted({case[1:] for case in T.PAIR_CASES})


@pytest.mark.parametrize("kind,rule,pu,pf,sym", RULE_SETS)
def test_pairs_catalogue_through_hm_match_batch_device(gpu, kind, rule, pu, pf, sym):
    """The four query counts as four problems of one call (blocks of 2 049 rows), plus one problem that pairs the longest a
    block with an EMPTY b block: the guard."""
    _, knn = gpu
    from cv_amd import _lib
    L = _lib.lib()
    cap, n = max(S.PAIR_COUNTS), len(S.PAIR_COUNTS)
    answers = [_pair_answer(na, kind, rule, pu, pf, sym) for na in S.PAIR_COUNTS]
    a = np.full((n, cap, 64), 0x5A, np.uint8); b = np.full((n + 1, cap, 64), 0xA5, np.uint8)
    for p, (c, _) in enumerate(answers):
        a[p, :len(c["a"])] = c["a"]; b[p, :len(c["b"])] = c["b"]
    d_a, d_b = _up(a), _up(b)
    d_na = _up(np.array(S.PAIR_COUNTS, np.int32)); d_nb = _up(np.array([len(c["b"]) for c, _ in answers] + [1], np.int32))
    ia = np.array(list(range(n)) + [n - 1], np.uint32); ib = np.arange(n + 1, dtype=np.uint32)
    d_pairs, d_n = _filled((n + 1) * cap * 8), _filled((n + 1) * 4)
    m = knn.Matcher(cap)
    try:
        _lib.check(L.hm_match_batch_device(m.handle, d_a.data_ptr(), d_na.data_ptr(), d_b.data_ptr(), d_nb.data_ptr(), cap, _u32p(ia), _u32p(ib),
                                           n + 1, rule, pu, pf, int(sym), d_pairs.data_ptr(), d_n.data_ptr(), _wait()), "match_batch")
        _lib.check(L.hm_sync(m.handle), "hm_sync")
    finally:
        m.close()
    gp, gn = _down(d_pairs, np.uint32, (n + 1, cap, 2)), _down(d_n, np.uint32, (n + 1,))
    for p, (c, want) in enumerate(answers):
        assert gn[p] == len(want), (p, gn[p], len(want))
        assert np.array_equal(gp[p, :gn[p]], want) and (gp[p, gn[p]:] == 0xFFFFFFFF).all(), p
    assert gn[n] == 0 and (gp[n] == 0xFFFFFFFF).all()                             # fewer than two on a side: no pairs


@pytest.mark.parametrize("n_views,k,better_by", T.BOV_CASES)
def test_best_of_views_catalogue(gpu, n_views, k, better_by):
    """Two scripted frames (300 and 123 features, their own views and landmark tables) through the batched entry point, and
    each through the single-frame one."""
    _, knn = gpu
    from cv_amd import _lib
    L = _lib.lib()
    frames = [S.best_of_views_case(n_views, k, better_by=better_by, seed=s) for s in (0, 1)]
    nqs = [300, 123]
    cap, nblk = frames[0]["cap"], n_views + 2
    landmarks = np.concatenate([c["landmarks"] for c in frames])
    counts = np.concatenate([c["counts"] for c in frames])
    views = np.stack([c["view_sel"] + f * nblk for f, c in enumerate(frames)]).astype(np.uint32)
    nb = np.stack([c["nb"] for c in frames])
    want = [S.best_of_views(c["nb"], nq, landmarks, views[f], counts, better_by) for f, (c, nq) in enumerate(zip(frames, nqs))]
    T.check_bov_scenarios(frames[0], *want[0])
    d_knn, d_lm, d_counts = _up(nb), _up(landmarks), _up(counts)
    d_nq = _up(np.array([7] + nqs, np.int32))                                      # frame f's count is d_nq[iq[f]], iq = (1, 2)
    m = knn.Matcher(cap)
    try:
        d_best, d_dec = _filled(2 * cap * 3 * 8, 0xEE), _filled(2 * cap * 4, 0xEE)
        _lib.check(L.hm_best_of_views_batch_device(m.handle, d_knn.data_ptr(), d_nq.data_ptr(), _u32p([1, 2]), cap, _u32p(views), 2, n_views, k,
                                                   d_lm.data_ptr(), d_counts.data_ptr(), better_by, d_best.data_ptr(), d_dec.data_ptr(), _wait()),
                   "best_of_views_batch")
        _lib.check(L.hm_sync(m.handle), "hm_sync")
        gb, gd = _down(d_best, np.uint32, (2, cap, 3, 2)), _down(d_dec, np.uint32, (2, cap))
        for f, nq in enumerate(nqs):
            assert np.array_equal(gb[f, :nq], want[f][0]) and np.array_equal(gd[f, :nq], want[f][1]), f
            assert (gd[f, nq:] == 0xEEEEEEEE).all() and (gb[f, nq:] == 0xEEEEEEEE).all()
            d_b1, d_d1 = _filled(cap * 3 * 8, 0xEE), _filled(cap * 4, 0xEE)
            _lib.check(L.hm_best_of_views_device(m.handle, d_knn[f * n_views * cap * k * 8:].data_ptr(), d_nq[4 * (f + 1):].data_ptr(), cap,
                                                 _u32p(views[f]), n_views, k, d_lm.data_ptr(), d_counts.data_ptr(), better_by,
                                                 d_b1.data_ptr(), d_d1.data_ptr(), _wait()), "best_of_views")
            _lib.check(L.hm_sync(m.handle), "hm_sync")
            assert np.array_equal(_down(d_b1, np.uint32, (cap, 3, 2)), gb[f]) and np.array_equal(_down(d_d1, np.uint32, (cap,)), gd[f]), f
    finally:
        m.close()


def test_landmark_pairs_catalogue(gpu):
    """Three frames of 8 192 features — the set at its load factor of one half with chains that wrap, the overflowing sums, the
    mixed frame — through the four landmark entry points, under each frame's observation counts."""
    _, knn = gpu
    from cv_amd import _lib
    L = _lib.lib()
    kinds, cap = ("full", "counts", "mixed"), 8192
    cases = [S.landmark_case(kind, cap) for kind in kinds]
    F, n_world = len(cases), cases[0]["n_world"]
    world = np.ones((n_world + F * cap, 4), np.float64)
    for f, c in enumerate(cases):
        world[n_world + f * cap:n_world + (f + 1) * cap, 3] = np.where(c["world_ok"], 0.0, -1.0)
    world[:n_world, 3] = np.where(cases[2]["world_lm"], 1.0, -1.0)
    state = lambda f, **kw: S.landmark_pairs(cases[f]["best"], cases[f]["decision"], kw.pop("merge_ok", cases[f]["merge_ok"]),
                                             kw.pop("world", world), n_world, n_world + f * cap, **kw)
    for f, kind in enumerate(kinds):
        own = cases[f]["obs"]
        T.check_landmark_scenarios(kind, cases[f], state(f), state(f, obs_counts=own), state(f, world=None, obs_counts=own))
    d_best = _up(np.stack([c["best"] for c in cases])); d_dec = _up(np.stack([c["decision"] for c in cases]))
    d_ok = _up(np.stack([c["merge_ok"] for c in cases])); d_world = _up(world)
    d_nq = _up(np.full(F, cap, np.int32)); iq = np.arange(F, dtype=np.uint32)
    m = knn.Matcher(cap)

    def run(call, *head_tail):
        d_pairs, d_np = _filled(F * cap * 8), _filled(F * 4)
        head, tail = head_tail
        _lib.check(call(m.handle, d_best.data_ptr(), d_dec.data_ptr(), *head, d_nq.data_ptr(), _u32p(iq), cap, F, *tail,
                        d_pairs.data_ptr(), d_np.data_ptr(), _wait()), call.__name__)
        _lib.check(L.hm_sync(m.handle), "hm_sync")
        return _down(d_pairs, np.uint32, (F, cap, 2)), _down(d_np, np.uint32, (F,))

    def same(got, f, want, what):
        gp, gn = got
        assert gn[f] == len(want), (what, f, gn[f], len(want))
        assert np.array_equal(gp[f, :gn[f]], want), (what, f)
        assert (gp[f, gn[f]:] == 0xFFFFFFFF).all(), (what, f)

    try:
        plain = run(L.hm_landmark_matches_batch_device, (d_ok.data_ptr(),), (d_world.data_ptr(), n_world))
        nomask = run(L.hm_landmark_pairs_batch_device, (), (d_world.data_ptr(), n_world))
        for f in range(F):
            same(plain, f, state(f), "matches")
            same(nomask, f, state(f, merge_ok=None), "pairs")
        for j in range(F):                                   # one table of observation counts per call: each case's own, on all frames
            d_obs = _up(cases[j]["obs"])
            ordered = run(L.hm_landmark_matches_ordered_batch_device, (d_ok.data_ptr(), d_obs.data_ptr()), (d_world.data_ptr(), n_world))
            original = run(L.hm_landmark_original_matches_batch_device, (d_ok.data_ptr(), d_obs.data_ptr()), (n_world,))
            for f in range(F):
                same(ordered, f, state(f, obs_counts=cases[j]["obs"]), f"ordered, counts of {kinds[j]}")
                same(original, f, state(f, world=None, obs_counts=cases[j]["obs"]), f"original, counts of {kinds[j]}")
    finally:
        m.close()


@pytest.mark.parametrize("n_codewords", S.CODEWORD_COUNTS)
def test_hash_bag_catalogue(gpu, n_codewords):
    """Bags of 0, 1 and cap = 70 features: hm_hash_bag one by one, hm_hash_bag_device as three frames of one call — through the
    default kernel and the int8 one (the launch follows the context's kernel switch)."""
    _, knn = gpu
    from cv_amd import _lib
    L = _lib.lib()
    cap, ns = 70, (0, 1, 70)
    cases = [S.hash_bag_case(n_codewords, n) for n in ns]
    cw = cases[2]["codewords"]
    want = [S.hash_bag(c["features"], cw) for c in cases]
    blocks = np.full((3, cap, 64), 0x5A, np.uint8)
    for f, c in enumerate(cases):
        blocks[f, :ns[f]] = c["features"]
    for kernel in ("fp4", "int8"):
        m = knn.Matcher(max(n_codewords, cap), kernel=kernel)
        try:
            for f, n in enumerate(ns):
                h = np.full(n_codewords // 8, 0xFF, np.uint8); words = np.zeros(max(n, 1), S.NB)
                feats = np.ascontiguousarray(blocks[f, :max(n, 1)])
                _lib.check(L.hm_hash_bag(m.handle, feats.ctypes.data, n, cw.ctypes.data, n_codewords, h.ctypes.data, words.ctypes.data), "hm_hash_bag")
                assert np.array_equal(h, want[f][0]), (kernel, n)
                assert np.array_equal(words[:n]["index"], want[f][1]) and np.array_equal(words[:n]["distance"], want[f][2]), (kernel, n)
            d_blocks, d_counts, d_cw = _up(blocks), _up(np.array(ns, np.int32)), _up(cw)
            d_hash, d_words = _filled(3 * n_codewords // 8), _filled(3 * cap * 8)
            _lib.check(L.hm_hash_bag_device(m.handle, d_blocks.data_ptr(), d_counts.data_ptr(), cap, 3, d_cw.data_ptr(), n_codewords,
                                            d_hash.data_ptr(), d_words.data_ptr(), _wait()), "hm_hash_bag_device")
            _lib.check(L.hm_sync(m.handle), "hm_sync")
            gh, gw = _down(d_hash, np.uint8, (3, n_codewords // 8)), _down(d_words, S.NB, (3, cap))
            for f, n in enumerate(ns):
                assert np.array_equal(gh[f], want[f][0]), (kernel, n)
                assert np.array_equal(gw[f, :n]["index"], want[f][1]) and np.array_equal(gw[f, :n]["distance"], want[f][2]), (kernel, n)
        finally:
            m.close()


@pytest.mark.parametrize("hash_bytes", S.HASH_BYTES)
def test_hash_knn_catalogue(gpu, hash_bytes):
    _, knn = gpu
    from cv_amd import _lib
    L = _lib.lib()
    m = knn.Matcher(16)
    try:
        for n in S.HASH_COUNTS:
            for kind in ("random", "equal"):
                c = S.hash_knn_case(hash_bytes, n, kind)
                for k in (1, 3, n, n + 5):
                    idx, dist = S.hash_knn(c["query"], c["hashes"], k)
                    out = np.full(k + 2, 0xFFFFFFFF, np.uint64).view(S.NB); n_out = C.c_uint32(77)
                    _lib.check(L.hm_hash_knn(m.handle, c["query"].ctypes.data, c["hashes"].ctypes.data, n, hash_bytes, k, out.ctypes.data,
                                             C.byref(n_out)), "hm_hash_knn")
                    assert n_out.value == len(idx) == min(k, n), (hash_bytes, n, kind, k)
                    assert np.array_equal(out[:len(idx)]["index"], idx) and np.array_equal(out[:len(idx)]["distance"], dist), (hash_bytes, n, kind, k)
                    assert (out[len(idx):]["index"] == 0xFFFFFFFF).all()
                    if kind == "equal":
                        assert idx.tolist() == list(range(min(k, n)))                  # insertion order
    finally:
        m.close()


# ---- the host half: the timing pool, scratch that grows and is reused, the staging ring past one turn ----------------------
# Descriptor blocks hold 65 queries x 193 targets unless stated: 65 = two column blocks of the wide kernel plus one query,
# 193 = one tile past the three-stage ring — the smallest sizes that cross every boundary of all four kernels.

def _near_copies(rng, a, nb):
    """nb random rows with row 3 * i a near copy of a[i] (2 bits away) wherever it fits: pairs that every rule accepts."""
    b = S.random_rows(rng, nb)
    for i in range(min(len(a), nb // 3)):
        b[3 * i] = S.flip(a[i], [i % 512, (i + 200) % 512])
    return b


def _timing(L, m, reset=0):
    from cv_amd import _lib
    ms, n = C.c_double(-1.0), C.c_uint64(77)
    _lib.check(L.hm_timing_get(m.handle, C.byref(ms), C.byref(n), reset), "hm_timing_get")
    return ms.value, n.value


@pytest.mark.parametrize("kernel", ["fp4", "fp4_regs", "int8", "valu"])
def test_timing_counts_the_knn_launches(gpu, kernel):
    """hm_timing_enable / hm_timing_get (bench.py's MFMA roofline rests on them): three hm_knn calls (k = 1, 2, 3) and one
    symmetric hm_match are four k-NN launches (the two directions of a match are two problems of ONE launch), a finite time
    above zero, and answers equal to the statement.  A read with reset leaves 0 launches and 0.0 ms; with timing off nothing is
    counted.  The VALU switch: its kernel exists for k = 2 only and its branch of launch_knn returns before the events are
    taken, so the k = 2 search and the match go uncounted; k = 1 and k = 3 run (and are counted) on the FP4 kernel: 2."""
    _, knn = gpu
    from cv_amd import _lib
    L = _lib.lib()
    rng = S._rng(69, 1)
    q, t = S.random_rows(rng, 65), S.random_rows(rng, 193)
    b = _near_copies(rng, q, 193)
    want_pairs = S.match(q, b, S.RULE_STRICT, 24, 0.5, True)
    assert len(want_pairs) >= 60
    m = knn.Matcher(193, kernel=kernel)
    try:
        assert _timing(L, m) == (0.0, 0)
        _lib.check(L.hm_timing_enable(m.handle, 1), "hm_timing_enable")
        for k in (1, 2, 3):
            _check_case(m.knn(q, t, k), q, t, k, None, f"{kernel}, timed: k {k}")
        assert np.array_equal(m.match(q, b, S.RULE_STRICT, 24, 0.5, True), want_pairs)
        ms, n = _timing(L, m)
        assert n == (2 if kernel == "valu" else 4), (kernel, n)
        assert np.isfinite(ms) and ms > 0.0, (kernel, ms)
        assert _timing(L, m, reset=1) == (ms, n)                                   # nothing new: the same sums, then cleared
        assert _timing(L, m) == (0.0, 0)
        _lib.check(L.hm_timing_enable(m.handle, 0), "hm_timing_enable")
        _check_case(m.knn(q, t, 3), q, t, 3, None, f"{kernel}, untimed")
        assert _timing(L, m) == (0.0, 0)
    finally:
        m.close()


def test_scratch_grows_and_is_reused(gpu):
    """Every grow-only scratch of the context through small, large, small on one fresh Matcher: the k-NN lists and the recoded
    blocks (hm_knn, then hm_set_targets + hm_knn_targets — once more on a second fresh context, where the resident path does the
    growing), the place-recognition scratch (hm_hash_knn), the batched lists (hm_match_batch_device — on that Matcher, whose
    lists are large by then, and on a third fresh context of capacity 64, where the batched path does the growing)."""
    _, knn = gpu
    from cv_amd import _lib
    L = _lib.lib()
    rng = S._rng(69, 2)
    t = S.random_rows(rng, 193)
    qs = {n: S.random_rows(rng, n) for n in (40, 1500)}
    for n in qs:
        qs[n][::7] = t[(np.arange(len(qs[n][::7])) * 5) % 193]                      # exact copies: distance 0, and ties among queries
    want = {n: S.knn(qs[n], t, 3) for n in qs}
    m, m2, m3 = knn.Matcher(2048), knn.Matcher(2048), knn.Matcher(64)
    try:
        for n in (40, 1500, 40):
            S.check_neighbors(m.knn(qs[n], t, 3), *want[n], S.ABI_ABSENT, f"hm_knn, {n} queries")
        for mm in (m, m2):
            mm.set_targets(t)
            for n in (40, 1500, 40):
                S.check_neighbors(mm.knn_targets(qs[n], 3), *want[n], S.ABI_ABSENT, f"hm_knn_targets, {n} queries")
        hashes = rng.integers(0, 256, (300, 64), dtype=np.uint8)
        hashes[299] = hashes[2]; hashes[7] = hashes[2]                              # ties, inside the short store as well
        query = S.flip(hashes[2], [0, 77, 511])
        for n in (8, 300, 8):
            idx, dist = S.hash_knn(query, hashes[:n], 5)
            out = np.full(5, 0xFFFFFFFF, np.uint64).view(S.NB); n_out = C.c_uint32(77)
            stored = np.ascontiguousarray(hashes[:n])
            _lib.check(L.hm_hash_knn(m.handle, query.ctypes.data, stored.ctypes.data, n, 64, 5, out.ctypes.data, C.byref(n_out)), "hm_hash_knn")
            assert n_out.value == 5 and np.array_equal(out["index"], idx) and np.array_equal(out["distance"], dist), n
            assert idx[0] == 2 and idx[1] == 7 and dist[0] == dist[1] == 3
        cap, nblk = 64, 5
        counts = np.array([64, 33, 2, 50, 1], np.int32)                             # (the last: fewer than two on a side, no pairs)
        a = np.full((nblk, cap, 64), 0x5A, np.uint8); bb = np.full((nblk, cap, 64), 0xA5, np.uint8)
        for blk in range(nblk):
            a[blk, :counts[blk]] = S.random_rows(rng, counts[blk])
            bb[blk, :counts[4 - blk]] = _near_copies(rng, a[blk, :counts[blk]], counts[4 - blk])
        d_a, d_b, d_na, d_nb = _up(a), _up(bb), _up(counts), _up(counts[::-1].copy())
        total = 0
        for mm in (m, m3):
            for ia, ib in (([1], [1]), ([0, 1, 2, 3, 4], [0, 1, 2, 3, 4]), ([3], [3])):
                n = len(ia)
                d_pairs, d_n = _filled(n * cap * 8), _filled(n * 4)
                _lib.check(L.hm_match_batch_device(mm.handle, d_a.data_ptr(), d_na.data_ptr(), d_b.data_ptr(), d_nb.data_ptr(), cap, _u32p(ia), _u32p(ib),
                                                   n, S.RULE_STRICT, 24, 0.5, 1, d_pairs.data_ptr(), d_n.data_ptr(), _wait()), "match_batch")
                _lib.check(L.hm_sync(mm.handle), "hm_sync")
                gp, gn = _down(d_pairs, np.uint32, (n, cap, 2)), _down(d_n, np.uint32, (n,))
                for p, (x, y) in enumerate(zip(ia, ib)):
                    wp = S.match(a[x, :counts[x]], bb[y, :counts[4 - y]], S.RULE_STRICT, 24, 0.5, True)
                    assert gn[p] == len(wp) and np.array_equal(gp[p, :gn[p]], wp) and (gp[p, gn[p]:] == 0xFFFFFFFF).all(), (n, p, gn[p], len(wp))
                    total += len(wp)
        assert total >= 80                                                         # the pairs are there to be found
    finally:
        m.close()
        m2.close()
        m3.close()


@pytest.mark.parametrize("times", [1, 8])
def test_staging_ring_past_one_turn_with_a_slot_regrown(gpu, times):
    """Six hm_knn_batch_device calls on a fresh context with no host wait in between, each into its own output slab: the ring
    of four staging slots goes round once and a half.  The calls hold 1, 1, 1, 1, n, 1 problems, n the first count whose
    descriptors (knn_stage_bytes: a 56-byte HmProbX and two 32-byte HmExpandJobs per problem, each table padded to 64, plus
    256) no longer fit what the slot got at its first use (twice the bytes of one problem, rounded up to 4 096): the fifth call
    regrows the slot of the first, whose kernels may still be running.  The two sizes and the slot's growth rule are restated
    here — a test cannot read them from the library —, so n = 33 is the boundary only while hm_match.hip keeps them; the
    second case takes eight times that count (264 problems, 31 936 bytes), which regrows the slot under any layout near it."""
    _, knn = gpu
    from cv_amd import _lib
    L = _lib.lib()
    up64 = lambda x: (x + 63) // 64 * 64
    stage = lambda n: up64(56 * n) + up64(32 * 2 * n) + 256
    first = (2 * stage(1) + 4095) // 4096 * 4096
    n_big = next(n for n in range(1, 1000) if stage(n) > first)
    assert (first, n_big) == (4096, 33) and stage(n_big - 1) <= first < stage(n_big)
    cap, nblk, k = 64, 4, 3
    rng = S._rng(69, 3)
    counts = np.array([64, 33, 1, 50], np.int32)
    blocks = np.full((nblk, cap, 64), 0x5A, np.uint8)
    for blk in range(nblk):
        blocks[blk, :counts[blk]] = S.random_rows(rng, counts[blk])
    blocks[1, :20] = blocks[0, 40:60]                                               # distance 0 across blocks, ties inside
    blocks[3, 10:14] = blocks[0, 7]
    answer = {(x, y): S.knn(blocks[x, :counts[x]], blocks[y, :counts[y]], k) for x in range(nblk) for y in range(nblk)}
    calls = []
    for c, n in enumerate((1, 1, 1, 1, n_big * times, 1)):
        iq = np.array([(c + p) % nblk for p in range(n)], np.uint32)
        it = np.array([(c + p // nblk + 1) % nblk for p in range(n)], np.uint32)
        calls.append((iq, it, _filled(n * cap * k * 8)))
    d_blocks, d_counts = _up(blocks), _up(counts)
    m = knn.Matcher(cap)
    try:
        wait = _wait()
        for iq, it, d_out in calls:
            _lib.check(L.hm_knn_batch_device(m.handle, d_blocks.data_ptr(), d_counts.data_ptr(), d_blocks.data_ptr(), d_counts.data_ptr(), cap,
                                             _u32p(iq), _u32p(it), len(iq), k, d_out.data_ptr(), wait), "knn_batch")
        _lib.check(L.hm_sync(m.handle), "hm_sync")
        for c, (iq, it, d_out) in enumerate(calls):
            got = _down(d_out, S.NB, (len(iq), cap, k))
            for p, (x, y) in enumerate(zip(iq, it)):
                S.check_neighbors(got[p, :counts[x]], *answer[x, y], S.ABI_ABSENT, f"call {c}, problem {p}: block {x} -> block {y}")
                assert (got[p, counts[x]:]["index"] == 0xFFFFFFFF).all(), (c, p)
    finally:
        m.close()
