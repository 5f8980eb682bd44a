"""The C restatements of the matcher stage (oracle/match_oracle.c, oracle/lsh_oracle.c) held to the independent numpy /
Python statement (tests/matching_statement.py) on its catalogue of designed inputs and on one random sweep: every index,
distance, pair, decision and hash byte equal.  Where an input's answer is known without a search (the ladders, the one-bit
probes, the ties, the extremes beside the sentinel) the statement is held to that closed form first, so a statement that
was wrong in the oracle's way would still fail."""
import numpy as np
import pytest

import matching_statement as S

KNN_CASES = S.knn_cases()


def _oracle_knn(O, q, t, k):
    return O.knn(q, t, k) if len(t) else S.as_neighbors(*S.knn(q, t, k), S.ORACLE_ABSENT)


def test_the_two_forms_of_the_statement_agree():
    """The sorted form of knn() and the crate's insertion procedure, on small problems full of equal distances."""
    rng = np.random.default_rng(5)
    for trial in range(120):
        nq, nt, k = int(rng.integers(1, 4)), int(rng.integers(0, 12)), int(rng.integers(1, 5))
        base = S.random_rows(rng, 1)[0]
        rows = lambda n: np.stack([S.flip(base, rng.permutation(512)[:rng.integers(0, 4)]) for _ in range(n)]) if n else np.zeros((0, 64), np.uint8)
        q, t = rows(nq), rows(nt)
        a, b = S.knn(q, t, k), S.knn_literal(q, t, k)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), trial
        assert np.array_equal(S.hamming(q, t), [[int(np.unpackbits(x ^ y).sum()) for y in t] for x in q] if nt else np.zeros((nq, 0)))


@pytest.mark.parametrize("case", KNN_CASES, ids=[c[0] for c in KNN_CASES])
def test_knn_catalogue(oracle, case):
    name, q, t, closed = case
    for k in (1, 2, 3):
        idx, dist = S.knn(q, t, k)
        cidx, cdist, mask = closed(k)
        assert np.array_equal(idx[mask], cidx[mask]) and np.array_equal(dist[mask], cdist[mask]), (name, k, "statement vs closed form")
        assert ((idx >= 0).sum(axis=1) == min(k, len(t))).all()                      # absent exactly in the slots past nt
        S.check_neighbors(oracle.knn(q, t, k), idx, dist, S.ORACLE_ABSENT, f"{name}, k {k}")
    if len(t) >= 2:
        S.check_neighbors(oracle.knn2(q, t), *S.knn(q, t, 2), S.ORACLE_ABSENT, f"{name}, knn2")


def test_knn_catalogue_reaches_what_it_was_built_for():
    d_seen = set()
    for name, q, t, closed in KNN_CASES:
        d_seen |= set(np.unique(S.hamming(q, t)).tolist())
    assert d_seen == set(range(513))                                                 # every distance 0..512 occurs
    pad = np.zeros(64, np.uint8); pad[60] = 0xC0; pad[61:] = 0xFF                    # bits 486..511
    assert any((t & pad).any() for _, _, t, _ in KNN_CASES)
    c = S.one_bit_probes(0)
    assert (S.hamming(c["q"], c["t"][:1]) == 1).all()


def test_largest_admitted_target_set(oracle):
    c = S.largest_target_set()
    assert len(c["t"]) == (1 << 21) - 1 and len(c["q"]) <= 4
    assert c["idx"][0].tolist() == [p for p, _ in S.LARGEST_PLANTS[:3]] and c["dist"][0].tolist() == [0, 1, 1]
    assert int(S.hamming(c["q"][:1], c["t"][1048575:1048576])[0, 0]) == 2
    assert c["dist"][1:].min() > 150 and c["idx"].max() > (1 << 20)                 # the background keeps its natural distances
    S.check_neighbors(oracle.knn(c["q"], c["t"], 3), c["idx"], c["dist"], S.ORACLE_ABSENT, "2^21 - 1 targets")


def test_aliased_blocks(oracle):
    c = S.aliased_blocks()
    differ = 0
    for a, b in zip(c["iq"], c["it"]):
        q, t = c["buf"][a, :c["nq"][a]], c["buf"][b, :c["nt"][b]]
        for k in (1, 3):
            S.check_neighbors(oracle.knn(q, t, k), *S.knn(q, t, k), S.ORACLE_ABSENT, f"blocks {a} -> {b}, k {k}")
        # the failure the case is built for: the answer over the OTHER side's count is a different one
        differ += not np.array_equal(S.knn(q, t, 1)[0], S.knn(q, c["buf"][b, :c["nq"][b]], 1)[0])
    assert differ >= 3
    c = S.aliased_codebook()
    for f in range(2):
        feats, cw = c["buf"][f, :c["counts"][f]], c["buf"][0, :c["n_codewords"]]
        h, wi, wd = S.hash_bag(feats, cw)
        oh, ow = oracle.hash_bag(feats, cw)
        assert np.array_equal(oh, h) and np.array_equal(ow["index"], wi) and np.array_equal(ow["distance"], wd)
    assert (wi[:20] >= 5).all() and (wd[:20] == 0).all()


PAIR_CASES = [(na, kind, rule, pu, pf, sym) for na in S.PAIR_COUNTS for kind, rule, pu, pf, sym in (
    ("better_by", S.RULE_STRICT, 24, 0.0, False), ("better_by", S.RULE_BETTER_BY, 24, 0.0, False),
    ("better_by", S.RULE_BETTER_BY, 24, 0.0, True), ("lowe", S.RULE_LOWE, 0, 0.5, False), ("twins", S.RULE_BETTER_BY, 0, 0.0, True))]


def pair_case_answer(na, kind, rule, pu, pf, sym):
    """The case, the statement's pairs, and the checks that the case reaches what it was built for."""
    c = S.pairs_case(na, kind, pu)
    fi, fd = S.knn(c["a"], c["b"], 2)
    assert np.array_equal(fd[:, 0], c["d0"]) and np.array_equal(fd[:, 1], c["d1"])    # the scripted distances are the real ones
    want = S.match(c["a"], c["b"], rule, pu, pf, sym)
    fwd = np.array([S.accept(rule, int(x), int(y), pu, pf) for x, y in zip(c["d0"], c["d1"])])
    if kind == "better_by":
        at_eq = c["d0"] + pu == c["d1"]
        assert at_eq.sum() > na // 5 and (fwd[at_eq] == (rule == S.RULE_BETTER_BY)).all()
        waves = fwd[:na // 64 * 64].reshape(-1, 64).sum(axis=1)
        assert (waves == 0).any() and (waves == 64).any() and ((waves > 0) & (waves < 64)).any()
        assert fwd[:1024].any() and not fwd[:1024].all() and (na <= 1024 or fwd[1024:].any())
    elif kind == "lowe":
        assert not fwd[(c["d0"] == 12) & (c["d1"] == 24)].any() and fwd[(c["d0"] == 11)].all() and fwd[c["d1"] == 25].all()
        assert not fwd[c["d0"] == 13].any()
    else:
        ri, rd = S.knn(c["b"], c["a"], 2)
        kept = set(want[:, 0].tolist())
        dropped_twin = [i for i in range(na) if fwd[i] and i not in kept and rd[fi[i, 0], 0] == fd[i, 0] and ri[fi[i, 0], 0] != i]
        assert len(dropped_twin) >= 200 and len(kept) >= 200             # one twin of every group's nearest pair each
    if not sym:
        assert np.array_equal(want[:, 0], np.flatnonzero(fwd))
    assert 0 < len(want) < na
    return c, want


@pytest.mark.parametrize("na,kind,rule,pu,pf,sym", PAIR_CASES)
def test_pairs_catalogue(oracle, na, kind, rule, pu, pf, sym):
    c, want = pair_case_answer(na, kind, rule, pu, pf, sym)
    assert np.array_equal(oracle.match(c["a"], c["b"], rule, pu, pf, sym), want)


def test_pairs_guard(oracle):
    rng = np.random.default_rng(3)
    for na, nb in ((0, 5), (1, 5), (5, 1), (5, 0), (1, 1)):
        a, b = S.random_rows(rng, na), S.random_rows(rng, nb)
        assert len(S.match(a, b, S.RULE_BETTER_BY, 24, 0.0, True)) == 0
        assert len(oracle.match(a, b, S.RULE_BETTER_BY, 24, 0.0, True)) == 0


BOV_CASES = [(1, 3, 24), (2, 3, 24), (64, 3, 24), (64, 3, 0), (2, 1, 24), (5, 2, 1)]


def check_bov_scenarios(c, best, dec):
    """The scripted scenarios came out as scripted (where the call has the slots for them)."""
    names = np.array(c["names"])
    assert set(np.unique(dec)) == {0, 1, 2} or c["nb"].shape[0] * c["nb"].shape[2] < 3 or c["better_by"] == 0
    if (c["counts"][c["view_sel"]] >= c["nb"].shape[2]).sum() * c["nb"].shape[2] >= 6 and c["nb"].shape[2] == 3:
        first = lambda n: best[np.flatnonzero(names == n)[0]]
        assert first("again_at_0")[:, 1].tolist() == [40, 100, 150] and first("again_at_1")[:, 1].tolist() == [50, 90, 150]
        assert first("again_at_2")[:, 1].tolist() == [50, 100, 140] and first("again_2_to_0")[:, 1].tolist() == [10, 50, 100]
        assert first("again_2_to_1")[:, 1].tolist() == [50, 60, 100] and first("again_1_to_0")[:, 1].tolist() == [49, 50, 150]
        assert first("again_worse")[:, 1].tolist() == [50, 100, 150]
        e = first("equal_keys")
        assert e[:, 1].tolist() == [77] * 3 and e[0, 0] < e[1, 0] < e[2, 0]
        bb = c["better_by"]
        if bb:
            assert (dec[names == "unique_at_equality"] == 1).all() and (dec[names == "unique_below"] != 1).all()
            assert (dec[names == "merge_at_equality"] == 2).all() and (dec[names == "merge_below"] == 0).all()
    two = names == "two_landmarks"
    if c["nb"].shape[0] * c["nb"].shape[2] >= 3:
        assert (dec[two] == 0).all() and (best[two][:, 2, 0] == S.NONE).all() and (best[two][:, 1, 0] != S.NONE).all()
        assert (best[names == "one_landmark"][:, 1, 0] == S.NONE).all()
    assert not (best[:, :, 0] >= 20000).any() or (best[:, :, 0][best[:, :, 0] >= 20000] == S.NONE).all()    # no poison slot was read


@pytest.mark.parametrize("n_views,k,better_by", BOV_CASES)
def test_best_of_views_catalogue(oracle, n_views, k, better_by):
    c = S.best_of_views_case(n_views, k, better_by=better_by)
    best, dec = S.best_of_views(c["nb"], c["nq"], c["landmarks"], c["view_sel"], c["counts"], better_by)
    check_bov_scenarios(c, best, dec)
    obest, odec = oracle.best_of_views(c["nb"], c["nq"], c["landmarks"], c["view_sel"], c["counts"], better_by)
    assert np.array_equal(obest, best) and np.array_equal(odec, dec)


def landmark_answers(kind, cap=8192, merged_base=None):
    """The case, its world table and the statement's three lists: feature order, consensus order, original matches."""
    c = S.landmark_case(kind, cap)
    base = c["n_world"] if merged_base is None else merged_base
    world = S.landmark_world(c, base, base + cap)
    plain = S.landmark_pairs(c["best"], c["decision"], c["merge_ok"], world, c["n_world"], base)
    ordered = S.landmark_pairs(c["best"], c["decision"], c["merge_ok"], world, c["n_world"], base, c["obs"])
    original = S.landmark_pairs(c["best"], c["decision"], c["merge_ok"], None, c["n_world"], base, c["obs"])
    return c, world, plain, ordered, original


def check_landmark_scenarios(kind, c, plain, ordered, original, cap=8192):
    keys = c["best"][:, :2, 0].reshape(-1)
    if kind == "full":
        assert len(set(keys.tolist())) == 2 * cap == S.LM_SLOTS // 2 and 0xFFFFFFFE in keys
        slots = np.array([S.lm_slot(x) for x in keys])
        assert (slots == 32760).sum() == 3000 and (slots == 5).sum() == 1000       # a chain that wraps, computed from the hash
        assert len(plain) == cap and np.array_equal(plain[:, 0], np.arange(cap))
        assert np.array_equal(ordered, plain) and np.array_equal(original, plain)  # all sums equal: feature order stays
    elif kind == "counts":
        obs = c["obs"].astype(np.int64)
        cnt = lambda l: np.where(l < c["n_world"], obs[np.minimum(l, c["n_world"] - 1)], 0)
        sums = cnt(c["best"][:, 0, 0].astype(np.int64)) + cnt(c["best"][:, 1, 0].astype(np.int64))
        assert (sums > 0xFFFFFFFF).sum() > 50 and (sums == 0xFFFFFFFF).sum() > 5   # overflow, and the exact limit
        top = original[:int((sums >= 0xFFFFFFFF).sum()), 0]
        assert np.array_equal(top, np.sort(top)) and (sums[top] >= 0xFFFFFFFF).all() and len(set(sums[top].tolist())) > 2
        assert len(original) == cap and 0 < len(ordered) < cap and not np.array_equal(ordered[:, 0], np.sort(ordered[:, 0]))
    else:
        assert 0 < len(plain) < cap // 2 and (plain[:, 1] >= c["n_world"]).any() and (plain[:, 1] < c["n_world"]).any()
        assert len(original) > len(ordered) == len(plain)
        named = [int(c["best"][i, 0, 0]) for i in range(cap) if c["decision"][i] == 1]
        assert named.count(0xFFFFFFFE) >= 2 or 0xFFFFFFFE in keys


@pytest.mark.parametrize("kind", ["full", "counts", "mixed"])
def test_landmark_pairs_catalogue(oracle, kind):
    c, world, plain, ordered, original = landmark_answers(kind)
    check_landmark_scenarios(kind, c, plain, ordered, original)
    base = c["n_world"]
    kw = dict(merge_ok=c["merge_ok"], n_world=c["n_world"], merged_base=base)
    assert np.array_equal(oracle.landmark_pairs(c["best"], c["decision"], world, **kw), plain)
    assert np.array_equal(oracle.landmark_pairs(c["best"], c["decision"], world, obs_counts=c["obs"], **kw), ordered)
    valid = np.ones_like(world)
    assert np.array_equal(oracle.landmark_pairs(c["best"], c["decision"], valid, obs_counts=c["obs"], **kw), original)
    # without a mask no merge passes
    nomask = S.landmark_pairs(c["best"], c["decision"], None, world, c["n_world"], base)
    assert np.array_equal(oracle.landmark_pairs(c["best"], c["decision"], world, n_world=c["n_world"]), nomask)
    assert (nomask[:, 1] < c["n_world"]).all()


@pytest.mark.parametrize("n_codewords", S.CODEWORD_COUNTS)
def test_hash_bag_catalogue(oracle, n_codewords):
    for n in (0, 1, 70):
        c = S.hash_bag_case(n_codewords, n)
        h, wi, wd = S.hash_bag(c["features"], c["codewords"])
        if n:
            assert wi[0] == 0 and wd[0] == 0 and h[0] & 1
        if n > 8:
            assert wi[1] == n_codewords - 2 and wi[2] == 0 and wi[8] == 0 and wd[8] == 1    # ties: the lowest index
            assert h[(n_codewords - 2) >> 3] & (1 << ((n_codewords - 2) & 7)) and not h[-1] & 0x80
        else:
            assert int(np.unpackbits(h).sum()) == n
        oh, ow = oracle.hash_bag(c["features"], c["codewords"])
        assert np.array_equal(oh, h) and np.array_equal(ow["index"], wi) and np.array_equal(ow["distance"], wd)


@pytest.mark.parametrize("hash_bytes", S.HASH_BYTES)
def test_hash_knn_catalogue(oracle, hash_bytes):
    for n in S.HASH_COUNTS:
        for kind in ("random", "equal"):
            c = S.hash_knn_case(hash_bytes, n, kind)
            for k in (1, 3, n, n + 5):
                idx, dist = S.hash_knn(c["query"], c["hashes"], k)
                assert len(idx) == min(k, n)
                if kind == "equal":
                    assert idx.tolist() == list(range(min(k, n))) and (dist == 1).all()
                else:
                    assert idx[0] == n // 2 and dist[0] == 1
                got = oracle.hash_knn(c["query"], c["hashes"], k)
                assert np.array_equal(got["index"], idx) and np.array_equal(got["distance"], dist), (hash_bytes, n, kind, k)


def test_random_sweep(oracle):
    """A few hundred small random problems through every function: rows a few bits from a handful of centres, so that small
    and equal distances are the rule."""
    rng = np.random.default_rng(0x5EED)
    def rows(n):
        centres = S.random_rows(rng, 3)
        return np.stack([S.flip(centres[rng.integers(0, 3)], rng.permutation(512)[:rng.integers(0, 6)]) for _ in range(n)]) if n else np.zeros((0, 64), np.uint8)
    for trial in range(300):
        nq, nt, k = int(rng.integers(1, 40)), int(rng.integers(1, 70)), int(rng.integers(1, 4))
        q, t = rows(nq), rows(nt)
        S.check_neighbors(oracle.knn(q, t, k), *S.knn(q, t, k), S.ORACLE_ABSENT, f"sweep {trial}")
        if nq >= 2 and nt >= 2:
            rule, pu, sym = int(rng.integers(0, 3)), int(rng.integers(0, 8)), bool(rng.integers(0, 2))
            pf = float(rng.choice([0.5, 0.8, 1.0]))
            assert np.array_equal(oracle.match(q, t, rule, pu, pf, sym), S.match(q, t, rule, pu, pf, sym)), trial
        if trial % 3 == 0:
            n_views, cap = int(rng.integers(1, 6)), nq
            counts = rng.integers(0, cap + 1, n_views + 1).astype(np.int32)
            sel = rng.permutation(n_views + 1)[:n_views].astype(np.uint32)
            nb = np.zeros((n_views, cap, k), S.NB)
            nb["index"] = rng.integers(0, cap, nb.shape); nb["distance"] = rng.integers(0, 12, nb.shape)
            lms = rng.integers(0, 9, (n_views + 1, cap)).astype(np.uint32)
            bb = int(rng.integers(0, 5))
            best, dec = S.best_of_views(nb, nq, lms, sel, counts, bb)
            obest, odec = oracle.best_of_views(nb, nq, lms, sel, counts, bb)
            assert np.array_equal(obest, best) and np.array_equal(odec, dec), trial
            n_world = 12
            world = rng.standard_normal((n_world + nq, 4)); world[rng.random(len(world)) < 0.3, 3] = -1.0
            ok = (rng.random(nq) < 0.7).astype(np.uint8)
            obs = rng.choice(np.array([0, 1, 5, 0xFFFFFFFF, 0xFFFFFFFE], np.uint32), n_world)
            for o in (None, obs):
                want = S.landmark_pairs(best, dec, ok, world, n_world, n_world, o)
                assert np.array_equal(oracle.landmark_pairs(best, dec, world, merge_ok=ok, n_world=n_world, merged_base=n_world, obs_counts=o), want), trial
            ncw = 32 * int(rng.integers(1, 3))
            cw = rows(ncw)
            h, wi, wd = S.hash_bag(q, cw)
            oh, ow = oracle.hash_bag(q, cw)
            assert np.array_equal(oh, h) and np.array_equal(ow["index"], wi) and np.array_equal(ow["distance"], wd), trial
            hb = 4 * int(rng.integers(1, 20))
            hs = rng.integers(0, 4, (int(rng.integers(1, 30)), hb), dtype=np.uint8)
            got = oracle.hash_knn(hs[0], hs, k + 2)
            idx, dist = S.hash_knn(hs[0], hs, k + 2)
            assert np.array_equal(got["index"], idx) and np.array_equal(got["distance"], dist), trial
