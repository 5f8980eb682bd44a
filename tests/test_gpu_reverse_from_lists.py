"""The reverse side of a symmetric match answered from the forward lists (cv_amd/csrc/hm_match.hip: k_decide, k_verify; the
bound: cv_amd/csrc/hm_rule.h) gives the pair lists of the reverse search, element for element: every case below is compared
with oracle.match under the three settings of the switch — auto, search, lists — and under auto with the fallback share set
low enough that the clustered problems take the fallback, each on the four kernel families, for STRICT and BETTER_BY at
param_u 24, 1 and 0 (BETTER_BY 0 has no bound and keeps the search under every setting).

Inputs are bit patterns with exact Hamming distances: rows derived from a random 64-byte base by flipping chosen bits, bases
about 256 bits from each other.  A gadget is one pair (a, b) with d(a, b) = 5 and one rival a' at distance x from b:
  far    a' has two nearer targets (1 and 2 bits away) and does not list b: the explicit-distance walk must find it;
  best   a' lists b first and its own second-best is a random row (far): only the per-target scatter sees it — built with a'
         at the lower and at the higher index, x = 5 is the tie;
  second a' lists b second.
x runs over tau - 1, tau, tau + 1 of every (rule, param_u), so each pair flips exactly at its rule's boundary (checked in
closed form besides the oracle), one step apart for the two rules."""
import ctypes as C
from functools import lru_cache
from itertools import product

import numpy as np
import pytest

import matching_statement as S
from test_gpu_parity import gpu  # noqa: F401  (gpu: the module fixture that builds the library)

pytestmark = pytest.mark.gpu

KERNELS = ["fp4", "fp4_regs", "int8", "valu"]
# (reverse_check, fallback_share_log2): 2^-5 of na * nb is below what the clustered problems ask for (see clustered())
SWITCH = [("auto", 0), ("search", 0), ("lists", 0), ("auto", 5)]
RULES = list(product([S.RULE_STRICT, S.RULE_BETTER_BY], [24, 1, 0]))
D0 = 5
XS = [3, 4, 5, 6, 7, 27, 28, 29, 30]          # tau of d0 = 5 is 29, 6, 5 (STRICT 24, 1, 0) and 28, 5 (BETTER_BY 24, 1)
KINDS = ["far", "best_lo", "best_hi", "second"]


def tau(rule, pu, d0):
    """hm_rule.h in Python: None where the rule keeps the search."""
    if rule == S.RULE_STRICT:
        return min(d0 + pu, 512)
    return min(d0 + pu - 1, 512) if pu >= 1 else None


@lru_cache(maxsize=None)
def gadgets():
    """(a rows, b rows, [(kind, x, index of a, index of b)])"""
    rng = S._rng(71, 0)
    A, B, where = [], [], []
    for kind in KINDS:
        for x in XS:
            base = S.random_rows(rng, 1)[0]
            a, rival = S.flip(base, np.arange(D0)), S.flip(base, 100 + np.arange(x))
            where.append((kind, x, len(A) + (1 if kind == "best_lo" else 0), len(B)))
            A += [rival, a] if kind == "best_lo" else [a, rival]
            B.append(base)
            if kind == "far":
                B += [S.flip(rival, [300]), S.flip(rival, [301, 302])]
            if kind == "second":
                B.append(S.flip(rival, [300]))
    A += list(S.random_rows(rng, 40)); B += list(S.random_rows(rng, 40))
    return np.array(A, np.uint8), np.array(B, np.uint8), where


@lru_cache(maxsize=None)
def planted(n):
    """n rows per side: every third b a near copy of an a, and rivals of assorted distance to those b among the last a rows,
    some with a nearer target of their own."""
    rng = S._rng(71, 1, n)
    a, b = S.random_rows(rng, n), S.random_rows(rng, n)
    for i in range(n // 3):
        b[3 * i] = S.flip(a[i], rng.choice(512, i % 7, replace=False))
    for i in range(0, n // 3, 4):
        a[n - 1 - i] = S.flip(b[3 * i], rng.choice(512, i % 45, replace=False))
        if i % 8 == 0:
            b[3 * i + 1] = S.flip(a[n - 1 - i], [int(rng.integers(512))])
    return a, b


@lru_cache(maxsize=None)
def clustered():
    """300 per side: one tight cluster of 200 (a base with up to three bits flipped: duplicates and near-duplicates, second-best
    distances of 0..6 throughout) and 100 pairs two bits apart.  Every accepted pair of the 100 (tau >= 5) has the 200 cluster
    rows as candidates: at least 100 * 200 distances of na * nb = 90 000 — above a share of 2^-5, below the built-in 1/4."""
    rng = S._rng(71, 2)
    base = S.random_rows(rng, 1)[0]
    a, b = S.random_rows(rng, 300), S.random_rows(rng, 300)
    for i in range(200):
        a[i] = S.flip(base, rng.choice(512, int(rng.integers(0, 4)), replace=False))
        b[i] = S.flip(base, rng.choice(512, int(rng.integers(0, 4)), replace=False))
    b[7] = a[3]; b[8] = a[3]; a[9] = a[3]                      # exact duplicates on both sides
    for i in range(200, 300):
        b[i] = S.flip(a[i], [i, (i + 77) % 512])
    perm = rng.permutation(300)
    return a[perm], b[rng.permutation(300)]


def cases():
    ga, gb, _ = gadgets()
    out = [("gadgets", ga, gb), ("clustered", *clustered())]
    return out + [(f"planted {n}", *planted(n)) for n in (70, 300, 1100)]


@lru_cache(maxsize=None)
def answer(name, rule, pu):
    from oracle import oracle as O
    a, b = next((a, b) for n, a, b in cases() if n == name)
    return np.asarray(O.match(a, b, rule, pu, 0.5, True), np.int64).reshape(-1, 2)


def test_gadgets_flip_at_the_boundary():
    """The oracle's answer on the gadgets is the closed form: (a, b) is a pair iff x > tau(rule, param_u, 5), for the x around
    that tau — the design reaches what it was built for, before any kernel is asked."""
    _, _, where = gadgets()
    seen = set()
    for rule, pu in RULES:
        t = tau(rule, pu, D0)
        if t is None:
            continue
        got = {tuple(p) for p in answer("gadgets", rule, pu).tolist()}
        for kind, x, ia, ib in where:
            if abs(x - t) <= 1:
                assert ((ia, ib) in got) == (x > t), (rule, pu, kind, x, t)
                seen.add((rule, pu, kind, x > t))
    assert len(seen) == 5 * len(KINDS) * 2                     # every bound, every kind, both sides of the boundary


@pytest.mark.parametrize("check,share", SWITCH, ids=[f"{c}{'-share' + str(s) if s else ''}" for c, s in SWITCH])
@pytest.mark.parametrize("kernel", KERNELS)
def test_hm_match_equals_oracle(gpu, kernel, check, share):
    _, knn = gpu
    m = knn.Matcher(1100, kernel=kernel, reverse_check=check, fallback_share_log2=share)
    try:
        for name, a, b in cases():
            for rule, pu in RULES:
                got = m.match(a, b, rule, pu, 0.5, True)
                assert np.array_equal(got, answer(name, rule, pu)), (kernel, check, share, name, rule, pu)
    finally:
        m.close()


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(torch.device("cuda", 0))


@pytest.mark.parametrize("check,share", SWITCH, ids=[f"{c}{'-share' + str(s) if s else ''}" for c, s in SWITCH])
@pytest.mark.parametrize("kernel", KERNELS)
def test_batch_over_one_buffer(gpu, kernel, check, share):
    """Three problems of one hm_match_batch_device call whose two sides are the SAME buffer of four blocks (capacity 320):
    the clustered pair (blocks 0, 1), an ordinary one (block 2 — random rows with near copies of block 0's rows planted —
    against block 0) and a block of ONE row against block 0: no pairs, count 0."""
    import torch
    _, knn = gpu
    from cv_amd import _lib
    L = _lib.lib()
    cap = 320
    ca, cb = clustered()
    rng = S._rng(71, 3)
    w = S.random_rows(rng, 300)
    for i in range(0, 300, 2):
        w[i] = S.flip(ca[i], rng.choice(512, i % 9, replace=False))
    blocks = np.full((4, cap, 64), 0x5A, np.uint8)
    counts = np.array([300, 300, 300, 1], np.int32)
    for k, rows in enumerate((ca, cb, w, w[:1])):
        blocks[k, :len(rows)] = rows
    ia, ib = np.array([0, 2, 3], np.uint32), np.array([1, 0, 0], np.uint32)
    d_blocks, d_counts = _up(blocks), _up(counts)
    m = knn.Matcher(cap, kernel=kernel, reverse_check=check, fallback_share_log2=share)
    try:
        for rule, pu in RULES:
            d_pairs = torch.full((3 * cap * 8,), 0xFF, dtype=torch.uint8, device=d_blocks.device)
            d_n = torch.full((3 * 4,), 0xFF, dtype=torch.uint8, device=d_blocks.device)
            _lib.check(L.hm_match_batch_device(m.handle, d_blocks.data_ptr(), d_counts.data_ptr(), d_blocks.data_ptr(), d_counts.data_ptr(), cap,
                                               ia.ctypes.data_as(C.c_void_p), ib.ctypes.data_as(C.c_void_p), 3, rule, pu, 0.5, 1,
                                               d_pairs.data_ptr(), d_n.data_ptr(), _lib.wait_handle(torch.cuda.current_stream())), "match_batch")
            _lib.check(L.hm_sync(m.handle), "hm_sync")
            gp = d_pairs.cpu().numpy().view(np.uint32).reshape(3, cap, 2)
            gn = d_n.cpu().numpy().view(np.uint32)
            for p in range(3):
                qa, tb = blocks[ia[p], :counts[ia[p]]], blocks[ib[p], :counts[ib[p]]]
                want = _batch_answer(p, rule, pu, qa.tobytes(), tb.tobytes())
                assert gn[p] == len(want), (kernel, check, share, rule, pu, p, gn[p], len(want))
                assert np.array_equal(gp[p, :gn[p]], want) and (gp[p, gn[p]:] == 0xFFFFFFFF).all(), (kernel, check, share, rule, pu, p)
            assert gn[2] == 0
    finally:
        m.close()


@lru_cache(maxsize=None)
def _batch_answer(p, rule, pu, a_bytes, b_bytes):
    from oracle import oracle as O
    a = np.frombuffer(a_bytes, np.uint8).reshape(-1, 64)
    b = np.frombuffer(b_bytes, np.uint8).reshape(-1, 64)
    if len(a) < 2 or len(b) < 2:                               # (the oracle refuses these; cv-sfm returns no matches)
        return np.zeros((0, 2), np.int64)
    return np.asarray(O.match(a, b, rule, pu, 0.5, True), np.int64).reshape(-1, 2)
