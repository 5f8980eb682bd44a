"""The explicit-distance walk of the reverse-from-lists check on the matrix unit (cv_amd/csrc/hm_match.hip: k_verify_mfma, the
FP4 families) at the edges of its shape: the 32-row tile, the 64-row stage, the 512-row segment of the work list, the
1 024-row index window of a grown segment, the 64 pairs of a wave and the 256 of a workgroup.  Every case is compared with
oracle.match and with Matcher(reverse_check="search") on the same input — neither runs the kernel — for the kernels fp4 and
fp4_regs under STRICT and BETTER_BY at param_u 24 and 1, always with reverse_check="lists" so that nothing falls back.

Inputs are bit patterns with exact Hamming distances (matching_statement's random_rows / flip; random rows lie about 256 bits
apart).  A designed pair is (a, b) with d(a, b) = d0 and nothing else near: it is accepted with tau = d0 + param_u (STRICT)
or d0 + param_u - 1 (BETTER_BY).  A FILLER is a query with two targets of its own, 1 and 2 bits away: its second-best
distance is 2, so it is a row of every designed pair's walk, and it is far from every pair's target.  A RIVAL of a pair is a
filler-like query x bits from the pair's target; its own two targets set where it sorts in the walk — (1, 1): second-best
distance 1, the first row; (1, 3): the last.  The pair survives iff x > tau, which test_designs_have_the_closed_form_answer
checks on the oracle alone, on the CPU, before any kernel is asked.  (Under BETTER_BY 1 a filler's own pair is accepted too,
with tau = 1 and an empty walk: those pairs end the accepted list.)"""
import ctypes as C
from functools import lru_cache
from itertools import combinations, islice

import numpy as np
import pytest

import matching_statement as S
from test_gpu_parity import gpu  # noqa: F401  (gpu: the module fixture that builds the library)

KERNELS = ["fp4", "fp4_regs"]
RULES = [(S.RULE_STRICT, 24), (S.RULE_STRICT, 1), (S.RULE_BETTER_BY, 24), (S.RULE_BETTER_BY, 1)]
D0 = 5
FIRST, FILLER, LAST = (1, 1), (1, 2), (1, 3)           # distances of a walk row's own two targets


def tau(rule, pu, d0):
    return min(d0 + pu - (1 if rule == S.RULE_BETTER_BY else 0), 512)


def flip_all(rows, bits):
    """S.flip on every row."""
    out = np.array(rows, np.uint8, copy=True)
    for b in bits:
        out[:, b >> 3] ^= np.uint8(1 << (b & 7))
    return out


@lru_cache(maxsize=None)
def fillers(n):
    f = S.random_rows(S._rng(72, 0, n), n)
    return f, np.concatenate([flip_all(f, [300]), flip_all(f, [301, 302])])


class Design:
    """Rows of both sides and what is known of the answer: `pairs` {(a, b): survives} for the designed pairs."""

    def __init__(self, *key):
        self.rng = S._rng(72, 1, *key)
        self.A, self.B, self.pairs, self.walk_rows = [], [], {}, []

    def pair(self, d0=D0, d1=None):
        """-> (index of a, index of b); d1: a second target at that distance from a (else the nearest random row)"""
        base = S.random_rows(self.rng, 1)[0]
        self.A.append(S.flip(base, np.arange(d0)))
        self.B.append(base)
        at = (len(self.A) - 1, len(self.B) - 1)
        if d1 is not None:
            self.B.append(S.flip(self.A[-1], 200 + np.arange(d1)))
        self.pairs[at] = True
        return at

    def walk_row(self, row, own):
        """a query with two targets of its own at the distances `own` -> its index"""
        self.A.append(np.array(row, np.uint8))
        self.B += [S.flip(row, 300 + np.arange(own[0])), S.flip(row, 320 + np.arange(own[1]))]
        self.walk_rows.append((len(self.A) - 1, len(self.B) - 2, own))
        return len(self.A) - 1

    def rival(self, at, x, own, t, bit=100):
        """a walk row x bits (bit, bit + 1, ...) from the target of pair `at`, whose bound is t: the pair dies iff x <= t"""
        self.pairs[at] = self.pairs[at] and x > t
        return self.walk_row(S.flip(self.B[at[1]], bit + np.arange(x)), own)

    def done(self, n_fillers=0):
        a, b = np.array(self.A, np.uint8).reshape(-1, 64), np.array(self.B, np.uint8).reshape(-1, 64)
        f, ft = fillers(n_fillers) if n_fillers else (np.zeros((0, 64), np.uint8),) * 2
        self.filler_pairs = [(len(a) + i, len(b) + i) for i in range(n_fillers)]
        return np.concatenate([a, f]), np.concatenate([b, ft])

    def closed_form(self, rule, pu):
        """the answer by reasoning: the designed pairs without a rival in reach, and the own pair of every walk row and
        filler that the rule accepts (nothing else is near their targets)"""
        out = [p for p, alive in self.pairs.items() if alive]
        out += [(ia, ib) for ia, ib, own in self.walk_rows if S.accept(rule, own[0], own[1], pu, 0.5)]
        if S.accept(rule, 1, 2, pu, 0.5):
            out += self.filler_pairs
        return np.array(sorted(out), np.int64).reshape(-1, 2)


# ---------------------------------------------------------------------------------------------------- the designs
# every design is a function of its key alone: (name, rule, param_u, ...) -> (a rows, b rows, closed-form answer or None)

TILE_F = (0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129)
SEG_F = (255, 256, 257, 511, 512, 513, 1023, 1024, 1025)
ACCEPTED = (1, 63, 64, 65, 255, 256, 257, 300)


def _edge(rule, pu, n_fillers, dx, own):
    """three pairs and the walk of n_fillers fillers; one rival of the middle pair at tau + dx, sorted by `own`"""
    D = Design(0, rule, pu, n_fillers, dx, *own)
    at = [D.pair() for _ in range(3)][1]
    D.rival(at, tau(rule, pu, D0) + dx, own, tau(rule, pu, D0))
    return D, n_fillers


def _two_segments(rule, pu, n_fillers, dx_first, dx_last):
    """two rivals of one pair, the first and the last row of a walk that spans several segments"""
    D = Design(1, rule, pu, n_fillers, dx_first, dx_last)
    at = [D.pair() for _ in range(2)][0]
    t = tau(rule, pu, D0)
    D.rival(at, t + dx_first, FIRST, t)
    D.rival(at, t + dx_last, LAST, t, bit=150)
    return D, n_fillers


def _accepted(rule, pu, n, dx_first, dx_last):
    """n accepted pairs: the first of the list (the largest tau: d0 = 7) and the last (the smallest: d0 = 3) have a rival at
    their tau + dx, the others (d0 = 5) none; two fillers.  Under BETTER_BY 1 the own pairs of the last one's rival and of the
    fillers are accepted as well (3, behind the designed ones in the list): the designed pairs are that many fewer where n
    allows."""
    extra = 3 if (rule, pu) == (S.RULE_BETTER_BY, 1) and n > 4 else 0
    D = Design(2, rule, pu, n, dx_first, dx_last)
    n -= extra
    ats = [D.pair(7 if i == 0 else 3 if i == n - 1 else D0) for i in range(n)]
    if n == 1:                                                 # one pair is the first and the last: one rival
        D.rival(ats[0], tau(rule, pu, 7) + dx_first, FILLER, tau(rule, pu, 7))
    else:
        D.rival(ats[0], tau(rule, pu, 7) + dx_first, FIRST, tau(rule, pu, 7))
        D.rival(ats[-1], tau(rule, pu, 3) + dx_last, FILLER, tau(rule, pu, 3))
    return D, 2


def _self(rule, pu, n_fillers, dx, dup):
    """P1 (d0 = 5, d1 = 40) and P2 (d0 = 30, d1 = 60) in one block: under param_u 24 the block walks to tau(P2) >= 53 >= d1(P1),
    and P1's own a is the LAST row of P1's walk (the fillers' second-best distance is 2).  dx: None, or a rival of P1 at its
    tau + dx (with P1's a at distance 5 the nearest row, the rival is the second key).  dup: a second query equal to P1's a —
    another query all the same, so both die."""
    D = Design(3, rule, pu, n_fillers, 99 if dx is None else dx, dup)
    p1, p2 = D.pair(5, 40), D.pair(30, 60)
    if dx is not None:
        D.rival(p1, tau(rule, pu, 5) + dx, FILLER, tau(rule, pu, 5))
    if dup:
        D.A.append(D.A[p1[0]].copy())
        D.pairs[p1] = False                                    # (and the copy's pair with the same target dies with it)
    return D, n_fillers - (0 if dx is None else 1)             # the walk: the fillers, the rival, P1's a


def _ties(rule, pu, variant):
    """rival_lo / rival_hi: a rival at exactly d0 (BETTER_BY 1: tau = d0), at the lower / the higher index than a.
    dup_rivals: two equal rivals at tau.  dup_fillers: every filler twice.  dup_targets: the pair's target twice (d0 = d1:
    never accepted)."""
    D = Design(4, rule, pu, *variant.encode())
    t = tau(rule, pu, D0)
    if variant == "rival_lo":
        base = S.random_rows(D.rng, 1)[0]
        D.walk_row(S.flip(base, 100 + np.arange(D0)), FILLER)
        D.A.append(S.flip(base, np.arange(D0))); D.B.append(base)
        D.pairs[(len(D.A) - 1, len(D.B) - 1)] = D0 > t
        D.pair()
    elif variant == "rival_hi":
        D.rival(D.pair(), D0, FILLER, t)
        D.pair()
    elif variant == "dup_rivals":
        at = D.pair()
        r = D.rival(at, t, FILLER, t)
        D.A.append(D.A[r].copy())                              # (shares the first one's targets)
        D.pair()
    elif variant == "dup_fillers":
        at = D.pair()
        D.rival(at, t + 1, LAST, t)
        D.pair()
        a, b = D.done(40)
        return np.concatenate([a, a[-40:]]), np.concatenate([b, b[-80:]]), None
    elif variant == "dup_targets":
        at = D.pair()
        D.B.append(D.B[at[1]].copy())
        D.pairs[at] = False
        D.rival(D.pair(), t, FILLER, t)
    a, b = D.done(40)
    # (the closed form is claimed where it was reasoned: a rival within one step of tau, every row once)
    known = variant in ("rival_hi", "dup_targets") and (variant == "dup_targets" or abs(D0 - t) <= 1)
    return a, b, (D.closed_form(rule, pu) if known else None)


def _grown(rule, pu):
    """The work list under its cap: 4 096 pairs two bits apart (16 blocks) and 4 096 rows that every one of them walks — a base
    row with two bits flipped, against two targets, the base and the base with bit 0 flipped: second-best distance 2 or 3 —
    with 8 208 queries: about 65 800 walk rows against room for 50 segments of 512 (66 units less 16 blocks), so under param_u
    24 and STRICT 1 the segments grow to 1 536 and the kernel takes them in two index windows.  Sixteen pairs over the blocks have a rival, 3 or 25 bits from their target: within
    the bound under param_u 1 or 24."""
    rng = S._rng(72, 5)
    a = S.random_rows(rng, 4096)
    b = a.copy()
    for i in range(4096):
        b[i, (i % 500) >> 3] ^= np.uint8(1 << ((i % 500) & 7))
        b[i, 63] ^= np.uint8(1 << (i % 8))
    c = S.random_rows(rng, 1)[0]
    walk = np.array([S.flip(c, pq) for pq in islice(combinations(range(512), 2), 4096)], np.uint8)
    rivals = [S.flip(b[i], 100 + np.arange(3 if i % 512 == 0 else 25)) for i in range(0, 4096, 256)]
    own = [S.flip(r, [300 + k]) for r in rivals for k in (0, 1)]
    return (np.concatenate([a, walk, np.array(rivals, np.uint8)]),
            np.concatenate([b, c[None, :], S.flip(c, [0])[None, :], np.array(own, np.uint8)]), None)


@lru_cache(maxsize=None)
def design(name, rule, pu, *args):
    if name == "grown":
        return _grown(rule, pu)
    if name == "ties":
        return _ties(rule, pu, *args)
    D, n_fillers = {"edge": _edge, "two_segments": _two_segments, "accepted": _accepted, "self": _self}[name](rule, pu, *args)
    a, b = D.done(n_fillers)
    return a, b, D.closed_form(rule, pu)


def keys(group):
    out = []
    for rule, pu in RULES:
        if group == "tiles":
            out += [("edge", rule, pu, f, dx, own) for f in TILE_F for dx in (-1, 0, 1) for own in (FIRST, LAST)]
        elif group == "segments":
            out += [("edge", rule, pu, f, dx, LAST) for f in SEG_F for dx in (-1, 0, 1)]
            out += [("two_segments", rule, pu, f, d1, d2) for f in (600, 1100) for d1, d2 in ((0, 1), (1, 0), (1, 1))]
        elif group == "accepted":
            out += [("accepted", rule, pu, n, d1, d2) for n in ACCEPTED for d1, d2 in ((0, 0), (0, 1), (1, 0), (1, 1))]
        elif group == "self":
            # (walks of 6 rows, and of 33 and 65: one above a multiple of 32, P1's a last, padding behind it)
            out += [("self", rule, pu, f, dx, dup) for f in (5, 32, 64) for dx, dup in ((None, 0), (0, 0), (1, 0), (None, 1))]
        elif group == "ties":
            out += [("ties", rule, pu, v) for v in ("rival_lo", "rival_hi", "dup_rivals", "dup_fillers", "dup_targets")]
        elif group == "grown":
            out += [("grown", rule, pu)]
    return out


GROUPS = ["tiles", "segments", "accepted", "self", "ties", "grown"]


@lru_cache(maxsize=None)
def answer(key):
    from oracle import oracle as O
    a, b, _ = design(*key)
    return np.asarray(O.match(a, b, key[1], key[2], 0.5, True), np.int64).reshape(-1, 2)


@pytest.mark.parametrize("group", GROUPS[:5])
def test_designs_have_the_closed_form_answer(group):
    """The oracle alone, on the CPU: every design whose answer was reasoned gives exactly that answer — the rival decides at
    x = tau - 1, tau, tau + 1 and nothing else in the design does."""
    claimed = 0
    for key in keys(group):
        _, _, want = design(*key)
        if want is not None:
            assert np.array_equal(answer(key), want), key
            claimed += 1
    assert claimed >= len(keys(group)) // 4


def test_self_design_puts_a_in_its_own_walk():
    """The statement (numpy) on the self design under STRICT 24: d1(P1's a) = 40 <= tau(P2) = 54, so the block of the two pairs
    walks over P1's a; and the accepted counts of the wave and workgroup designs are the ones named."""
    a, b, _ = design("self", S.RULE_STRICT, 24, 32, None, 0)
    _, fd = S.knn(a[:2], b, 2)
    assert fd.tolist() == [[5, 40], [30, 60]] and tau(S.RULE_STRICT, 24, 30) == 54
    for rule, pu in RULES:
        for n in ACCEPTED:
            a, b, _ = design("accepted", rule, pu, n, 1, 1)
            _, fd = S.knn(a, b, 2)
            got = sum(S.accept(rule, int(d0), int(d1), pu, 0.5) for d0, d1 in fd)
            assert got == (n if n > 4 or (rule, pu) != (S.RULE_BETTER_BY, 1) else n + 3), (rule, pu, n, got)


@pytest.mark.gpu
@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("kernel", KERNELS)
def test_lists_equal_oracle_and_search(gpu, kernel, group):
    _, knn = gpu
    ks = keys(group)
    cap = max(max(len(design(*k)[0]), len(design(*k)[1])) for k in ks)
    lists = knn.Matcher(cap, kernel=kernel, reverse_check="lists")
    search = knn.Matcher(cap, kernel=kernel, reverse_check="search")
    try:
        for key in ks:
            a, b, _ = design(*key)
            got = lists.match(a, b, key[1], key[2], 0.5, True)
            assert np.array_equal(got, answer(key)), (kernel, key, "oracle")
            assert np.array_equal(got, search.match(a, b, key[1], key[2], 0.5, True)), (kernel, key, "search")
    finally:
        lists.close()
        search.close()


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(torch.device("cuda", 0))


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", KERNELS)
def test_mixed_batch(gpu, kernel):
    """One hm_match_batch_device call over ONE buffer of five blocks under reverse_check="auto" with the share at 2^-5: a
    problem that stays on the lists (an edge design: 66 walk rows for each of three pairs, far below the share), the
    clustered problem of test_gpu_reverse_from_lists, which that share sends to the fallback, and a block of one row: count 0."""
    import torch
    _, knn = gpu
    from cv_amd import _lib
    from test_gpu_reverse_from_lists import clustered
    L = _lib.lib()
    ca, cb = clustered()
    for rule, pu in RULES:
        ea, eb, _ = design("edge", rule, pu, 65, 0, LAST)
        sides = (ea, eb, ca, cb, ca[:1])
        cap = max(len(s) for s in sides)
        blocks = np.full((5, cap, 64), 0x5A, np.uint8)
        counts = np.array([len(s) for s in sides], np.int32)
        for k, rows in enumerate(sides):
            blocks[k, :len(rows)] = rows
        ia, ib = np.array([0, 2, 4], np.uint32), np.array([1, 3, 1], np.uint32)
        d_blocks, d_counts = _up(blocks), _up(counts)
        m = knn.Matcher(cap, kernel=kernel, reverse_check="auto", fallback_share_log2=5)
        try:
            d_pairs = torch.full((3 * cap * 8,), 0xFF, dtype=torch.uint8, device=d_blocks.device)
            d_n = torch.full((3 * 4,), 0xFF, dtype=torch.uint8, device=d_blocks.device)
            _lib.check(L.hm_match_batch_device(m.handle, d_blocks.data_ptr(), d_counts.data_ptr(), d_blocks.data_ptr(), d_counts.data_ptr(), cap,
                                               ia.ctypes.data_as(C.c_void_p), ib.ctypes.data_as(C.c_void_p), 3, rule, pu, 0.5, 1,
                                               d_pairs.data_ptr(), d_n.data_ptr(), _lib.wait_handle(torch.cuda.current_stream())), "match_batch")
            _lib.check(L.hm_sync(m.handle), "hm_sync")
        finally:
            m.close()
        gp = d_pairs.cpu().numpy().view(np.uint32).reshape(3, cap, 2)
        gn = d_n.cpu().numpy().view(np.uint32)
        from oracle import oracle as O
        for p, (qa, tb) in enumerate(((ea, eb), (ca, cb))):
            want = np.asarray(O.match(qa, tb, rule, pu, 0.5, True), np.int64).reshape(-1, 2)
            assert gn[p] == len(want), (kernel, rule, pu, p, gn[p], len(want))
            assert np.array_equal(gp[p, :gn[p]], want) and (gp[p, gn[p]:] == 0xFFFFFFFF).all(), (kernel, rule, pu, p)
        assert gn[2] == 0 and (gp[2] == 0xFFFFFFFF).all(), (kernel, rule, pu)
