"""The consensus stage (rs_essential_arrsac / rs_p3p_arrsac and their batched entries) in plain Python / numpy, written from
the text of include/akz.h and the papers it cites, and a catalogue of designed scenes on which every rule decides at equality.

Nothing here imports the C oracle (oracle/), compiles an akz_*_math.h or reads a kernel.  What is stated:

  draw, scene_seed      the sampler: splitmix64 / xoshiro256++ (Blackman, Vigna: "Scrambled linear pseudorandom number
                        generators"), one stream per minimal sample, K distinct indices (high 32 bits x n >> 32, duplicates
                        redrawn); the seed of scene s of a batched call; the re-sampling stream.
  shuffle_order         RS_BATCH_SHUFFLE: the 32-bit key of every position and the stable ascending order.
  inlier_matrix         CameraToCamera::residual (LAPACK eigh) and WorldToCamera::residual as float64, taken over from
                        test_gpu_independent_geometry.py: the boolean matrix [pose, match] and the residuals nearest to the
                        threshold on either side.
  consensus             the loop over such a matrix: blocks, the exact bound, Wald's SPRT (Raguram, Frahm, Pollefeys, ECCV
                        2008, section 3; Matas, Chum: "Randomized RANSAC with sequential probability ratio test", ICCV 2005),
                        the candidate cap and its halving (the preemption function f(i) = floor(M 2^-floor(i/B))), the
                        inlier-guided re-sampling rounds, the final arg-max, and all five fields of rs_arrsac_stats.

The statement never solves for a pose.  The poses of a set of minimal samples come from a PROVIDER, a callable
samples [h, K] -> (poses [h, 4, 3, 4], ok [h, 4]): the oracle's solvers on the CPU, the exhaustive device entry followed by
rs_debug_poses on the GPU.  Re-sampled hypotheses go through the provider with the samples the statement predicts, so a wrong
re-sampled index shows as a different pose, count and winner.

Designed scenes: one set of world points and G planted poses; match m observes its point under the pose of its group
(labels[m]; -1 = an unrelated bearing).  Caller samples are drawn inside one group, the threshold is 1e-9.  The planted pose of
a sample's group then comes back with exactly its group as inliers (residuals ~1e-16), every other pose a solver returns for
that sample has its own sample matches as inliers at the most (P3P) or none (two-view), and the residuals of everything else
lie orders of magnitude above the threshold: the count of every pose after every block is a closed form of the labels and
the scoring order.  Two conditions hold on every case and are asserted wherever a case runs (no case is excused):
no residual between thr / 100 and 100 thr, and no SPRT decision within 1e-9 (relative) of the likelihood ratio threshold.

Family "five_point" is the two-view consensus with RS_ESTIMATOR_FIVE_POINT: 5-match samples, ten hypothesis slots a sample
(the provider returns [10 h, 4, 3, 4]; slots without a solution are not ok and never live), ids (10 sample + solution) 4 + pose,
max_candidates and stats.poses counting poses.
"""
import math
from dataclasses import dataclass, field, replace

import numpy as np

from test_gpu_independent_geometry import _np_residuals, _projective, _rodrigues, _w2c_residual

NONE = 0xFFFFFFFF
SAMPLE_SIZE = {"p3p": 3, "two_view": 8, "five_point": 5}
SLOTS = {"p3p": 1, "two_view": 1, "five_point": 10}     # hypothesis slots a sample owns (rs_five_point_batch: ten)
M64 = (1 << 64) - 1
THR = 1e-9
POSE_TOL = 1e-6                       # the reference's EPSILON_APPROX (lambda-twist/tests/consensus.rs)
ALTERATIONS = ("ties_descending", "budget_spent_on_retired", "sprt_over_all_matches", "unstable_shuffle")


# ------------------------------------------------------------------------------------------------ sampler and shuffle
def splitmix64(state):
    """One step of splitmix64: (new state, output)."""
    state = (state + 0x9E3779B97F4A7C15) & M64
    z = state
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return state, z ^ (z >> 31)


def _rotl(x, k):
    return ((x << k) | (x >> (64 - k))) & M64


class Xoshiro256pp:
    """xoshiro256++ 1.0, its four words filled by successive splitmix64 outputs (rand_xoshiro's seed_from_u64)."""

    def __init__(self, seed):
        self.s = []
        for _ in range(4):
            seed, out = splitmix64(seed)
            self.s.append(out)

    def next(self):
        s = self.s
        r = (_rotl((s[0] + s[3]) & M64, 23) + s[0]) & M64
        t = (s[1] << 17) & M64
        s[2] ^= s[0]
        s[3] ^= s[1]
        s[1] ^= s[2]
        s[0] ^= s[3]
        s[2] ^= t
        s[3] = _rotl(s[3], 45)
        return r


def draw(seed, h, n, K):
    """The minimal sample of stream h: K distinct indices below n.  Stream h is seeded with seed + 0xD1B54A32D192ED03 (h + 1)."""
    g = Xoshiro256pp((seed + 0xD1B54A32D192ED03 * (h + 1)) & M64)
    out = []
    while len(out) < K:
        v = ((g.next() >> 32) * n) >> 32
        if v not in out:
            out.append(v)
    return out


def samples_of(seed, n, n_hyp, K):
    return np.array([draw(seed, h, n, K) for h in range(n_hyp)], np.uint32).reshape(n_hyp, K)


RESAMPLE_XOR = 0xA5A5A5A55A5A5A5A    # the re-sampling rounds draw from stream h of seed ^ this, h = the sample's number


def scene_seed(seed, scene):
    return (seed + 0x9E3779B97F4A7C15 * scene) & M64


def shuffle_keys(seed_s, n):
    return [splitmix64(((seed_s ^ 0x5851F42D4C957F2D) + 0xD1342543DE82EF95 * j) & M64)[1] >> 32 for j in range(n)]


def shuffle_order(seed_s, n, alter=()):
    """position -> match: ascending key, equal keys in index order."""
    keys = shuffle_keys(seed_s, n)
    if "unstable_shuffle" in alter:
        return np.array(sorted(range(n), key=lambda j: (keys[j], -j)), np.int64)
    return np.array(sorted(range(n), key=lambda j: keys[j]), np.int64)     # (Python's sort is stable)


# ------------------------------------------------------------------------------------------------ residual predicates
def inlier_matrix(family, poses, first, second, thr):
    """poses [P, 3, 4] -> (inl [P, n] bool, below, above): the largest residual under thr and the smallest one at or over it."""
    poses = np.asarray(poses, np.float64).reshape(-1, 3, 4)
    n = len(first)
    if len(poses) == 0 or n == 0:
        return np.zeros((len(poses), n), bool), 0.0, math.inf
    if family == "p3p":
        res = np.stack([_w2c_residual(P[:, :3], P[:, 3], first, second) for P in poses])
    else:
        res = _np_residuals(poses, first, second)
    res = np.where(np.isnan(res), math.inf, res)
    inl = res < thr
    below = float(res[inl].max()) if inl.any() else 0.0
    above = float(res[~inl].min()) if (~inl).any() else math.inf
    return inl, below, above


# ------------------------------------------------------------------------------------------------ the loop
@dataclass(frozen=True)
class Params:
    """rs_arrsac_params, field for field (n_hypotheses: see Case.samples)."""
    block_size: int
    init_blocks: int = 0
    max_candidates: int = 0
    bound: bool = True
    sprt: bool = False
    halve: bool = False
    sprt_delta: float = 0.05
    sprt_ratio: float = 1e3
    seed: int = 0
    estimations_per_block: int = 0
    threshold: float = THR

    def kw(self):
        """the keyword arguments of oracle.arrsac and of EssentialConsensus.arrsac_model_inliers"""
        return dict(block_size=self.block_size, init_blocks=self.init_blocks, max_candidates=self.max_candidates,
                    bound=self.bound, sprt=self.sprt, halve=self.halve, sprt_delta=self.sprt_delta, sprt_ratio=self.sprt_ratio,
                    seed=self.seed, estimations_per_block=self.estimations_per_block)


@dataclass
class Result:
    best_id: int
    pose: np.ndarray
    inliers: np.ndarray
    stats: dict
    sprt_margin: float               # smallest |lhs - ln ratio| / ln ratio over the SPRT decisions taken
    below: float                     # residuals nearest to the threshold, over every pose the run made
    above: float
    samples: np.ndarray              # every minimal sample the run made, row = sample number (unused rounds: NONE rows)
    poses: np.ndarray                # [samples, 4, 3, 4] as the provider gave them
    ok: np.ndarray
    counts: dict = field(default_factory=dict)       # pose id -> count when the run ended


def sprt_rejects(c, best, seen, delta, log_ratio):
    """Wald's test on a pose with c inliers among `seen` matches, eps = best / seen.  (rejected, lhs).
    lhs = c ln(delta / eps) + (seen - c) ln((1 - delta) / (1 - eps)) is linear in c and equals -seen KL(eps || delta) <= 0
    at c = best: a pose at the best count is never rejected, and where eps <= delta (the slope is then >= 0) no pose is."""
    l_in = math.log(delta) - (math.log(best) - math.log(seen))
    l_out = math.log(1.0 - delta) - (math.log(seen - best) - math.log(seen))
    lhs = c * l_in + (seen - c) * l_out
    return lhs > log_ratio, lhs


def consensus(family, first, second, prm, samples, provider, order=None, alter=()):
    """The whole procedure on one scene.  samples [H, K] are the initial minimal samples (the caller's, or samples_of());
    order: position -> match (None: index order)."""
    n = len(first)
    K, slots = SAMPLE_SIZE[family], SLOTS[family]
    order = np.arange(n) if order is None else np.asarray(order, np.int64)
    thr, E, M = prm.threshold, prm.estimations_per_block, prm.max_candidates
    rows, pose_of, count = {}, {}, {}
    all_samples, all_poses, all_ok = [], [], []
    gap = [0.0, math.inf]

    def make(first_sample, smp):
        """the poses of samples first_sample.. -> ids of the valid ones, ascending; their inlier rows are kept"""
        smp = np.asarray(smp, np.uint32).reshape(-1, K)
        poses, ok = provider(smp)
        poses = np.asarray(poses, np.float64).reshape(len(smp) * slots, 4, 3, 4)
        ok = np.asarray(ok).reshape(len(smp) * slots, 4).astype(bool)
        all_samples.append(smp); all_poses.append(poses); all_ok.append(ok)
        sel = np.argwhere(ok)
        inl, below, above = inlier_matrix(family, poses[ok], first, second, thr)
        gap[0], gap[1] = max(gap[0], below), min(gap[1], above)
        ids = []
        for (h, p), row in zip(sel, inl):
            pid = 4 * (slots * first_sample + int(h)) + int(p)
            rows[pid], pose_of[pid], count[pid] = row, poses[h, p], 0
            ids.append(pid)
        return ids

    def unused(k):
        all_samples.append(np.full((k, K), NONE, np.uint32)); all_poses.append(np.zeros((k * slots, 4, 3, 4)))
        all_ok.append(np.zeros((k * slots, 4), bool))

    made = len(samples)
    alive = make(0, samples)
    prune = prm.bound or prm.sprt or M > 0 or E > 0
    bs = prm.block_size if prune else max(n, 1)           # nothing to decide between blocks: one block
    log_ratio = math.log(prm.sprt_ratio) if prm.sprt else 0.0
    seen = blocks = evaluated = 0
    sprt_margin = math.inf
    while seen < n:
        hi = min(seen + bs, n)
        blk = order[seen:hi]
        for pid in alive:
            count[pid] += int(rows[pid][blk].sum())
        evaluated += len(alive) * (hi - seen)
        seen = hi
        blocks += 1
        if not prune or seen >= n:                        # nothing is retired after the last block
            continue
        best = max((count[p] for p in alive), default=0)
        left = n - seen
        cap = 0
        if M and blocks >= prm.init_blocks:
            cap = M
            if prm.halve:
                cap = max(1, M >> (blocks - prm.init_blocks))
        # bound, then SPRT (only when 0 < best < seen)
        passed = []
        for pid in alive:
            c = count[pid]
            keep = c + left >= best
            if keep and prm.sprt and 0 < best < seen:
                total = n if "sprt_over_all_matches" in alter else seen
                rejected, lhs = sprt_rejects(c, best, total, prm.sprt_delta, log_ratio)
                sprt_margin = min(sprt_margin, abs(lhs - log_ratio) / log_ratio)
                keep = not rejected
            if keep:
                passed.append(pid)
        # The cap ranks the population BEFORE this block's retirements by (distance to the best count, id): the poses nearer
        # than the cap-th one stay, those as far as it share what is left of the cap, in ascending id, among the poses that
        # passed bound and SPRT.  (Bound and SPRT retire by count alone, from the far end of that ranking, so ranking the
        # population after them instead gives the same survivors; what can be told apart is whether a retired pose takes a
        # place of the tie budget, and only in the bin of 2047 and more, the one bin that holds different counts.)
        if cap and len(alive) > cap:
            dist = {p: min(best - count[p], 2047) for p in alive}
            T = sorted(dist.values())[cap - 1]
            budget = cap - sum(1 for d in dist.values() if d < T)
            at_T = [p for p in (alive if "budget_spent_on_retired" in alter else passed) if dist[p] == T]
            if "ties_descending" in alter:
                at_T = at_T[::-1]
            admitted = set(at_T[:budget])
            passed = [p for p in passed if dist[p] < T or p in admitted]
        alive = passed
        if cap == 1 and E == 0 and prm.halve:             # a single survivor cannot be overtaken
            break
        if E and blocks >= prm.init_blocks:
            if alive:
                b = max(alive, key=lambda p: (count[p], -p))
                L = [int(m) for m in order[:seen] if rows[b][m]]
                evaluated += seen
                if len(L) >= K:
                    smp = [[L[j] for j in draw(prm.seed ^ RESAMPLE_XOR, made + e, len(L), K)] for e in range(E)]
                    for pid in make(made, smp):
                        count[pid] = int(rows[pid][order[:seen]].sum())
                        evaluated += seen
                        alive.append(pid)
                else:
                    unused(E)
            else:
                unused(E)
            made += E                                     # a round that drew nothing still takes its sample numbers
    stats = dict(poses=4 * slots * made, survivors=len(alive), blocks=blocks, residuals_evaluated=evaluated,
                 residuals_exhaustive=4 * slots * made * n)
    smp_all = np.concatenate(all_samples) if all_samples else np.zeros((0, K), np.uint32)
    res = Result(NONE, np.zeros((3, 4)), np.zeros(0, np.uint32), stats, sprt_margin, gap[0], gap[1], smp_all,
                 np.concatenate(all_poses), np.concatenate(all_ok), {p: count[p] for p in alive})
    if alive:
        w = max(alive, key=lambda p: (count[p], -p))
        res.best_id, res.pose = w, pose_of[w]
        res.inliers = np.flatnonzero(rows[w]).astype(np.uint32)
    return res


def margins_hold(res, thr=THR):
    """the two conditions of a designed case"""
    return res.below <= thr / 100 and res.above >= 100 * thr and res.sprt_margin >= 1e-9


# ------------------------------------------------------------------------------------------------ designed scenes
@dataclass
class Case:
    name: str
    family: str                      # "p3p" | "two_view"
    first: np.ndarray                # bearings [n, 3] (two-view: of camera a)
    second: np.ndarray               # world points [n, 4] | bearings of camera b [n, 3]
    labels: np.ndarray               # group of every match, -1: unrelated
    planted: list                    # (R, t) of every group; two-view: |t| = 1
    samples: np.ndarray              # caller samples [H, K], or None: the sampler draws n_hyp of them
    sample_group: list               # group of every caller sample (None where samples is None)
    prm: Params
    n_hyp: int = 0
    expect: dict = field(default_factory=dict)   # closed forms: winner = (sample, group) | None, stats = {field: value}

    @property
    def K(self):
        return SAMPLE_SIZE[self.family]

    def initial_samples(self):
        if self.samples is not None:
            return self.samples
        return samples_of(self.prm.seed, len(self.first), self.n_hyp, self.K)


def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _scene(family, seed, labels):
    labels = np.asarray(labels, np.int64)
    n, G = len(labels), int(labels.max()) + 1 if len(labels) else 0
    rng = np.random.default_rng(seed)
    X = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(4, 8, n)], 1)
    planted = []
    junk = rng.standard_normal((n, 3)); junk[:, 2] = np.abs(junk[:, 2]) + 0.5
    seen_by = _unit(junk)
    for g in range(G):
        R = _rodrigues((rng.random(3) - 0.5) * 0.6)
        t = (rng.random(3) - 0.5) * (1.0 if family == "p3p" else 2.0)
        if family != "p3p":
            t = t / np.linalg.norm(t)
        planted.append((R, t))
        m = labels == g
        seen_by[m] = _unit(X[m] @ R.T + t)
    if family == "p3p":
        return seen_by, _projective(X), labels, planted
    return _unit(X), seen_by, labels, planted


def _runs(*runs):
    """labels from (group, count) runs"""
    return np.concatenate([np.full(c, g, np.int64) for g, c in runs])


def _pick(rng, labels, group, K, lo=0, hi=None):
    """K distinct matches of `group` with index in [lo, hi)"""
    pool = np.flatnonzero(labels == group)
    pool = pool[(pool >= lo) & (pool < (len(labels) if hi is None else hi))]
    return rng.choice(pool, K, replace=False)


def _case(name, family, seed, labels, groups, prm, lo=0, hi=None, **expect):
    """caller samples: one inside group groups[h] for every h, drawn among the matches [lo, hi)"""
    first, second, labels, planted = _scene(family, seed, labels)
    rng = np.random.default_rng(seed + 1)
    K = SAMPLE_SIZE[family]
    seen, smp = set(), []
    for g in groups:
        while True:
            s = tuple(int(v) for v in _pick(rng, labels, g, K, lo, hi))
            if tuple(sorted(s)) not in seen:
                seen.add(tuple(sorted(s)))
                break
        smp.append(s)
    return Case(name, family, first, second, labels, planted, np.array(smp, np.uint32), list(groups), prm, len(groups), dict(expect))


def _sampler_case(name, family, seed, labels, n_hyp, prm, **expect):
    first, second, labels, planted = _scene(family, seed, labels)
    return Case(name, family, first, second, labels, planted, None, None, prm, n_hyp, dict(expect))


def _seen_alike(P, Q, depth):
    """A world point that poses P and Q see at the same bearing, at `depth` in front of P's camera: with Y = depth (u, v, 1)
    the point is X = Rp^T (Y - tp), and (u, v) solves proj(Rq X + tq) = (u, v) (Newton, numerical Jacobian).  Such points
    form a curve; a match on it is an exact inlier of both poses."""
    (Rp, tp), (Rq, tq) = P, Q

    def g(uv):
        Y = depth * np.array([uv[0], uv[1], 1.0])
        Z = Rq @ (Rp.T @ (Y - tp)) + tq
        return Z[:2] / Z[2] - uv, Y, Z
    uv = np.zeros(2)
    for _ in range(60):
        f0 = g(uv)[0]
        J = np.stack([(g(uv + h)[0] - f0) / 1e-7 for h in (np.array([1e-7, 0.0]), np.array([0.0, 1e-7]))], 1)
        uv = uv - np.linalg.solve(J, f0)
    f0, Y, Z = g(uv)
    assert np.abs(f0).max() < 1e-14 and Z[2] > 0, (f0, Z)
    return Rp.T @ (Y - tp), Y / np.linalg.norm(Y)


OVERTAKE_SEED = 730
FIVE_POINT_SEED = 722             # the first seed from 720 on whose scene meets the residual margin


def designed_cases():
    """name -> Case.  The closed forms (`expect`) are derived in the comments from the labels and the order alone."""
    out = []
    A, B, C, D, X = 0, 1, 2, 3, -1
    for fam, s0 in (("p3p", 100), ("two_view", 200)):
        # ---- the bound at equality.  Blocks of 10 on 40 matches.  Sample 0 is in B, sample 1 in A.
        # stays: A 20, B 20.  After block 2 B has 0 + 20 == 20, after block 3 10 + 10 == 20: it stays both times, ends 20 : 20
        # and wins by its lower id.  retired: one B match of block 3 is unrelated instead.  After block 3 B has
        # 9 + 10 == 20 - 1: it is retired and A wins with 20.
        bound = Params(block_size=10)
        out.append(_case(f"{fam}/bound/stays", fam, s0 + 1, _runs((A, 20), (B, 20)), [B, A], bound,
                         winner=(0, B), stats=dict(blocks=4, poses=8)))
        out.append(_case(f"{fam}/bound/retired", fam, s0 + 2, _runs((A, 20), (B, 9), (X, 1), (B, 10)), [B, A], bound,
                         winner=(1, A), stats=dict(blocks=4, poses=8)))
        # the same without RS_PRUNE_BOUND but with a cap (one that never cuts) to ask for blocks: the bound still retires B
        out.append(_case(f"{fam}/bound/without_its_flag", fam, s0 + 2, _runs((A, 20), (B, 9), (X, 1), (B, 10)), [B, A],
                         Params(block_size=10, bound=False, max_candidates=100), winner=(1, A), stats=dict(blocks=4, poses=8)))
        # ---- the winner's ties.  Blocks of 6 on 30 matches: A 6, B 12, unrelated 6, A 6.  Samples A, B, A: B (the later id)
        # leads 12 : 6 until the last block (A: 6 + 6 == 12 keeps it), the end is 12 : 12 : 12 and sample 0 wins.
        out.append(_case(f"{fam}/winner/lowest_id", fam, s0 + 3, _runs((A, 6), (B, 12), (X, 6), (A, 6)),
                         [A, B, A], Params(block_size=6), winner=(0, A), stats=dict(blocks=5, poses=12)))
        # the same with the two groups in exchanged samples: the winner is B of sample 0
        out.append(_case(f"{fam}/winner/lowest_hypothesis", fam, s0 + 4, _runs((A, 6), (B, 12), (X, 6), (A, 6)),
                         [B, A, A, B], Params(block_size=6), winner=(0, B), stats=dict(blocks=5, poses=16)))
        # ---- block sizes: 1, n - 1, n, n + 1, and n no multiple of the block.  n = 23, A 13, B 10.
        lab = _runs((B, 5), (A, 13), (B, 5))
        for bs in (1, 22, 23, 24, 5):
            out.append(_case(f"{fam}/blocks/size_{bs}", fam, s0 + 5, lab, [B, A, B], Params(block_size=bs),
                             winner=(1, A), stats=dict(blocks=-(-23 // bs), poses=12)))
        # no rule at all: one block whatever block_size says
        out.append(_case(f"{fam}/blocks/no_rule", fam, s0 + 5, lab, [B, A, B], Params(block_size=5, bound=False),
                         winner=(1, A), stats=dict(blocks=1, poses=12)))
        # n == K and n == K + 1: with the sampler every sample of n == K is a permutation of all matches
        K = 3 if fam == "p3p" else 8
        out.append(_sampler_case(f"{fam}/blocks/n_eq_K", fam, s0 + 6, _runs((A, K)), 5, Params(block_size=2, seed=11),
                                 winner=(0, A), stats=dict(blocks=-(-K // 2), poses=20)))
        out.append(_sampler_case(f"{fam}/blocks/n_eq_K_plus_1", fam, s0 + 7, _runs((A, K + 1)), 5, Params(block_size=K, seed=12),
                                 winner=(0, A), stats=dict(blocks=2, poses=20)))
        # ---- halving.  M = 8, blocks of 4 on 40 matches (ten blocks), twelve samples.  The cap is 8, 4, 2, 1 after blocks
        # init, init + 1, ..; with no re-sampling the loop ends at cap 1: blocks = max(init, 1) + 3.  init_blocks 0: the
        # first decision is after block 1 with a shift of 1 (8 >> 1 = 4, 2, 1): three blocks.
        lab = np.tile(np.array([A, A, B, X]), 10)
        smp = [A, B] * 6
        for init, blocks in ((0, 3), (1, 4), (3, 6), (20, 10)):
            out.append(_case(f"{fam}/halve/init_{init}", fam, s0 + 8, lab, smp, Params(block_size=4, init_blocks=init, max_candidates=8, halve=True),
                             winner=(0, A), stats=dict(blocks=blocks, poses=48, **({"survivors": 1} if init < 20 else {}))))
        # with re-sampling the loop goes on to the last block
        out.append(_case(f"{fam}/halve/resampling_goes_on", fam, s0 + 8, lab, smp,
                         Params(block_size=4, init_blocks=1, max_candidates=8, halve=True, estimations_per_block=2, seed=5),
                         stats=dict(blocks=10, poses=4 * (12 + 2 * 9))))
        # a shift of 31 and more: blocks of one match on 40 matches
        out.append(_case(f"{fam}/halve/shift_past_31", fam, s0 + 8, lab, smp,
                         Params(block_size=1, init_blocks=0, max_candidates=8, halve=True, estimations_per_block=1, seed=6),
                         stats=dict(blocks=40, poses=4 * (12 + 39))))
        # ---- the cap at the population's size and one below it (two-view: every sample has four poses; P3P: the provider's
        # count decides which of the two caps cuts, both are run)
        lab = _runs((A, 4), (X, 4), (A, 12), (B, 12))
        for M in (23, 24) if fam == "two_view" else range(3, 13):
            out.append(_case(f"{fam}/cap/population_{M}", fam, s0 + 9, lab, [A] * (6 if fam == "two_view" else 3),
                             Params(block_size=8, init_blocks=1, max_candidates=M), lo=8, winner=(0, A)))
        # ---- SPRT.  delta 0.05, ratio 1e3 (ln = 6.908), blocks of 10 on 40 matches.
        sp = Params(block_size=10, sprt=True)
        # best == seen after every block but the last: the test is off, nothing but the bound retires
        out.append(_case(f"{fam}/sprt/best_eq_seen", fam, s0 + 10, _runs((A, 30), (B, 10)), [B, A], sp, winner=(1, A), stats=dict(blocks=4)))
        # best == 0 after the first block (ten unrelated matches first, samples drawn behind them)
        out.append(_case(f"{fam}/sprt/best_zero", fam, s0 + 11, _runs((X, 10), (A, 20), (B, 10)), [B, A], sp, lo=10,
                         winner=(1, A), stats=dict(blocks=4)))
        # eps = 1/2, ratio 6e4 (ln = 11.0): a pose with no inlier has lhs = seen ln(0.95 / 0.5) = 0.642 seen: 6.42 <= 11.0 after
        # block 1 (kept), 12.8 after block 2 (rejected, though 0 + 20 >= 10 passes the bound).  A and B alternate: their poses (5 of
        # 10, 10 of 20, 15 of 30) are at the best count, the poses without support go after block 2 and the three planted ones
        # remain.  B ties A (20 : 20) and sample 0 wins.
        out.append(_case(f"{fam}/sprt/rejected_at_block_2", fam, s0 + 12, np.tile(np.array([A, B]), 20), [A, B, A],
                         replace(sp, sprt_ratio=6e4), lo=30 if fam == "p3p" else 0, winner=(0, A), stats=dict(blocks=4, poses=12, survivors=3)))
        # ---- re-sampling: E = 2, init_blocks 1, one sample in A drawn behind block 1.  After block 1 the best pose has exactly
        # K - 1 inliers among the matches seen (the round draws nothing and keeps its sample numbers 1, 2) or exactly K (the
        # round draws the only set there is, twice).
        bs, tail = (4, 8) if fam == "p3p" else (10, 12)
        for k in (K - 1, K):
            lab = _runs((A, k), (X, bs - k), (A, tail), (X, 4))
            rounds = -(-len(lab) // bs) - 1
            out.append(_case(f"{fam}/resample/best_has_{'K' if k == K else 'K_minus_1'}", fam, s0 + 13 + k, lab, [A],
                             Params(block_size=bs, init_blocks=1, estimations_per_block=2, seed=3), lo=bs + (4 if fam == "p3p" else 0),
                             winner=(0, A), stats=dict(blocks=rounds + 1, poses=4 * (1 + 2 * rounds))))
        # ---- hypothesis counts with the caller's samples, all in one group
        if fam == "p3p":
            lab = np.where(np.arange(50) % 5 == 4, X, A)
            for H in (1, 63, 64, 65, 255, 256, 257):
                out.append(_case(f"p3p/count_given/{H}", fam, s0 + 20, lab, [A] * H, Params(block_size=16, init_blocks=1, max_candidates=40),
                                 winner=(0, A), stats=dict(blocks=4, poses=4 * H)))
    # ---- the cap at the threshold distance (P3P).  64 matches, blocks of 16, init_blocks 1.  Block 1 holds 8 A and 8 B matches,
    # the rest 16 A and 32 B: A ends with 24, B with 40.  320 samples, all drawn among the matches 16.., so after block 1 every
    # planted pose has 8 and every other pose 0: the planted poses tie at distance 0, one per sample.  All samples are in A but
    # sample j, which is in B.  With cap M <= 320 the tie budget is M: B's pose is the (j + 1)-th tie.  j = M - 1: inside, B
    # stays and wins with 40.  j = M: outside, B is retired and the A pose of sample 0 wins with 24.
    # (Two-view: the same scene with 8-match samples at two of the caps; the three other poses of a sample's essential matrix
    # have no support at all.)
    lab = np.concatenate([_runs((A, 8), (B, 8)), np.tile(np.array([B, A, B]), 16)])
    for fam, seed, caps in (("p3p", 302, (1, 63, 64, 65, 255, 256, 257)), ("two_view", 320, (64, 257))):
        for M in caps:
            for where, j in (("inside", M - 1), ("outside", M)):
                groups = [A] * 320
                groups[j] = B
                out.append(_case(f"{fam}/cap/ties_{M}_{where}", fam, seed, lab, groups, Params(block_size=16, init_blocks=1, max_candidates=M),
                                 lo=16, winner=(j, B) if where == "inside" else (0, A), stats=dict(blocks=4, poses=1280)))
    # ---- the last bin (P3P).  4 300 matches, two blocks of 2 150.  Block 1: L matches of A, one of C, the rest unrelated; block
    # 2: 3 of A, 2 141 of C, 6 of D.  Samples A, D, D, C, all drawn in block 2 (so that no other pose of theirs has support).
    # After block 1 A has L, C's pose 1, every other pose 0, and left = 2 150 >= L keeps them all past the bound.  Cap 2.  L = 2 046 / 2 047: C is at distance L - 1 <
    # 2 047, alone in its bin, ahead of the zero poses: it stays and wins with 2 142.  L = 2 048: C's distance 2 047 is in the
    # last bin with the zero poses (2 048), which come first by id: C is retired and A wins.
    for L in (2046, 2047, 2048):
        lab = _runs((A, L), (C, 1), (X, 2149 - L), (A, 3), (C, 2141), (D, 6))
        first, second, labels, planted = _scene("p3p", 400, lab)
        rng = np.random.default_rng(401)
        smp = [_pick(rng, labels, A, 3, lo=2150), _pick(rng, labels, D, 3), _pick(rng, labels, D, 3), _pick(rng, labels, C, 3, lo=2150)]
        out.append(Case(f"p3p/cap/last_bin_{L}", "p3p", first, second, labels, planted, np.array(smp, np.uint32), [A, D, D, C],
                        Params(block_size=2150, init_blocks=1, max_candidates=2), 4,
                        dict(winner=(3, C) if L < 2048 else (0, A), stats=dict(blocks=2, poses=16))))
    # ---- the tie budget skips retired poses (P3P).  4 320 matches, blocks of 2 220 and 2 100.  Block 1: 2 150 of A, 70 of C; block 2:
    # 3 of A, 6 of D, 2 091 of C.  Samples A, D, D, C drawn in block 2.  After block 1 (left 2 100): A 2 150; C 70, distance 2 080,
    # in the last bin, 70 + 2 100 >= 2 150 passes the bound; the poses without support, also in the last bin and earlier by id, do
    # not (2 100 < 2 150).  Cap 2: the one place left goes to the first pose of the bin that is still a candidate: C stays and
    # wins with 2 161 against 2 153.
    lab = _runs((A, 2150), (C, 70), (A, 3), (D, 6), (C, 2091))
    first, second, labels, planted = _scene("p3p", 410, lab)
    rng = np.random.default_rng(411)
    smp = [_pick(rng, labels, A, 3, lo=2220), _pick(rng, labels, D, 3), _pick(rng, labels, D, 3), _pick(rng, labels, C, 3, lo=2220)]
    out.append(Case("p3p/cap/budget_skips_retired", "p3p", first, second, labels, planted, np.array(smp, np.uint32), [A, D, D, C],
                    Params(block_size=2220, init_blocks=1, max_candidates=2), 4,
                    dict(winner=(3, C), stats=dict(blocks=2, poses=16, survivors=2))))
    # ---- no model: three identical world points seen at three identical bearings, n >= K; with re-sampling every round
    # (all candidates gone before it) still takes its numbers
    first, second, labels, planted = _scene("p3p", 700, _runs((A, 12)))
    first[:] = first[0]; second[:] = second[0]
    for E in (0, 2):
        out.append(Case(f"p3p/no_model/E_{E}", "p3p", first.copy(), second.copy(), labels, planted, np.array([[0, 1, 2], [3, 4, 5]], np.uint32),
                        [None, None], Params(block_size=4, estimations_per_block=E, max_candidates=4), 2,
                        dict(winner=None, stats=dict(blocks=3, poses=4 * (2 + 2 * E), survivors=0, residuals_evaluated=0))))
    # ---- eight matches that are one match repeated by value (two-view).  The eight-point solver does not refuse them: the
    # normal matrix has a null space of eight dimensions, the solver takes one of its vectors, and four poses come out that
    # no match supports.  So there IS a model: every count is 0, the lowest id wins and the inlier list is empty.
    first, second, labels, planted = _scene("two_view", 710, _runs((X, 12)))
    first[:] = first[0]; second[:] = second[0]
    out.append(Case("two_view/degenerate/one_match_repeated", "two_view", first, second, labels, planted,
                    np.array([np.arange(8), np.arange(4, 12)], np.uint32), [None, None], Params(block_size=4, max_candidates=4), 2,
                    dict(stats=dict(blocks=3, poses=8, survivors=4))))
    # ---- five-point: 14 matches, A 8 and B 6 interleaved, blocks of 4, cap 6 poses after block 1.  Sixteen samples: sample h is
    # permutation h // 2 of ONE five-match set of A (h even) or of B (h odd), so the catalogue's poses are those of two sets (the
    # other real solutions of a set have one-dimensional residuals: with sixteen different sets no scene meets the residual
    # margin).  A leads from block 1 on; the eight planted poses of A tie throughout and sample 0 wins: id (10 * 0 + solution) 4
    # + pose.  stats.poses = 16 * 10 * 4 whatever the number of solutions.
    lab = np.array([A, B, A, A, B, A, B, A, A, B, A, B, A, B])
    first, second, labels, planted = _scene("five_point", FIVE_POINT_SEED, lab)
    rng = np.random.default_rng(FIVE_POINT_SEED + 1)
    sets = {A: _pick(rng, labels, A, 5), B: _pick(rng, labels, B, 5)}
    smp = [rng.permutation(sets[A if h % 2 == 0 else B]) if h > 1 else sets[A if h % 2 == 0 else B] for h in range(16)]
    out.append(Case("five_point/sixteen_samples", "five_point", first, second, labels, planted, np.array(smp, np.uint32), [A, B] * 8,
                    Params(block_size=4, init_blocks=1, max_candidates=6), 16, dict(winner=(0, A), stats=dict(blocks=4, poses=640))))
    # ---- a re-sampled pose that overtakes (P3P).  Poses P (group A) and Q (group C), and three matches S whose world points both
    # poses see at the same bearing: exact inliers of both.  20 matches, blocks of 4, E = 1, init_blocks 1:  S S S x | A A A A |
    # C C C C | C C C C | C x x x.  The one caller sample is in A.  After block 1 P has exactly the three S; the round's only
    # possible sample is S, whose poses include P again and Q, which no initial sample knows.  Q joins with 3, passes the bound
    # after block 2 (3 + 12 >= 7), ties P after block 3 (7 : 7, P is re-sampled from) and ends with 12 against 7: the winner is
    # the pose of sample 1 (the first re-sampled one) that is Q, its inliers are S and C.
    rng = np.random.default_rng(OVERTAKE_SEED)
    P = (_rodrigues((rng.random(3) - 0.5) * 0.4), (rng.random(3) - 0.5) * 1.0)
    Q = (_rodrigues((rng.random(3) - 0.5) * 0.4), (rng.random(3) - 0.5) * 1.0 + np.array([0.0, 0.0, 0.7]))
    lab = _runs((2, 3), (X, 1), (A, 4), (1, 9), (X, 3))
    n = len(lab)
    Xw = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(4, 8, n)], 1)
    junk = rng.standard_normal((n, 3)); junk[:, 2] = np.abs(junk[:, 2]) + 0.5
    bear = _unit(junk)
    bear[lab == A] = _unit(Xw[lab == A] @ P[0].T + P[1])
    bear[lab == 1] = _unit(Xw[lab == 1] @ Q[0].T + Q[1])
    for m, depth in zip(np.flatnonzero(lab == 2), (4.0, 6.0, 9.0)):
        Xw[m], bear[m] = _seen_alike(P, Q, depth)
    out.append(Case("p3p/resample/overtakes", "p3p", bear, _projective(Xw), lab, [P, Q], np.array([[4, 5, 6]], np.uint32), [A],
                    Params(block_size=4, init_blocks=1, estimations_per_block=1, seed=2), 1,
                    dict(resampled_winner=(1, 1, np.flatnonzero(lab >= 1)), stats=dict(blocks=5, poses=20))))
    # ---- hypothesis counts with the sampler (two-view: one group, every sample inside it, every count ties)
    for H in (1, 63, 64, 65, 255, 256, 257):
        out.append(_sampler_case(f"two_view/count/{H}", "two_view", 802, _runs((A, 40)), H,
                                 Params(block_size=16, init_blocks=1, max_candidates=40, seed=H), winner=(0, A), stats=dict(blocks=3, poses=4 * H)))
    # ---- hypothesis counts with the sampler (P3P, one group and a fifth unrelated: most samples are all-inlier)
    lab = np.where(np.arange(50) % 5 == 4, X, A)
    for H in (1, 63, 64, 65, 255, 256, 257):
        out.append(_sampler_case(f"p3p/count/{H}", "p3p", 801, lab, H, Params(block_size=16, init_blocks=1, max_candidates=40, seed=H),
                                 stats=dict(blocks=4, poses=4 * H)))
    return {c.name: c for c in out}


def planted_slot(case, res, sample):
    """slot * 4 + pose of sample `sample` that is the planted pose of its group (to POSE_TOL), asserted to exist"""
    R, t = case.planted[case.sample_group[sample] if case.sample_group else 0]
    slots = SLOTS[case.family]
    P, ok = res.poses[slots * sample:slots * (sample + 1)].reshape(-1, 3, 4), res.ok[slots * sample:slots * (sample + 1)].reshape(-1)
    gaps = [max(np.abs(P[q, :, :3] - R).max(), np.abs(P[q, :, 3] - t).max()) if ok[q] else math.inf for q in range(len(P))]
    q = int(np.argmin(gaps))
    assert gaps[q] < POSE_TOL, (case.name, sample, gaps)
    return q


def check_closed_form(case, res):
    """the case's own expectation against the statement's run, and the two margin conditions"""
    assert margins_hold(res, case.prm.threshold), (case.name, res.below, res.above, res.sprt_margin)
    if case.sample_group and case.sample_group[0] is not None:
        for h in range(len(case.sample_group)):            # every sample gives its group's planted pose
            planted_slot(case, res, h)
    exp = case.expect
    if "winner" in exp:
        if exp["winner"] is None:
            assert res.best_id == NONE and len(res.inliers) == 0, (case.name, res.best_id)
        else:
            h, g = exp["winner"]
            if case.sample_group:
                assert case.sample_group[h] == g, case.name
                assert res.best_id == 4 * SLOTS[case.family] * h + planted_slot(case, res, h), (case.name, res.best_id, h)
            else:
                assert res.best_id // (4 * SLOTS[case.family]) == h, (case.name, res.best_id)
            assert np.array_equal(res.inliers, np.flatnonzero(case.labels == g)), (case.name, res.inliers)
    if "resampled_winner" in exp:
        h, g, inliers = exp["resampled_winner"]
        R, t = case.planted[g]
        gaps = [max(np.abs(res.poses[h, p, :, :3] - R).max(), np.abs(res.poses[h, p, :, 3] - t).max()) if res.ok[h, p] else math.inf
                for p in range(4)]
        assert min(gaps) < POSE_TOL and res.best_id == 4 * h + int(np.argmin(gaps)), (case.name, res.best_id, gaps)
        assert h >= len(case.samples) and np.array_equal(res.inliers, inliers), (case.name, res.inliers)
    for key, val in exp.get("stats", {}).items():
        assert res.stats[key] == val, (case.name, key, res.stats)


# ------------------------------------------------------------------------------------------------ batched entries
def calibrate(cam, xy):
    """CameraIntrinsics::calibrate (cv-pinhole/src/lib.rs:108-117): pixel -> unit bearing.  cam = (fx, fy, cx, cy, skew)."""
    fx, fy, cx, cy, skew = cam[:5]
    xy = np.asarray(xy, np.float64)
    y = (xy[:, 1] - cy) / fy
    x = (xy[:, 0] - cx - skew * y) / fx
    return _unit(np.stack([x, y, np.ones(len(xy))], 1))


def project(cam, P):
    fx, fy, cx, cy, skew = cam[:5]
    x, y = P[:, 0] / P[:, 2], P[:, 1] / P[:, 2]
    return np.stack([fx * x + skew * y + cx, fy * y + cy], 1)


@dataclass
class Batch:
    """The arguments of a batched call.  Scene s reads pair list s, whose entries index keypoint block ia[s] (and ib[s], or the
    world table); xy_* are the keypoints' pixel coordinates [block, cap, 2] float32."""
    name: str
    family: str
    cap: int
    cam_a: tuple
    cam_b: tuple
    xy_a: np.ndarray
    xy_b: np.ndarray
    world: np.ndarray
    pairs: np.ndarray
    npairs: np.ndarray
    ia: list
    ib: list
    prm: Params
    n_hyp: int
    shuffle: bool
    labels: list

    def n(self, s):
        return min(int(self.npairs[s]), self.cap)      # counts above the capacity are clipped

    def scene(self, s):
        """(first, second) of scene s as this module calibrates them"""
        n = self.n(s)
        pr = self.pairs[s, :n].astype(np.int64)
        first = calibrate(self.cam_a, self.xy_a[self.ia[s]][pr[:, 0]])
        if self.family == "p3p":
            return first, self.world[pr[:, 1]]
        return first, calibrate(self.cam_b, self.xy_b[self.ib[s]][pr[:, 1]])


def batch_scene(batch, s, first, second, provider, alter=()):
    """Scene s of a batched call on the bearings / points it ran on: the single-scene procedure with the scene's seed, the
    sampler's samples and, with RS_BATCH_SHUFFLE, the shuffled order.  Fewer matches than a minimal sample: nothing runs."""
    K = 3 if batch.family == "p3p" else 8
    n = len(first)
    if n < K:
        zero = dict(poses=0, survivors=0, blocks=0, residuals_evaluated=0, residuals_exhaustive=0)
        return Result(NONE, np.zeros((3, 4)), np.zeros(0, np.uint32), zero, math.inf, 0.0, math.inf, np.zeros((0, K), np.uint32),
                      np.zeros((0, 4, 3, 4)), np.zeros((0, 4), bool)), None
    seed_s = scene_seed(batch.prm.seed, s)
    order = shuffle_order(seed_s, n, alter) if batch.shuffle else None
    res = consensus(batch.family, first, second, replace(batch.prm, seed=seed_s), samples_of(seed_s, n, batch.n_hyp, K), provider,
                    order=order, alter=alter)
    return res, order


CAM_A = (984.2439, 980.8141, 690.0, 233.1966, 0.0)
# the two-view scenes are exact in float32 pixels: focal lengths that are powers of two, everything else dyadic
CAM_2A = (1024.0, 1024.0, 512.0, 256.0, 0.0)
CAM_2B = (2048.0, 1024.0, 768.0, 512.0, 64.0)
RZ90 = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])


def _batch(name, family, seed, sizes, cap, prm, n_hyp, shuffle, labels_of=None, tries=None):
    """Scenes of the given sizes (a size above cap: the list is full and its count says more).  Every fifth match of a scene is
    unrelated unless labels_of(s, n) gives labels; groups are poses of the scene; the keypoint blocks lie in reverse order.
    Keypoints are float32 pixels, so a scene is built from the pixels: P3P: the world point of a match is its keypoint's ray at a
    random depth, taken back through the group's pose (consistent to float64 rounding).  Two-view: camera b is camera a turned
    by 0 or 90 degrees about the optical axis and moved in its image plane by dyadic amounts, inverse depths are dyadic: both
    pixels of a match are exact float32 numbers and the bearings are consistent to float64 rounding.
    tries[s]: which draw of scene s is taken, the first that meets the residual margin (found on the CPU, asserted by the tests)."""
    rng = np.random.default_rng(seed)
    S_ = len(sizes)
    two = family == "two_view"
    cam_a, cam_b = (CAM_2A, CAM_2B) if two else (CAM_A, None)
    xy_a = np.zeros((S_, cap, 2), np.float32); xy_b = np.zeros((S_, cap, 2), np.float32)
    pairs = np.zeros((S_, cap, 2), np.uint32)
    ia = [S_ - 1 - s for s in range(S_)]
    ib = [(s * 2 + 1) % S_ for s in range(S_)] if S_ % 2 else ia
    total = sum(min(size, cap) for size in sizes)
    rows = rng.permutation(total)                          # where the scenes' points lie in the world table
    world = np.zeros((total, 4))
    labels, at = [], 0
    for s, size in enumerate(sizes):
        n = min(size, cap)
        rng = np.random.default_rng([seed, s, tries[s] if tries else 0])
        lab = labels_of(s, n) if labels_of is not None else None
        lab = np.where(np.arange(n) % 5 == 4, -1, 0) if lab is None else lab
        labels.append(lab)
        fa = rng.permutation(cap)[:n]; fb = rng.permutation(cap)[:n]
        if two:
            xy_a[ia[s]] = rng.integers(0, 4096, (cap, 2)) / 4.0
            xy_b[ib[s]] = rng.integers(0, 4096, (cap, 2)) / 4.0
        else:
            xy_a[ia[s]] = rng.uniform(0, 1200, (cap, 2))
        pairs[s, :n, 0] = fa
        pairs[s, :n, 1] = fb if two else rows[at:at + n]
        if not two:
            world[rows[at:at + n]] = _projective(np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.2, 1.2, n), rng.uniform(4, 9, n)], 1))
        for g in range(int(lab.max(initial=-1)) + 1):
            m = np.flatnonzero(lab == g)
            px = xy_a[ia[s], fa[m]].astype(np.float64)
            fx, fy, cx, cy, skew = cam_a
            y = (px[:, 1] - cy) / fy
            ray = np.stack([(px[:, 0] - cx - skew * y) / fx, y, np.ones(len(m))], 1)
            if two:
                R = RZ90 if (g + s) % 2 else np.eye(3)
                t = np.array([rng.integers(1, 8) / 4.0 * (-1) ** g, rng.integers(1, 8) / 8.0, 0.0])
                w = rng.integers(8, 17, len(m)) / 64.0
                q = ray @ R.T + w[:, None] * t
                pb = project(cam_b, q)
                assert np.array_equal(pb.astype(np.float32).astype(np.float64), pb)
                xy_b[ib[s], fb[m]] = pb
            else:
                R, t = _rodrigues((rng.random(3) - 0.5) * 0.3), (rng.random(3) - 0.5) * 0.8
                Xc = ray * rng.uniform(4, 9, (len(m), 1))
                world[rows[at + m]] = _projective((Xc - t) @ R) * rng.uniform(0.5, 2.0, (len(m), 1))
        at += n
    return Batch(name, family, cap, cam_a, cam_b, xy_a, xy_b if two else None, None if two else world, pairs,
                 np.array(sizes, np.uint32), ia, ib if two else None, prm, n_hyp, shuffle, labels)


def tie_labels(n, seed=569, i=545, j=1088):
    """Two groups arranged by POSITION in the shuffled order of (seed, n), where matches i and j have equal keys and i comes
    first: the positions up to i's hold as many matches of group 0 as of group 1, i among the former; j, the next position,
    is unrelated.  A block that ends with i leaves the groups tied; with the pair exchanged group 0 is one behind."""
    order = shuffle_order(seed, n)
    p = int(np.flatnonzero(order == i)[0])
    assert order[p + 1] == j
    lab = np.zeros(n, np.int64)
    for pos, m in enumerate(order):
        lab[m] = (p - pos) % 2 if pos <= p else (pos % 2)
    if (p + 1) % 2:
        lab[order[0]] = -1
    lab[j] = -1
    return lab


TIE_N, TIE_BLOCK = 1106, 1003        # shuffle_order(569, 1106) has match 545 at position 1002 and match 1088 behind it


def _undrawn_unrelated(seed, n_hyp, K):
    """labels of a scene whose unrelated matches are a third of those no initial sample draws: every sample then lies inside
    the one group, every pose a solver returns for it is the planted one or has its own sample as support, and every count
    ties: the order of the ids decides everything"""
    def labels(s, n):
        lab = np.zeros(n, np.int64)
        if n >= K:
            drawn = np.unique(samples_of(scene_seed(seed, s), n, n_hyp, K))
            free = np.setdiff1d(np.arange(n), drawn)
            lab[free[free % 3 == 0]] = -1
        return lab
    return labels


def designed_batches(seeds=(901, 910, 921, 930, 940), tries=((0, 0, 0, 0), (2, 0, 0, 0, 0, 0, 0, 1, 0), (1, 0, 0, 0, 0, 0, 0, 1, 0), None, (0, 0, 0, 2, 0, 0, 1, 0, 3))):
    """name -> Batch: scenes that end while others go on (0, K - 1, K, 17, 256, 257, the capacity, a count above it), keypoint
    blocks in a permuted order, a shuffled order whose keys tie at a block's edge, re-sampling rounds that find a scene
    finished."""
    out = [
        # scene 0: caller's seed 569, 1 106 matches: the keys of matches 545 and 1 088 tie; the first block ends with 545 and
        # leaves the two groups tied, cap 1 keeps the lower id; 1 088 in its place would leave group 1 alone in front
        _batch("p3p/shuffle_tie", "p3p", seeds[0], [TIE_N, 3, 17, 0], 1200,
               Params(block_size=TIE_BLOCK, init_blocks=1, max_candidates=1, seed=569), 64, True,
               lambda s, n: tie_labels(n) if s == 0 else np.zeros(n, np.int64), tries[0]),
        _batch("p3p/ragged", "p3p", seeds[1], [200, 0, 2, 3, 17, 256, 257, 512, 513], 512,
               Params(block_size=50, init_blocks=2, max_candidates=16, halve=True, sprt=True, estimations_per_block=2, seed=124), 32, True,
               _undrawn_unrelated(124, 32, 3), tries[1]),
        _batch("two_view/ragged", "two_view", seeds[2], [300, 0, 7, 8, 17, 256, 257, 512, 513], 512,
               Params(block_size=40, init_blocks=1, max_candidates=24, sprt=True, estimations_per_block=2, seed=1061), 16, True,
               _undrawn_unrelated(1061, 16, 8), tries[2]),
        # halving without re-sampling ends the loop of the whole call at cap 1 (after block init_blocks + 3): the scenes that
        # are finished by then ran all their blocks, the others count only what ran; the first one in index order
        _batch("two_view/halving_stop", "two_view", seeds[3], [100, 8, 17, 40, 0, 64, 65, 128, 129], 128,
               Params(block_size=16, init_blocks=1, max_candidates=8, halve=True, seed=7), 16, False, _undrawn_unrelated(7, 16, 8), tries[3]),
        _batch("p3p/halving_stop", "p3p", seeds[4], [100, 3, 17, 40, 0, 80, 81, 128, 129], 128,
               Params(block_size=16, init_blocks=2, max_candidates=8, halve=True, sprt=True, seed=1061), 32, True,
               _undrawn_unrelated(1061, 32, 3), tries[4]),
    ]
    return {b.name: b for b in out}
