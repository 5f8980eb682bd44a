"""tests/consensus_statement.py on the CPU: the catalogue's closed forms against the statement, the statement's sampler,
scene seed and shuffle against rs_arrsac_samples and the oracle's, oracle/arrsac_oracle.c against the statement on every
designed case (winner, inlier list, survivors, blocks, poses made, residuals evaluated), and the statement with one rule
altered against the unaltered oracle on the case designed for that rule: every case can fail.

The pose provider here is the oracle's solvers (eight_point / essential_poses / p3p_poses); the loop, the sampler, the
shuffle and the residual predicates are the statement's own."""
import ctypes as C

import numpy as np
import pytest

import consensus_statement as S

CASES = S.designed_cases()


def oracle_provider(O, case):
    a, b = case.first, case.second

    def provider(smp):
        if case.family == "five_point":
            # the host build of include/akz_five_point_math.h (tests/five_point_checker.py), then the oracle's E -> four poses
            import five_point_checker as ck
            E, ns = ck.essentials(a, b, smp)
            poses = np.zeros((len(smp) * 10, 4, 3, 4)); ok = np.zeros((len(smp) * 10, 4), bool)
            for h in range(len(smp)):
                for k in range(int(ns[h])):
                    P = O.essential_poses(E[h, k])
                    if P is not None:
                        poses[10 * h + k], ok[10 * h + k] = P, True
            return poses, ok
        poses = np.zeros((len(smp), 4, 3, 4)); ok = np.zeros((len(smp), 4), bool)
        for h, s in enumerate(np.asarray(smp, np.int64)):
            if case.family == "p3p":
                P = O.p3p_poses(a[s], b[s])[:4]
            else:
                E = O.eight_point(a[s], b[s])
                P = None if E is None else O.essential_poses(E)
                P = np.zeros((0, 3, 4)) if P is None else P
            poses[h, :len(P)] = P
            ok[h, :len(P)] = True
        return poses, ok
    return provider


def run_statement(O, case, alter=()):
    return S.consensus(case.family, case.first, case.second, case.prm, case.initial_samples(), oracle_provider(O, case), alter=alter)


def run_oracle(O, case):
    """orc_arrsac with the stats kept where no model comes out: (best_id, pose, inliers, stats)"""
    prm = O._arrsac_params(case.prm.threshold, case.n_hyp, case.prm.seed, case.prm.block_size, case.prm.init_blocks,
                           case.prm.max_candidates, case.prm.bound, case.prm.sprt, case.prm.sprt_delta, case.prm.sprt_ratio,
                           case.prm.estimations_per_block, case.prm.halve)
    a = np.ascontiguousarray(case.first, np.float64); b = np.ascontiguousarray(case.second, np.float64)
    n = len(a)
    si = None if case.samples is None else np.ascontiguousarray(case.samples, np.uint32)
    pose = np.zeros((3, 4)); best = C.c_uint32(S.NONE); ninl = C.c_uint32(0)
    inl = np.zeros(max(n, 1), np.uint32); st = np.zeros(5, np.uint32)
    O.lib().orc_arrsac(int(case.family == "p3p"), a.ctypes.data, b.ctypes.data, n, None if si is None else si.ctypes.data,
                       C.byref(prm), pose.ctypes.data, C.byref(best), inl.ctypes.data, C.byref(ninl), st.ctypes.data)
    stats = dict(residuals_evaluated=int(st[0]) | (int(st[1]) << 32), survivors=int(st[2]), blocks=int(st[3]), poses=4 * int(st[4]))
    return best.value, pose, inl[:ninl.value].copy(), stats


@pytest.fixture(scope="module")
def runs(oracle):
    """the statement's run of every case, made once"""
    return {name: run_statement(oracle, case) for name, case in CASES.items()}


def test_the_catalogue_reaches_every_rule():
    names = set(CASES)
    for fam in ("p3p", "two_view"):
        for rule in ("bound/stays", "bound/retired", "winner/lowest_id", "winner/lowest_hypothesis", "blocks/size_1", "blocks/n_eq_K",
                     "halve/init_0", "halve/shift_past_31", "halve/resampling_goes_on"):
            assert f"{fam}/{rule}" in names
    for M in (1, 63, 64, 65, 255, 256, 257):
        assert {f"p3p/cap/ties_{M}_inside", f"p3p/cap/ties_{M}_outside", f"p3p/count/{M}"} <= names
    assert {"five_point/sixteen_samples", "p3p/resample/overtakes", "two_view/degenerate/one_match_repeated", "p3p/no_model/E_2",
            "p3p/cap/budget_skips_retired", "p3p/cap/last_bin_2048"} <= names
    for H in (1, 63, 64, 65, 255, 256, 257):
        assert {f"two_view/count/{H}", f"p3p/count_given/{H}"} <= names
    assert all(c.prm.threshold == 1e-9 for c in CASES.values())


@pytest.mark.parametrize("name", sorted(CASES))
def test_closed_forms_and_margins(runs, name):
    """Every case's expectation, derived from the labels and the order alone, holds on the statement's run; no residual lies
    between thr / 100 and 100 thr; no SPRT decision lies within 1e-9 of the ratio."""
    S.check_closed_form(CASES[name], runs[name])


def test_the_population_caps_straddle_the_live_count(runs):
    """cap == live count (nothing is cut) and cap == live count - 1 (the last pose by id goes) are both in the catalogue:
    for P3P the number of live poses is the solver's, so it is read from the run."""
    for fam, caps in (("p3p", range(3, 13)), ("two_view", (23, 24))):
        live = {int(runs[f"{fam}/cap/population_{M}"].ok.sum()) for M in caps}
        assert len(live) == 1
        live = live.pop()
        assert live in caps and live - 1 in caps, (fam, live)
        after_block_1 = 8 * live                                   # every pose scored on the first block of 8
        assert runs[f"{fam}/cap/population_{live}"].stats["residuals_evaluated"] >= after_block_1


def test_five_point_layout(runs):
    """ten slots a sample, unused slots never live, ids (10 sample + solution) 4 + pose, the cap counts poses"""
    res = runs["five_point/sixteen_samples"]
    assert res.ok.shape == (160, 4) and res.stats["poses"] == 640 and res.stats["residuals_exhaustive"] == 640 * 14
    n_sol = res.ok.any(axis=1).reshape(16, 10).sum(1)
    assert (n_sol >= 1).all() and (n_sol < 10).any()                # some slots are unused ...
    for h in range(16):
        assert not res.ok[10 * h + n_sol[h]:10 * (h + 1)].any()    # ... the ones behind a sample's solutions
    assert all(res.ok[pid // 4, pid % 4] for pid in res.counts)     # ... and none of them is live
    assert res.best_id < 40 and res.stats["survivors"] <= 6        # sample 0; at most max_candidates POSES survive block 1


@pytest.mark.parametrize("seed", range(8))
def test_ranking_the_cap_after_the_retirements_changes_nothing(seed):
    """Bound and SPRT retire by count alone, from the far end of the cap's ranking.  So the survivors are the same whether the
    cap ranks the population before this block's retirements (the rule) or after them: random count vectors, both ways."""
    rng = np.random.default_rng(seed)
    for _ in range(300):
        n_alive, cap = int(rng.integers(1, 40)), int(rng.integers(1, 40))
        best = int(rng.integers(1, 4000))
        count = rng.integers(0, best + 1, n_alive); count[rng.integers(n_alive)] = best
        floor = int(rng.integers(0, best + 1))                    # bound and SPRT keep exactly the counts >= floor
        passed = [i for i in range(n_alive) if count[i] >= floor]

        def survivors(population):
            if not (cap and len(population) > cap):
                return passed
            d = {i: min(best - int(count[i]), 2047) for i in population}
            T = sorted(d.values())[cap - 1]
            budget = cap - sum(1 for v in d.values() if v < T)
            at_T = [i for i in passed if d.get(i) == T][:budget]
            return [i for i in passed if d[i] < T or i in at_T]
        # (2047 and more share a bin: there the floor may split a bin, which is where the tie budget's rule is observable)
        if best - floor < 2047:
            assert survivors(list(range(n_alive))) == survivors(passed)


@pytest.mark.parametrize("name", sorted(n for n, c in CASES.items() if c.family != "five_point"))
def test_the_oracle_equals_the_statement(oracle, runs, name):
    case, want = CASES[name], runs[name]
    best, pose, inl, st = run_oracle(oracle, case)
    assert best == want.best_id, (name, best, want.best_id, st, want.stats)
    assert np.array_equal(inl, want.inliers), name
    if best != S.NONE:
        assert pose.tobytes() == np.ascontiguousarray(want.pose).tobytes(), name
    for key in ("survivors", "blocks", "poses", "residuals_evaluated"):
        assert st[key] == want.stats[key], (name, key, st, want.stats)


def test_sampler_scene_seed_and_shuffle(oracle):
    from cv_amd import build
    from cv_amd.ransac import EssentialConsensus
    build.build()
    for seed, n, K in ((0, 50, 3), (7, 8, 8), (2**64 - 3, 5000, 8), (12345, 3, 3), (99, 6, 5), (3, 8192, 5)):
        want = S.samples_of(seed, n, 40, K)
        assert np.array_equal(EssentialConsensus.arrsac_samples(seed, n, 40, K), want), (seed, n, K)
        for h in (0, 1, 39):
            assert oracle.arrsac_draw(seed, h, n, K).tolist() == want[h].tolist()
    for seed in (0, 569, 2**64 - 1):
        for s in (0, 1, 5, 65534):
            assert S.scene_seed(seed, s) == oracle.scene_seed(seed, s)
    for seed, n in ((569, 2048), (124, 3000), (1061, 1800), (5, 17), (5, 1), (5, 0)):
        assert np.array_equal(S.shuffle_order(seed, n), oracle.shuffle_order(seed, n)), (seed, n)


@pytest.mark.parametrize("seed,i,j,n", [(569, 545, 1088, 2048), (124, 609, 2822, 3000), (1061, 1332, 1703, 1800)])
def test_shuffle_keys_that_tie_keep_index_order(oracle, seed, i, j, n):
    keys = S.shuffle_keys(seed, n)
    assert keys[i] == keys[j]
    order = S.shuffle_order(seed, n).tolist()
    assert order.index(j) == order.index(i) + 1
    assert np.array_equal(oracle.shuffle_order(seed, n), order)
    # checker refuses: an order that is not stable differs from the oracle's exactly there
    bad = S.shuffle_order(seed, n, alter=("unstable_shuffle",)).tolist()
    assert bad.index(i) == bad.index(j) + 1 and not np.array_equal(oracle.shuffle_order(seed, n), bad)


def test_sprt_never_rejects_at_the_best_count_nor_below_delta():
    """Two guards of the written rule are consequences of the inequality, not additions to it: lhs(c = best) =
    -seen KL(eps || delta) <= 0 < ln ratio, and with eps <= delta lhs grows with c, so no pose below the best is rejected
    either.  (An altered statement without them cannot disagree with anything: there is no case for them to design.)"""
    for seen in range(2, 120):
        for best in range(1, seen):
            for delta in (0.01, 0.05, 0.5, 0.9):
                assert S.sprt_rejects(best, best, seen, delta, 0.0)[1] <= 1e-12
                if best / seen <= delta:
                    assert max(S.sprt_rejects(c, best, seen, delta, 0.0)[1] for c in range(best + 1)) <= 1e-12


REFUSALS = [
    ("ties_descending", "p3p/cap/ties_64_inside"),
    ("ties_descending", "p3p/cap/ties_257_outside"),
    ("budget_spent_on_retired", "p3p/cap/budget_skips_retired"),
    ("sprt_over_all_matches", "p3p/sprt/rejected_at_block_2"),
]


@pytest.mark.parametrize("alter,name", REFUSALS, ids=[f"{a}-{n}" for a, n in REFUSALS])
def test_checker_refuses(oracle, alter, name):
    """The statement with one rule altered disagrees with the unaltered oracle on the case designed for that rule."""
    case = CASES[name]
    got = run_statement(oracle, case, alter=(alter,))
    best, pose, inl, st = run_oracle(oracle, case)
    same = best == got.best_id and np.array_equal(inl, got.inliers) and all(st[k] == got.stats[k] for k in st)
    assert not same, (alter, name)


# ------------------------------------------------------------------------------------------------ batched entries
BATCHES = S.designed_batches()


def _kp(O, xy):
    k = np.zeros(len(xy), O.KP_DTYPE)
    k["x"], k["y"] = xy[:, 0], xy[:, 1]
    return k


def oracle_scene(O, b, s):
    """orc_arrsac_pairs / orc_p3p_arrsac_pairs on scene s of a batch"""
    pr = b.pairs[s, :b.n(s)]
    if b.family == "p3p":
        return O.p3p_arrsac_pairs(_kp(O, b.xy_a[b.ia[s]]), pr, b.world, b.cam_a + (None,), b.prm.threshold, b.n_hyp, scene=s,
                                  shuffle=b.shuffle, **b.prm.kw())
    return O.arrsac_pairs(_kp(O, b.xy_a[b.ia[s]]), _kp(O, b.xy_b[b.ib[s]]), pr, b.cam_a + (None,), b.cam_b + (None,), b.prm.threshold,
                          b.n_hyp, scene=s, shuffle=b.shuffle, **b.prm.kw())


class _Scene:
    def __init__(self, family, first, second):
        self.family, self.first, self.second = family, first, second


@pytest.mark.parametrize("name", sorted(BATCHES))
def test_the_oracle_equals_the_statement_on_batched_scenes(oracle, name):
    """Every scene of every designed batch: calibrated bearings (1e-14 between the statement's float64 and the oracle's), scoring
    order, winner, inlier list and the stats of every scene that has a minimal sample; both margin conditions."""
    b = BATCHES[name]
    K = 3 if b.family == "p3p" else 8
    for s in range(len(b.npairs)):
        want = oracle_scene(oracle, b, s)
        first, second = b.scene(s)
        ofirst = want["bearings" if b.family == "p3p" else "bearings_a"]
        osecond = want["world" if b.family == "p3p" else "bearings_b"]
        if b.n(s):
            assert np.abs(first - ofirst).max() < 1e-14 and np.abs(second - osecond).max() < 1e-14, (name, s)
        res, order = S.batch_scene(b, s, ofirst, osecond, oracle_provider(oracle, _Scene(b.family, ofirst, osecond)))
        assert S.margins_hold(res, b.prm.threshold), (name, s, res.below, res.above, res.sprt_margin)
        if b.shuffle and b.n(s) >= K:
            assert np.array_equal(order, want["order"]), (name, s)
        assert res.best_id == want["best_id"], (name, s, res.best_id, want["best_id"])
        assert np.array_equal(res.inliers, want["inliers"]), (name, s)
        if b.n(s) >= K:
            assert res.best_id != S.NONE and want["pose"].tobytes() == np.ascontiguousarray(res.pose).tobytes(), (name, s)
            for key in ("survivors", "blocks", "poses", "residuals_evaluated"):
                assert want["stats"][key] == res.stats[key], (name, s, key, want["stats"], res.stats)
            assert np.array_equal(res.inliers, np.flatnonzero(b.labels[s] == int(b.labels[s][res.inliers[0]]))), (name, s)


def test_checker_refuses_an_unstable_shuffle_on_the_tied_scene(oracle):
    """Scene 0 of the tie batch: with the two matches of equal key exchanged the other group wins."""
    b = BATCHES["p3p/shuffle_tie"]
    want = oracle_scene(oracle, b, 0)
    first, second = want["bearings"], want["world"]
    bad, order = S.batch_scene(b, 0, first, second, oracle_provider(oracle, _Scene("p3p", first, second)), alter=("unstable_shuffle",))
    assert sorted(order.tolist()) == list(range(b.n(0))) and not np.array_equal(order, want["order"])
    assert bad.best_id != want["best_id"] and not np.array_equal(bad.inliers, want["inliers"])
