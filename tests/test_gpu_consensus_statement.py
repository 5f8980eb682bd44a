"""The consensus stage on the DEVICE against tests/consensus_statement.py on its catalogue of designed scenes.

rs_essential_arrsac, rs_p3p_arrsac and both *_batch_device entries run every designed case; the statement runs the same
case with the device as its pose provider (the exhaustive entry of the same estimator on a second context, then
rs_debug_poses) and its own sampler, shuffle, float64 residual predicates and loop.  Required: equal winner id, inlier list,
inlier count and all five fields of rs_arrsac_stats; the returned pose equals the provider's pose of that id bit for bit; the
batched scenes' calibrated bearings (1e-14) and scoring order equal the statement's; both margin conditions and every closed
form of the catalogue hold on the device's poses too."""
import ctypes as C

import numpy as np
import pytest

import consensus_statement as S

pytestmark = pytest.mark.gpu

CASES = S.designed_cases()
BATCHES = S.designed_batches()
STATS = np.dtype([("poses", "<u4"), ("survivors", "<u4"), ("blocks", "<u4"), ("reserved", "<u4"),
                  ("residuals_evaluated", "<u8"), ("residuals_exhaustive", "<u8")])


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cv_amd import build
    build.build()
    return True


def device_provider(family, first, second, max_samples):
    """samples -> (poses, ok) through rs_p3p_batch / rs_essential_batch and rs_debug_poses on a context of its own"""
    from cv_amd.ransac import EssentialConsensus
    slots = S.SLOTS[family]
    ctx = EssentialConsensus(max(len(first), 8), slots * max(max_samples, 1))

    def provider(smp):
        smp = np.ascontiguousarray(smp, np.uint32)
        if family == "p3p":
            ctx.p3p_model_inliers(first, second, smp, S.THR)
        elif family == "five_point":
            ctx.five_point_model_inliers(first, second, smp, S.THR)
        else:
            ctx.model_inliers(first, second, smp, S.THR)
        return ctx.poses(slots * len(smp))
    provider.close = ctx.close
    return provider


def _params(cons, prm, n_hyp, family="two_view"):
    return cons.make_params(prm.threshold, n_hypotheses=n_hyp, seed=prm.seed, block_size=prm.block_size, init_blocks=prm.init_blocks,
                            max_candidates=prm.max_candidates, bound=prm.bound, sprt=prm.sprt, sprt_delta=prm.sprt_delta,
                            sprt_ratio=prm.sprt_ratio, estimations_per_block=prm.estimations_per_block, halve=prm.halve,
                            estimator="five_point" if family == "five_point" else "eight_point")


def device_run(case):
    """rs_p3p_arrsac / rs_essential_arrsac on a context that is exactly full: (best_id, pose, inliers, stats) — the stats also
    where no model comes out"""
    from cv_amd import _lib
    from cv_amd._device import call
    from cv_amd.ransac import EssentialConsensus
    n = len(case.first)
    rounds = -(-n // case.prm.block_size)
    cons = EssentialConsensus(max(n, 8), S.SLOTS[case.family] * (case.n_hyp + case.prm.estimations_per_block * rounds))
    prm = _params(cons, case.prm, case.n_hyp, case.family)
    a = np.ascontiguousarray(case.first, np.float64); b = np.ascontiguousarray(case.second, np.float64)
    si = None if case.samples is None else np.ascontiguousarray(case.samples, np.uint32)
    pose = np.zeros((3, 4), np.float64); best = C.c_uint32(); ninl = C.c_uint32()
    inl = np.zeros(max(n, 1), np.uint32)
    st = _lib.ArrsacStats()
    call("rs_p3p_arrsac" if case.family == "p3p" else "rs_essential_arrsac", cons._h, a.ctypes.data, b.ctypes.data, n,
         None if si is None else si.ctypes.data, prm, pose.ctypes.data, C.byref(best), inl.ctypes.data, n, C.byref(ninl), st)
    stats = {k: int(getattr(st, k)) for k in ("poses", "survivors", "blocks", "residuals_evaluated", "residuals_exhaustive")}
    cons.close()
    return best.value, pose, inl[:ninl.value].copy(), stats


@pytest.mark.parametrize("name", sorted(CASES))
def test_single_scene_entries_equal_the_statement(gpu, name):
    case = CASES[name]
    provider = device_provider(case.family, case.first, case.second, max(case.n_hyp, case.prm.estimations_per_block))
    want = S.consensus(case.family, case.first, case.second, case.prm, case.initial_samples(), provider)
    S.check_closed_form(case, want)                         # margins and closed forms on the device's own poses
    provider.close()
    best, pose, inl, stats = device_run(case)
    assert best == want.best_id, (name, best, want.best_id, stats, want.stats)
    assert np.array_equal(inl, want.inliers), (name, inl, want.inliers)
    assert stats == want.stats, (name, stats, want.stats)
    if best != S.NONE:
        assert pose.tobytes() == np.ascontiguousarray(want.pose).tobytes(), (name, pose, want.pose)


@pytest.mark.parametrize("family", ["p3p", "two_view", "five_point"])
def test_fewer_matches_than_a_minimal_sample_are_refused(gpu, family):
    """n == K - 1 through the single-scene entries: AKZ_E_INVALID (the batched entries give such a scene "no model")."""
    from cv_amd._lib import AkzError
    from cv_amd.ransac import EssentialConsensus
    K = S.SAMPLE_SIZE[family]
    first, second, _, _ = S._scene(family, 5, S._runs((0, K - 1)))
    cons = EssentialConsensus(8, 40)
    with pytest.raises(AkzError):
        cons.arrsac_model_inliers(first, second, S.THR, n_hypotheses=4, block_size=2, p3p=family == "p3p",
                                  estimator="five_point" if family == "five_point" else "eight_point")
    cons.close()


def _kp(xy):
    from cv_amd._lib import KP_DTYPE
    k = np.zeros(xy.shape[:-1], KP_DTYPE)
    k["x"], k["y"] = xy[..., 0], xy[..., 1]
    return k


@pytest.mark.parametrize("name", sorted(BATCHES))
def test_batched_entries_equal_the_statement(gpu, name):
    import torch
    from cv_amd.ransac import EssentialConsensus
    b = BATCHES[name]
    p3p = b.family == "p3p"
    K = 3 if p3p else 8
    S_, cap = len(b.npairs), b.cap
    dev = torch.device("cuda", 0)

    def up(x, dt):
        return torch.from_numpy(np.ascontiguousarray(x).view(dt)).to(dev)
    d_ka = up(_kp(b.xy_a).view(np.uint8).reshape(len(b.xy_a), cap, 28), np.uint8)
    d_kb = None if p3p else up(_kp(b.xy_b).view(np.uint8).reshape(len(b.xy_b), cap, 28), np.uint8)
    d_world = up(b.world, np.float64) if p3p else None
    d_pairs = up(b.pairs, np.int32)
    d_np = up(b.npairs, np.int32)
    d_pose = torch.zeros((S_, 12), dtype=torch.float64, device=dev)
    d_best = torch.zeros((S_,), dtype=torch.int32, device=dev)
    d_inl = torch.zeros((S_, cap), dtype=torch.int32, device=dev)
    d_ninl = torch.zeros((S_,), dtype=torch.int32, device=dev)
    d_stats = torch.zeros((S_, STATS.itemsize), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    E = b.prm.estimations_per_block
    cons = EssentialConsensus(cap, b.n_hyp + E * -(-cap // b.prm.block_size))     # exactly full
    cons.reserve(S_)
    prm = _params(cons, b.prm, b.n_hyp)
    for rep in range(2):                                     # the second call runs over the first one's leftovers
        if p3p:
            cons.p3p_model_inliers_batch_device(d_ka.data_ptr(), cap, b.ia, d_pairs.data_ptr(), d_np.data_ptr(), d_world.data_ptr(),
                                                len(b.world), cons.camera(b.cam_a + (None,)), prm, d_pose.data_ptr(), d_best.data_ptr(),
                                                d_inl.data_ptr(), d_ninl.data_ptr(), d_stats.data_ptr(), shuffle=b.shuffle)
        else:
            cons.model_inliers_batch_device(d_ka.data_ptr(), d_kb.data_ptr(), cap, b.ia, b.ib, d_pairs.data_ptr(), d_np.data_ptr(),
                                            cons.camera(b.cam_a + (None,)), cons.camera(b.cam_b + (None,)), prm, d_pose.data_ptr(),
                                            d_best.data_ptr(), d_inl.data_ptr(), d_ninl.data_ptr(), d_stats.data_ptr(), shuffle=b.shuffle)
    cons.sync()
    pose = d_pose.cpu().numpy(); best = d_best.cpu().numpy().view(np.uint32); inl = d_inl.cpu().numpy().view(np.uint32)
    ninl = d_ninl.cpu().numpy().view(np.uint32)
    st = d_stats.cpu().numpy().view(STATS).reshape(S_)
    for s in range(S_):
        n = b.n(s)
        ga, gb, go = cons.scene_world(s, cap) if p3p else cons.scene(s, cap)
        first, second = b.scene(s)
        assert len(ga) == n, (name, s, len(ga), n)
        if n:
            assert np.abs(ga - first).max() < 1e-14 and np.abs(gb - second).max() < 1e-14, (name, s)
        provider = device_provider(b.family, ga, gb, max(b.n_hyp, E)) if n >= K else None
        want, order = S.batch_scene(b, s, ga, gb, provider)
        if provider:
            provider.close()
        got = {k: int(st[k][s]) for k in want.stats}
        assert S.margins_hold(want, b.prm.threshold), (name, s, want.below, want.above, want.sprt_margin)
        if b.shuffle and n >= K:
            assert np.array_equal(go, order), (name, s)
        assert best[s] == want.best_id, (name, s, best[s], want.best_id, got, want.stats)
        assert ninl[s] == len(want.inliers) and np.array_equal(inl[s, :ninl[s]], want.inliers), (name, s)
        assert got == want.stats, (name, s, got, want.stats)
        if want.best_id != S.NONE:
            assert pose[s].tobytes() == np.ascontiguousarray(want.pose).tobytes(), (name, s)
            assert np.array_equal(want.inliers, np.flatnonzero(b.labels[s] == int(b.labels[s][want.inliers[0]]))), (name, s)
    cons.close()
