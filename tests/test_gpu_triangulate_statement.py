"""The triangulation kernels (cv_amd/csrc/rs_triangulate.hip) held to the independent float64 statement of the stage
(tests/triangulate_statement.py) on its catalogue — the K1 + skew camera, every element of settings_grid x thresholds, the
prefixes around the 256-lane block, the ragged capacity of 300 — and, on the same inputs, to the host build of
include/akz_triangulate_math.h bit for bit.  tests/test_triangulate_statement.py holds the host build to the statement."""
import ctypes as C

import numpy as np
import pytest

import triangulate_checker as tc
import triangulate_statement as S
from test_triangulate_statement import (MERGE_SETTINGS, POISON, catalogue, host_landmarks, host_merged, host_pairs, host_settings,
                                        judge_merged, judge_pairs, kps_of, landmark_names, landmark_runs)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cv_amd import build
    build.build()
    return torch


def _dev(torch, a, view=None):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(view) if view is not None else a).to(torch.device("cuda", 0))


def _kps_dev(torch, xy):
    kps = kps_of(xy)
    return _dev(torch, kps.view(np.uint8).reshape(kps.shape + (28,)))


def _params(st):
    from cv_amd import triangulation
    return triangulation.make_params(st.eps, st.max_sweeps, st.robust_minimum_observations, st.n_views, st.min_cos)


class _DeviceTable:
    """a statement Table where the kernels read it"""

    def __init__(self, torch, t):
        self.t = t
        self.kps, self.poses = _kps_dev(torch, t.xy), _dev(torch, t.poses)
        self.start, self.obs = _dev(torch, t.start, np.int32), _dev(torch, t.obs, np.int32)

    def head(self, cons):
        """the arguments every table entry point begins with"""
        t = self.t
        return (cons._h, self.kps, t.cap, t.n_blocks, self.poses, cons.camera(t.cam), self.start, self.obs, t.n_obs)


def test_landmark_table_against_the_statement(gpu):
    """rs_triangulate_landmarks_device on table(513): the prefixes 1, 255, 256, 257 and 513 with and without a reason array
    (the poisoned rows behind stay as they were), then the whole table once per element of settings_grid x thresholds (132
    launches), every launch judged over all 513 rows against the statement and, in bytes, against the host build; a sweep
    limit of 1.  Reasons 0, 1, 2, 4, 5, 6 all occur, 3 under the sweep limit, and each of the 16 chosen landmarks flips
    between its two thresholds.
    Measured on the MI355X: reasons over the sweep [16092, 22308, 27724, 0, 464, 468, 660], 16 of 16 flips, worst
    sin(angle) / bound of the device 3.3e-4 — the host build's own figure, as its bytes are the device's."""
    torch = gpu
    from cv_amd._device import call
    from cv_amd.ransac import EssentialConsensus
    cat = catalogue()
    t, pre = cat["table"], cat["prepared"]
    n_all = t.n_landmarks
    cons = EssentialConsensus(8, 1)
    dt = _DeviceTable(torch, t)
    dev = dt.kps.device
    d_world = torch.empty((n_all + 3, 4), dtype=torch.float64, device=dev)
    d_reason = torch.empty((n_all + 3,), dtype=torch.uint8, device=dev)

    def launch(st, n, with_reason=True):
        d_world.fill_(POISON); d_reason.fill_(99)
        torch.cuda.synchronize()
        call("rs_triangulate_landmarks_device", *dt.head(cons), n, _params(st), d_world, d_reason if with_reason else None, None)
        cons.sync()
        world, reason = d_world.cpu().numpy(), d_reason.cpu().numpy()
        assert (world[n:] == POISON).all() and (reason[n if with_reason else 0:] == 99).all(), n
        return world[:n], reason[:n]

    default = S.Settings()
    for n in (1, 255, 256, 257, 513):
        rows = S.landmarks(t, default, n_landmarks=n, prepared=pre)
        want, want_r = host_landmarks(t, default, n=n)
        world, reason = launch(default, n)
        S.hold(landmark_names(n, f"prefix {n}"), world, reason, rows, default)
        assert world.tobytes() == want.tobytes() and np.array_equal(reason, want_r), n
        world, _ = launch(default, n, with_reason=False)
        assert world.tobytes() == want.tobytes(), n
    worst, hist, reasons_at = 0.0, np.zeros(7, np.int64), {}
    for what, st in landmark_runs(cat):
        world, reason = launch(st, n_all)
        worst = max(worst, S.hold(landmark_names(n_all, what), world, reason, S.landmarks(t, st, prepared=pre), st))
        want, want_r = host_landmarks(t, st)
        assert world.tobytes() == want.tobytes() and np.array_equal(reason, want_r), what
        hist += np.bincount(reason, minlength=7)
        reasons_at[(st.robust_minimum_observations, st.n_views, st.min_cos)] = reason
    print("launches:", len(reasons_at), "reasons 0..6 over the sweep:", hist.tolist())
    assert len(reasons_at) == 132 and (hist[[0, 1, 2, 4, 5, 6]] > 0).all() and hist[3] == 0
    flips = 0
    for l in cat["chosen"]:
        lo, hi = S.around(pre[l].best)
        flips += int(reasons_at[(3, 0xFFFFFFFF, lo)][l] != 2 and reasons_at[(3, 0xFFFFFFFF, hi)][l] == 2)
    print("threshold flips:", flips, "of", len(cat["chosen"]))
    assert flips == len(cat["chosen"]) == 16
    st1 = S.Settings(max_sweeps=1)
    world, reason = launch(st1, n_all)
    S.hold(landmark_names(n_all, "one sweep"), world, reason, S.landmarks(t, st1, prepared=pre), st1)
    want, want_r = host_landmarks(t, st1)
    assert world.tobytes() == want.tobytes() and np.array_equal(reason, want_r) and (reason == 3).sum() > 50
    print("reasons 0..6 under a sweep limit of 1:", np.bincount(reason, minlength=7).tolist())
    print(f"worst sin(angle) / bound of the device: {worst:.3g}")
    cons.close()


def test_merge_candidates_against_the_statement(gpu):
    """rs_triangulate_merged_device on merge_case(): capacity 300 (a ragged second block of lanes), the K1 + skew camera, the
    default settings and (3, 2): the rows written and no others, reasons and points against the statement, bytes against the
    host build.  Measured on the MI355X: worst sin(angle) / bound of the device 3.4e-4, the host build's own figure."""
    torch = gpu
    from cv_amd._device import call
    from cv_amd.ransac import EssentialConsensus
    cat = catalogue()
    mc, pre = cat["merge"], cat["merge_prepared"]
    t = mc.table
    F = mc.decision.shape[0]
    cons = EssentialConsensus(8, 1)
    dt = _DeviceTable(torch, t)
    d_best, d_dec, d_ok = _dev(torch, mc.best, np.int32), _dev(torch, mc.decision, np.int32), _dev(torch, mc.merge_ok)
    worst = 0.0
    for what, st in MERGE_SETTINGS:
        d_world = torch.full((mc.n_world + F * t.cap, 4), POISON, dtype=torch.float64, device=d_best.device)
        d_reason = torch.full((F, t.cap), 255, dtype=torch.uint8, device=d_best.device)
        torch.cuda.synchronize()
        call("rs_triangulate_merged_device", *dt.head(cons), t.n_landmarks, _params(st), d_best, d_dec, d_ok, F, mc.n_world, d_world,
             d_reason, None)
        cons.sync()
        world, reason = d_world.cpu().numpy(), d_reason.cpu().numpy()
        names, pts, why, rows = judge_merged(mc, world, reason, S.merged(mc, st, prepared=pre), what)
        worst = max(worst, S.hold(names, pts, why, rows, st))
        want, want_r = host_merged(mc, st)
        assert world.tobytes() == want.tobytes() and np.array_equal(reason, want_r), what
        print(what, "rows", len(rows), "reasons 0..6:", np.bincount(why, minlength=7).tolist())
    print(f"worst sin(angle) / bound of the device: {worst:.3g}")
    cons.close()


def test_two_view_inliers_against_the_statement(gpu):
    """rs_triangulate_pairs_batch_device on pair_case(): a context reserved for 5 scenes; pose, best_id and inliers uploaded by
    hand (the consensus is not what this tests); K1 on side a only; n_inliers 0, 1, 256 and 0xFFFF (clamped to 300), a scene
    without a model whose 300 rows stay poisoned, npairs above the capacity.  Rows, reasons and points against the statement,
    bytes against the host build.  Measured on the MI355X: reasons [456, 0, 0, 0, 0, 90, 11] (the short baselines put 90 inliers
    behind a camera), worst sin(angle) / bound of the device 2.3e-4, the host build's own figure."""
    torch = gpu
    from cv_amd.ransac import EssentialConsensus
    pc = catalogue()["pairs"]
    S_, cap = len(pc.npairs), pc.cap
    cons = EssentialConsensus(cap, 8)
    cons.reserve(S_)
    d_ka, d_kb = _kps_dev(torch, pc.xy_a), _kps_dev(torch, pc.xy_b)
    d_pairs, d_np = _dev(torch, pc.pairs, np.int32), _dev(torch, pc.npairs, np.int32)
    d_pose, d_best = _dev(torch, pc.pose), _dev(torch, pc.best_id, np.int32)
    d_inl, d_ninl = _dev(torch, pc.inliers, np.int32), _dev(torch, pc.n_inliers, np.int32)
    d_pts = torch.full((S_, cap, 4), POISON, dtype=torch.float64, device=d_ka.device)
    d_why = torch.full((S_, cap), 255, dtype=torch.uint8, device=d_ka.device)
    torch.cuda.synchronize()
    st = S.Settings()
    cons.triangulate_inliers(d_ka, d_kb, cap, pc.ia, pc.ib, d_pairs, d_np, cons.camera(pc.cam_a), cons.camera(pc.cam_b), d_pose, d_best,
                             d_inl, d_ninl, d_pts, d_why, params=_params(st))
    cons.sync()
    pts, why = d_pts.cpu().numpy(), d_why.cpu().numpy()
    got = {(int(s), int(i)): (pts[s, i], why[s, i]) for s, i in np.argwhere(why != 255)}
    rows = S.pairs(pc, st)
    names, p, r, rws = judge_pairs(got, rows, "default")
    worst = S.hold(names, p, r, rws, st)
    untouched = why == 255
    assert (pts[untouched] == POISON).all() and untouched[3].all() and untouched[0].all() and untouched[1, 1:].all()
    want = host_pairs(pc, st)
    assert set(want) == set(got)
    for k, (wp, wr) in want.items():
        assert got[k][0].tobytes() == wp.tobytes() and got[k][1] == wr, k
    print("rows", len(rows), "reasons 0..6:", np.bincount(np.array(r, np.int64), minlength=7).tolist())
    print(f"worst sin(angle) / bound of the device: {worst:.3g}")
    cons.close()


def test_single_lists_against_the_statement(gpu):
    """rs_triangulate_observations on list_case(n), n = 0, 1, 2, 3, 48: the statement's reason and point, the host build's
    bytes.  Measured on the MI355X: worst sin(angle) / bound of the device 1.7e-4, the host build's own figure."""
    assert gpu is not None
    from cv_amd._device import call
    from cv_amd.ransac import EssentialConsensus
    cons = EssentialConsensus(8, 1)
    st = S.Settings()
    worst = 0.0
    for n, (P, B) in catalogue()["lists"].items():
        P, B = np.ascontiguousarray(P.reshape(-1, 12)), np.ascontiguousarray(B)
        point, reason = np.full(4, POISON), C.c_uint8(99)
        call("rs_triangulate_observations", cons._h, P.ctypes.data if n else None, B.ctypes.data if n else None, n, _params(st),
             point.ctypes.data, C.byref(reason))
        worst = max(worst, S.hold([f"list/n={n}"], [point], [reason.value], [S.observations(P, B, st)], st))
        want, want_r = tc.observations(P, B, st=host_settings(st))
        assert point.tobytes() == want.tobytes() and reason.value == want_r, n
    print(f"worst sin(angle) / bound of the device: {worst:.3g}")
    cons.close()
