"""A reconstruction's life on the device against the world it was drawn from (tests/reconstruction_life_statement.py): two
reconstructions are started (reconstruction.start_reconstructions) and grown by a batch of three frames each (Registration.
sharing_view -> consensus -> refine -> landmark_table.add_views_and_regenerate) on the tables, poses and world tables the phase
before left on the device, then normalised, joined through a bridging frame (reconstruction.merge_reconstructions) and exported
(export_reconstruction, read_ply), with exactly the one wait each chain documents.  After every phase the tensors are copied out and
held to the table invariants and, through one fitted similarity, to the ground truth within BOUNDS — which were measured from
the chain of statements on the CPU, not from the device.  The statement chain is not run here.  Run with -m gpu."""
import numpy as np
import pytest

import reconstruction_life_statement as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cv_amd import build
    build.build()
    return torch


@pytest.fixture(scope="module")
def cons(gpu):
    from cv_amd.ransac import EssentialConsensus
    c = EssentialConsensus(2048, 1024)
    c.reserve(2)
    yield c
    c.close()


@pytest.fixture(scope="module")
def reg(gpu):
    from cv_amd.registration import Registration
    cw = np.random.default_rng(1).integers(0, 256, (32, 64), dtype=np.uint8)
    p = L.SETTINGS["p3p"]
    r = Registration(gpu, L.CAP, 3, 3, cw, L.CAM6, threshold=p["threshold"], n_hypotheses=p["n_hypotheses"], max_candidates=p["max_candidates"],
                     estimations_per_block=p["estimations_per_block"], block_size=p["block_size"], seed=p["seed"])
    yield r
    r.close()


u32 = lambda t: t.cpu().numpy().view(np.uint32)


def parameters():
    from cv_amd.covisibility import Covisibility
    from cv_amd.pose_graph import PoseGraph
    from cv_amd.reconstruction import ObservationFilter
    from cv_amd.single_view import SingleViewRefiner
    from cv_amd.three_view import ThreeViewConstraints, ThreeViewInit
    S = L.SETTINGS
    return dict(tv=ThreeViewInit.params(**S["three_view"]), sv=SingleViewRefiner.params(**S["single_view"]),
                flt=ObservationFilter.params(**S["filter"]), cv=Covisibility.params(**S["covisibility"]),
                # (optimization_minimum_landmarks is ONE setting of the reference: the candidates and the constraints share it)
                tvc=ThreeViewConstraints.params(optimization_minimum_landmarks=S["covisibility"]["optimization_minimum_landmarks"], **S["constraint"]),
                pg=PoseGraph.params(**S["pose_graph"]))


def pools(torch, w):
    """the keypoint pool (block v = view v), the feature counts and the poses of all 13 blocks on the device"""
    from cv_amd import _lib
    dev = torch.device("cuda", 0)
    kps = np.zeros((L.N_VIEWS, L.CAP), _lib.KP_DTYPE)
    kps["x"], kps["y"], kps["size"] = w.px[..., 0], w.px[..., 1], 4.0
    d_kps = torch.from_numpy(kps.view(np.uint8).reshape(L.N_VIEWS, L.CAP, 28).copy()).to(dev)
    return d_kps, torch.from_numpy(w.counts.view(np.int32).copy()).to(dev), torch.zeros((L.N_VIEWS, 12), dtype=torch.float64, device=dev)


class Waits:
    """counts the waits of a chain as the neighbouring modules do: the consensus' sync and torch.cuda.synchronize"""

    def __init__(self, torch, monkeypatch, *contexts):
        self.seen = []
        for c in {type(c) for c in contexts}:
            monkeypatch.setattr(c, "sync", lambda s, _f=c.sync: (self.seen.append("rs_sync"), _f(s))[1])
        monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: self.seen.append("synchronize"))

    def take(self):
        got, self.seen[:] = list(self.seen), []
        return got


def start(torch, cons, w, prm, d_kps, d_poses, triple, view_base):
    """phase 1 for one reconstruction -> the StartResult"""
    from cv_amd.reconstruction import start_reconstructions
    dev = d_kps.device
    pairs, npairs = L.pair_lists(w, triple)
    d_pairs, d_npairs = torch.from_numpy(pairs.view(np.int32)).to(dev), torch.from_numpy(npairs.view(np.int32)).to(dev)
    a = dict(L.SETTINGS["arrsac"])
    arrsac = cons.make_params(a.pop("threshold"), **a)
    c, f, s = triple
    d_kps_dst, d_counts_dst = d_kps.clone(), torch.from_numpy(w.counts.view(np.int32).copy()).to(dev)
    r = start_reconstructions(torch, cons, d_kps, w.counts, L.CAP, cons.camera(L.CAM6), d_pairs, d_npairs, [c, c], [f, s], arrsac, [(0, 1)], [c], [f], [s],
                              L.N_VIEWS, view_base, d_kps_dst=d_kps_dst, d_counts_dst=d_counts_dst, d_poses=d_poses, minimum=L.SETTINGS["join_minimum"],
                              seed=L.SETTINGS["join_seed"], tv_params=prm["tv"], pg_params=prm["pg"], params=prm["flt"])
    return r


def started_state(r, d_poses, view_range):
    """what phase 1 left, copied out: the state the checks read and the tensors phase 2 goes on from"""
    from cv_amd import _lib
    from cv_amd.reconstruction import stopped_at
    assert u32(r.join.verdict).tolist() == [0] and u32(r.bootstrap[0]).tolist() == [_lib.RS_TV_OK] and u32(r.start.frame_verdict).tolist() == [0]
    assert stopped_at(u32(r.verdict)[0]) is None, stopped_at(u32(r.verdict)[0])
    n_rows, n_obs = (int(v) for v in u32(r.start.counts_out)[:2])
    kept, split = (int(v) for v in u32(r.filter.counts)[:2])
    st = L.SimpleNamespace(poses=d_poses.cpu().numpy().copy(), rows=L.rows_of(u32(r.filter.obs_start_out), u32(r.filter.obs_out).reshape(-1, 2), n_rows),
                           world=r.world.cpu().numpy()[:n_rows], reason=r.world_reason.cpu().numpy()[:n_rows],
                           table_rows=L.rows_of(u32(r.start.obs_start_out), u32(r.start.obs_out).reshape(-1, 2), n_rows),
                           table_map=u32(r.start.landmarks_out).reshape(L.N_VIEWS, L.CAP), views=[int(v) for v in u32(r.start.views_out)[0]],
                           tombstones=[], split=u32(r.filter.split_out).reshape(-1, 2)[:split])
    assert sum(len(x) for x in st.rows) == kept and view_range[0] <= min(st.views)
    return st


def grow(torch, reg, w, prm, d_kps, d_counts, d_poses, table, d_world, d_split, d_split_count, host_rows, frames, stored, view_range, regenerated=True):
    """phase 2 for one reconstruction: the frames' registration and add_views_and_regenerate behind it, no wait in between ->
    (RefineOutputs, AddViewsTensors, RegenerateResult)"""
    from cv_amd.landmark_table import add_views_and_regenerate
    dev = d_kps.device
    F = len(frames)
    best, decision = L.matcher_tables(w, frames, stored, L.map_of(host_rows))
    # what match_views() leaves, set by hand: the matcher's search is not what this test is about
    reg._cur, reg._fb, reg._calls = reg._sets[0], np.asarray(frames, np.uint32), 1
    reg._select(0)
    reg.best.copy_(torch.from_numpy(best.view(np.int32)).to(dev))
    reg.decision.copy_(torch.from_numpy(decision.view(np.int32)).to(dev))
    n_world = table.n_landmarks
    none = torch.zeros((F * L.CAP, 4), dtype=torch.float64, device=dev)
    none[:, 3] = -1.0
    world = torch.cat([d_world[:n_world], none])                      # room for the merge candidates' rows: every one "None"
    torch.cuda.current_stream(dev).synchronize()                      # the uploads above; the chain below waits once
    d_mask = reg.sharing_view(table)
    reg.consensus(d_kps, d_counts, world, n_world, d_merge_ok=d_mask, stream_to_wait=reg.rs_stream())
    out = reg.refine(d_poses, table.d_start, table.d_obs, n_world, params=prm["sv"], stream=torch.cuda.current_stream(dev))
    if not regenerated:                                               # add_views alone: the destination's side of a bridging frame
        added = reg.add_views(table, d_poses, d_split, d_split_count)
        reg.sync()
        return out, added, None, d_mask
    added, result = add_views_and_regenerate(torch, reg, table, d_kps, d_poses, np.array(view_range, np.uint32), d_split, d_split_count,
                                             targets=np.arange(*view_range, dtype=np.uint32), cv_params=prm["cv"], tvc_params=prm["tvc"],
                                             pg_params=prm["pg"], params=prm["flt"])
    return out, added, result, d_mask


def grown_state(out, added, result, d_mask, d_poses, old_rows):
    from cv_amd import _lib
    from cv_amd.reconstruction import stopped_at
    assert not d_mask.cpu().numpy().any()
    assert u32(out.verdict)[:added.n_frames].tolist() == [_lib.RS_SV_OK] * added.n_frames, u32(out.verdict).tolist()
    assert u32(added.frame_verdict).tolist() == [0] * added.n_frames and u32(added.call_verdict).tolist() == [0]
    assert stopped_at(u32(result.verdict)[0]) is None, stopped_at(u32(result.verdict)[0])
    n_rows, n_obs = (int(v) for v in u32(added.counts_out)[:2])
    kept, split = (int(v) for v in u32(result.filter.counts)[:2])
    table_rows = L.rows_of(u32(added.obs_start_out), u32(added.obs_out).reshape(-1, 2), n_rows)
    rows = L.rows_of(u32(result.filter.obs_start_out), u32(result.filter.obs_out).reshape(-1, 2), n_rows)
    assert sum(len(x) for x in rows) == kept and all(not r for r in L.rows_of(u32(added.obs_start_out), u32(added.obs_out).reshape(-1, 2))[n_rows:])
    return L.SimpleNamespace(poses=d_poses.cpu().numpy().copy(), rows=rows, world=result.world.cpu().numpy()[:n_rows],
                             reason=result.world_reason.cpu().numpy()[:n_rows], table_rows=table_rows,
                             table_map=u32(added.landmarks_out).reshape(L.N_VIEWS, L.CAP), views=sorted({b for r in rows for b, _ in r}),
                             tombstones=[l for l in range(len(old_rows)) if old_rows[l] and not table_rows[l]],
                             split=u32(result.filter.split_out).reshape(-1, 2)[:split])


def hold(scene, phase, w, st, view_range):
    """the invariants and aligned_errors against BOUNDS; every figure is printed before it is asserted"""
    broken = L.invariants(st.table_rows, view_range, st.table_map, st.tombstones) + L.invariants(st.rows, view_range, tombstones=st.tombstones)
    e = L.aligned_errors(st.poses, st.world, st.reason, L.truth_of(w, st.rows, st.views))
    bounds = L.BOUNDS[scene][phase]
    print(scene, w.seed, phase, view_range, {k: "%.3e (bound %.3e)" % (e[k], 4 * bounds[k]) for k in ("rotation", "centre", "point")},
          "left out %.3f" % e["left_out"], "scale %.4f" % e["similarity"][0], "broken", broken[:3])
    assert broken == []
    assert len(st.views) == L.VIEWS_AFTER[phase], st.views                       # no view may be left out
    assert e["left_out"] <= L.LEFT_OUT_CAP[scene], e["left_out"]
    for k in ("rotation", "centre", "point"):
        assert e[k] <= 4 * bounds[k], (k, e[k], 4 * bounds[k])
    return e


def life(torch, cons, reg, w, scene, monkeypatch, tmp_path=None, merged=False):
    """the phases for both reconstructions of a world, the checks after each -> what the byte-identity test goes on from"""
    prm = parameters()
    d_kps, d_counts, d_poses = pools(torch, w)
    waits = Waits(torch, monkeypatch, cons, reg.cons)
    kept = {}
    for name, triple, frames, view_range in (("A", L.A_START, L.A_GROW, L.A_VIEWS), ("B", L.B_START, L.B_GROW, L.B_VIEWS)):
        waits.take()
        r = start(torch, cons, w, prm, d_kps, d_poses, triple, view_range[0])
        assert waits.take() == ["rs_sync"]
        st = started_state(r, d_poses, view_range)
        hold(scene, "start", w, st, view_range)
        table = r.filter.table(torch)
        out, added, result, d_mask = grow(torch, reg, w, prm, d_kps, d_counts, d_poses, table, r.world, r.filter.split_out, r.filter.counts[1:2],
                                          st.rows, frames, triple, view_range)
        assert waits.take() == ["rs_sync"]
        refined = [t.cpu().numpy().copy() for t in (out.pose, out.verdict, out.final, out.n_final, out.stats, reg.noriginals)]   # (the next batch reuses them)
        g = grown_state(out, added, result, d_mask, d_poses, st.rows)
        hold(scene, "grow", w, g, view_range)
        kept[name] = (r, st, refined, added, result, g)
    if merged:
        merge_and_export(torch, cons, reg, w, scene, prm, waits, d_kps, d_counts, d_poses, kept, tmp_path)
    return prm, (d_kps, d_counts, d_poses), kept


def normalized(torch, cons, w, prm, d_kps, d_poses, g, result, view_range):
    """normalize_reconstruction for one side and the world table of its filtered rows under the new poses, one wait: the
    documented step in front of a merge of two reconstructions that were bootstrapped on their own"""
    from cv_amd import triangulation
    from cv_amd.reconstruction_merge import ReconstructionMerge
    table = result.filter.table(torch)
    n = ReconstructionMerge(cons).normalize_tensors(torch, list(range(*view_range)), w.counts, L.map_of(g.rows), L.CAP, result.world, d_poses)
    world, reason = table.new_world(), torch.zeros((table.n_landmarks,), dtype=torch.uint8, device=d_poses.device)
    triangulation.triangulate_landmarks_device(cons._h, table, d_kps, L.CAP, L.N_VIEWS, d_poses, cons.camera(L.CAM6), prm["flt"].triangulate, world, reason)
    cons.sync()
    assert u32(n.verdict).tolist() == [0]
    return table, world


def merge_and_export(torch, cons, reg, w, scene, prm, waits, d_kps, d_counts, d_poses, kept, tmp_path):
    """phases 3 and 4: both sides normalised, the bridging frame registered in B (with regenerate over [6, 13)) and in A
    (add_views alone), merge_reconstructions with the frame's pose taken from B, export_reconstruction and the file read back"""
    from cv_amd import _lib
    from cv_amd.export import read_ply
    from cv_amd.reconstruction import export_reconstruction, merge_reconstructions, stopped_at
    waits.take()
    side = {}
    for name, view_range in (("A", L.A_VIEWS), ("B", L.B_VIEWS)):
        _, _, _, _, result, g = kept[name]
        side[name] = normalized(torch, cons, w, prm, d_kps, d_poses, g, result, view_range) + (result, g)
        assert waits.take() == ["rs_sync"]
    table, world, result, g = side["B"]
    out, added_b, result_b, d_mask = grow(torch, reg, w, prm, d_kps, d_counts, d_poses, table, world, result.filter.split_out, result.filter.counts[1:2],
                                          g.rows, [L.BRIDGE], list(range(*L.B_VIEWS)), L.B_WITH_BRIDGE)
    assert waits.take() == ["rs_sync"]
    b = grown_state(out, added_b, result_b, d_mask, d_poses, g.rows)
    hold(scene, "bridge", w, b, L.B_WITH_BRIDGE)
    src_pose = b.poses[L.BRIDGE].copy()                              # the frame's pose in B, before A's add_views writes the block's row
    table, world, result, g = side["A"]
    out, added_a, _, d_mask = grow(torch, reg, w, prm, d_kps, d_counts, d_poses, table, world, result.filter.split_out, result.filter.counts[1:2],
                                   g.rows, [L.BRIDGE], list(range(*L.A_VIEWS)), L.A_VIEWS, regenerated=False)
    assert waits.take() == ["rs_sync"]
    assert u32(out.verdict)[:1].tolist() == [_lib.RS_SV_OK] and u32(added_a.frame_verdict).tolist() == [0] and not d_mask.cpu().numpy().any()
    merge_map, merged, _, mres = merge_reconstructions(
        torch, cons, added_a.table(torch), added_b.table(torch), d_kps, L.CAP, cons.camera(L.CAM6), d_poses, L.A_VIEWS, L.B_WITH_BRIDGE, L.BRIDGE, src_pose, 0,
        reg.originals, reg.noriginals, reg.refined.final, d_counts, added_b.landmarks_out, best=reg.best, n_world=table.n_landmarks,
        cv_params=prm["cv"], tvc_params=prm["tvc"], pg_params=prm["pg"], params=prm["flt"])
    assert waits.take() == ["rs_sync"]
    assert u32(merged.call_verdict).tolist() == [0] and stopped_at(u32(mres.verdict)[0]) is None, (u32(merged.call_verdict), stopped_at(u32(mres.verdict)[0]))
    n_rows = int(u32(merged.counts_out)[0])
    rows = L.rows_of(u32(mres.filter.obs_start_out), u32(mres.filter.obs_out).reshape(-1, 2), n_rows)
    m = L.SimpleNamespace(poses=d_poses.cpu().numpy().copy(), rows=rows, world=mres.world.cpu().numpy()[:n_rows], reason=mres.world_reason.cpu().numpy()[:n_rows],
                          table_rows=L.rows_of(u32(merged.obs_start_out), u32(merged.obs_out).reshape(-1, 2), n_rows),
                          table_map=u32(merged.landmarks_out).reshape(L.N_VIEWS, L.CAP), views=sorted({v for r in rows for v, _ in r}), tombstones=[])
    e = hold(scene, "merge", w, m, L.MERGED_VIEWS)
    scale, (one, many, sharing) = abs(np.log(L.relative_scale(m, w))), L.shared_points_are_one_landmark(w, m)
    print(scene, w.seed, "merge: |ln relative scale| %.3e (bound %.3e); map entries applied %d;" % (scale, 4 * L.BOUNDS[scene]["merge"]["scale"], int(u32(merged.counts_out)[2])),
          "shared points in one row %d, in several %d, rows of one point sharing a view %d" % (one, many, sharing))
    assert scale <= 4 * L.BOUNDS[scene]["merge"]["scale"]
    assert sharing == 0 and one >= L.SHARED_MERGED_AT_LEAST[scene]
    # phase 4
    path = tmp_path / "life.ply"
    res = export_reconstruction(torch, cons, mres.filter.table(torch), mres.world, w.colours, list(range(L.N_VIEWS)), w.counts, merged.landmarks_out, L.CAP,
                                d_poses, path)
    assert waits.take() == ["rs_sync"] and res.verdict == 0
    xyz, rgb, faces, _ = read_ply(path)
    x = L.exported_errors(w, m, xyz, rgb, res.key, e["similarity"])
    bounds = L.BOUNDS[scene]["export"]
    print(scene, w.seed, "export:", {k: "%.3e (bound %.3e)" % (x[k], 4 * bounds[k]) for k in ("centre", "point")}, "points", len(res.key), "wrong colours", x["wrong_colours"])
    assert len(xyz) == 5 * L.N_VIEWS + len(res.key) and len(res.key) == int((m.world[:, 3] > 0).sum()) and len(faces) == 4 * L.N_VIEWS
    assert x["wrong_colours"] == 0 and x["centre"] <= 4 * bounds["centre"] and x["point"] <= 4 * bounds["point"]


@pytest.mark.parametrize("seed", L.SEEDS["exact"])
def test_the_exact_world_from_the_first_pair_to_the_file(gpu, cons, reg, monkeypatch, tmp_path, seed):
    life(gpu, cons, reg, L.world(seed, 0.0, 0.0), "exact", monkeypatch, tmp_path, merged=True)


@pytest.mark.parametrize("seed", L.SEEDS["noisy"])
def test_the_noisy_world_from_the_first_pair_to_the_file(gpu, cons, reg, monkeypatch, tmp_path, seed):
    life(gpu, cons, reg, L.world(seed, 0.5, 0.1), "noisy", monkeypatch, tmp_path, merged=True)


def test_growing_from_the_bytes_of_the_start_equals_the_chained_run(gpu, cons, reg, monkeypatch):
    """phase 2 again from the BYTES phase 1 left — copied to the host and up again into fresh tensors, the table through a fresh
    LandmarkTable.from_device — gives every output byte of the chained run: a difference would be a stale or unordered read in
    the chain, not a wrong result"""
    from cv_amd.triangulation import LandmarkTable
    torch = gpu
    w = L.world(L.SEEDS["noisy"][0], 0.5, 0.1)
    prm, (d_kps, d_counts, d_chained), kept = life(torch, cons, reg, w, "noisy", monkeypatch)
    monkeypatch.undo()
    r, st, want_refined, added, result, _ = kept["A"]
    dev = d_kps.device
    fresh = lambda t: torch.from_numpy(t.cpu().numpy().copy()).to(dev)
    flt = r.filter
    table = LandmarkTable.from_device(torch, fresh(flt.obs_start_out), fresh(flt.obs_out), flt.n_landmarks, flt.n_obs)
    d_poses = torch.from_numpy(st.poses.copy()).to(dev)
    out2, added2, result2, _ = grow(torch, reg, w, prm, fresh(d_kps), fresh(d_counts), d_poses, table, fresh(r.world), fresh(flt.split_out),
                                    fresh(flt.counts)[1:2], st.rows, L.A_GROW, L.A_START, L.A_VIEWS)
    same = lambda a, b, what: np.array_equal(a.cpu().numpy().view(np.uint8), b.cpu().numpy().view(np.uint8)) or pytest.fail(what)
    n = want_refined[5].view(np.uint32)
    for k, t in enumerate((out2.pose, out2.verdict, out2.final, out2.n_final, out2.stats, reg.noriginals)):
        got, want = t.cpu().numpy(), want_refined[k]
        if k == 2:                                                    # d_final is written for a frame's matches: the rest is the caller's
            assert all(np.array_equal(got[f, :n[f]], want[f, :n[f]]) for f in range(3)), "final"
        else:
            assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), ("refined", k)
    for name in ("obs_start_out", "obs_out", "counts_out", "landmarks_out", "obs_counts_out", "frame_verdict", "stats", "call_verdict"):
        same(getattr(added2, name), getattr(added, name), name)
    for name in ("keep", "lm_state", "tri_reason", "robust", "obs_start_out", "obs_out", "split_out", "counts", "recon_verdict", "stats"):
        same(getattr(result2.filter, name), getattr(result.filter, name), "filter." + name)
    same(result2.world, result.world, "world")
    same(result2.world_reason, result.world_reason, "world_reason")
    same(result2.recorded, result.recorded, "recorded")
    same(d_poses[:6], d_chained[:6], "poses")                        # (the chained run went on to B: rows 6 and up are B's)
