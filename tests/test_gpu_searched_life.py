"""A reconstruction's life on the device with the matcher in the loop (tests/searched_life_statement.py): descriptors, keypoints
and counts are uploaded once; hm_match_batch_device makes the bootstrap's pair lists where reconstruction.start_reconstructions
reads them; each side grows in two calls of Registration.match_views -> sharing_view -> triangulate_merged -> consensus(d_merge_ok,
d_obs_counts) -> refine -> landmark_table.add_views_and_regenerate, every one reading the landmarks_out / obs_counts_out TENSORS the
call before wrote; the bridging frame is registered by search on both sides, then merge and export as in
test_gpu_reconstruction_life.py.  Each chain has the one wait it documents.  After every call the tensors are copied out and held
  - byte for byte to the matcher's statement on the device's OWN inputs (best / decision over the device's landmarks_out, the hash,
    the share mask over the device's table, the match lists over the device's world table and obs_counts_out, the pair lists), and
  - to the ground truth: the table invariants, aligned_errors within four times BOUNDS — measured from the chain of statements on
    the CPU, not from the device — and, in the exact worlds, conditions(): every decision-1 match names a landmark of the feature's
    own point, every applied merge joins two landmarks of one point and leaves one of them alive.
The statement chain is not run here.  Run with -m gpu."""
import numpy as np
import pytest

import landmark_table_statement as LT
import matching_statement as M
import reconstruction_life_statement as L
import searched_life_statement as S
import test_gpu_reconstruction_life as G

pytestmark = pytest.mark.gpu
u32 = G.u32
CODEWORDS = np.random.default_rng(1).integers(0, 256, (32, 64), dtype=np.uint8)


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
    p = L.SETTINGS["p3p"]
    r = Registration(gpu, L.CAP, 3, 6, CODEWORDS, L.CAM6, threshold=p["threshold"], n_hypotheses=p["n_hypotheses"], max_candidates=p["max_candidates"],
                     estimations_per_block=p["estimations_per_block"], block_size=p["block_size"], better_by=S.BETTER_BY, seed=p["seed"])
    yield r
    r.close()


def start(torch, cons, reg, w, prm, d_kps, d_descs, d_counts, d_poses, triple, view_base):
    """phase 1: the two pair lists of the triple by the symmetric better-by match on the matcher's stream, start_reconstructions
    behind that stream -> (StartResult, d_pairs, d_npairs)"""
    from cv_amd import _device, knn
    from cv_amd.reconstruction import start_reconstructions
    dev = d_kps.device
    c, f, s = triple
    d_pairs, d_npairs = torch.zeros((2, L.CAP, 2), dtype=torch.int32, device=dev), torch.zeros((2,), dtype=torch.int32, device=dev)
    d_kps_dst, d_counts_dst = d_kps.clone(), d_counts.clone()
    a = dict(L.SETTINGS["arrsac"])
    arrsac = cons.make_params(a.pop("threshold"), **a)
    torch.cuda.current_stream(dev).synchronize()                      # the allocations above; the chain below waits once
    ia, _ = _device.index_list([c, c])
    ib, _ = _device.index_list([f, s])
    _device.call("hm_match_batch_device", reg.matcher.handle, d_descs, d_counts, d_descs, d_counts, L.CAP, ia, ib, 2, knn.RULE_BETTER_BY,
                 S.BETTER_BY, 0.0, 1, d_pairs, d_npairs, None)
    with torch.cuda.stream(reg._hm_s):                                # start_reconstructions orders itself behind the current torch stream
        r = start_reconstructions(torch, cons, d_kps, w.counts, L.CAP, cons.camera(L.CAM6), d_pairs, d_npairs, [c, c], [f, s], arrsac, [(0, 1)], [c], [f],
                                  [s], L.N_VIEWS, view_base, d_kps_dst=d_kps_dst, d_counts_dst=d_counts_dst, d_poses=d_poses,
                                  minimum=L.SETTINGS["join_minimum"], seed=L.SETTINGS["join_seed"], tv_params=prm["tv"], pg_params=prm["pg"],
                                  params=prm["flt"])
    return r, d_pairs, d_npairs


def grow(torch, reg, w, prm, d_kps, d_descs, d_counts, d_poses, table, d_world, d_split, d_split_count, d_landmarks, d_obs_counts, frames, stored,
         graph, regenerated=True):
    """one call: the frames' search against the stored views over d_landmarks, the share test, the merge candidates' rows, the
    consensus in the order of d_obs_counts, the refinement and add_views_and_regenerate over the graph's blocks; no tensor
    visits the host and nothing is waited for before the chain's own wait -> SimpleNamespace of what the checks read"""
    from cv_amd.landmark_table import add_views_and_regenerate
    dev = d_kps.device
    F, n_world = len(frames), table.n_landmarks
    none = torch.zeros((F * L.CAP, 4), dtype=torch.float64, device=dev)
    none[:, 3] = -1.0
    world = torch.cat([d_world[:n_world], none])                      # room for the merge candidates' rows
    torch.cuda.current_stream(dev).synchronize()                      # (that copy; the chain below waits once)
    reg.match_views(d_descs, d_counts, list(frames), [list(stored)] * F, d_landmarks)
    d_mask = reg.sharing_view(table)
    reg.triangulate_merged(table, d_kps, d_poses, d_mask, world, n_world)
    reg.consensus(d_kps, d_counts, world, n_world, d_merge_ok=d_mask, stream_to_wait=reg.rs_stream(), d_obs_counts=d_obs_counts)
    out = reg.refine(d_poses, table.d_start, table.d_obs, n_world, params=prm["sv"], stream=torch.cuda.current_stream(dev))
    if regenerated:
        added, result = add_views_and_regenerate(torch, reg, table, d_kps, d_poses, np.array(graph, np.uint32), d_split, d_split_count,
                                                 targets=np.arange(*graph, dtype=np.uint32), cv_params=prm["cv"], tvc_params=prm["tvc"],
                                                 pg_params=prm["pg"], params=prm["flt"])
    else:                                                             # add_views alone: the destination's side of a bridging frame
        added, result = reg.add_views(table, d_poses, d_split, d_split_count), None
        reg.sync()
    return L.SimpleNamespace(out=out, added=added, result=result, d_mask=d_mask, world=world, table=table, n_world=n_world, frames=list(frames),
                             stored=list(stored), d_landmarks=d_landmarks, d_obs_counts=d_obs_counts)


def bytes_of_the_call(reg, w, g):
    """the matcher's statement on the DEVICE'S inputs of the call, byte for byte -> the call as conditions() reads it"""
    F, n_world = len(g.frames), g.n_world
    landmarks = u32(g.d_landmarks).reshape(L.N_VIEWS, L.CAP)
    best, decision = u32(reg.best)[:F], u32(reg.decision)[:F]
    want_best, want_decision = S.searched_tables(w, g.frames, g.stored, landmarks)
    live = np.arange(L.CAP)[None, :] < w.counts[g.frames][:, None]   # what lies behind a frame's count is nobody's
    assert np.array_equal(decision[live], want_decision[live]), "decision"
    assert np.array_equal(best[live], want_best[live]), "best"
    hashes = reg.hash.cpu().numpy()
    for frame in g.frames:
        assert np.array_equal(hashes[frame - reg.hash_block0], M.hash_bag(w.descs[frame, :w.counts[frame]], CODEWORDS)[0]), ("hash", frame)
    rows = L.rows_of(u32(g.table.d_start)[:n_world + 1], u32(g.table.d_obs).reshape(-1, 2))
    mask = g.d_mask.cpu().numpy()[:F]
    assert np.array_equal(mask[live] != 0, np.array(LT.sharing_mask(rows, best, decision, n_world), np.uint8)[live] != 0), "merge_ok"
    world, obs_counts = g.world.cpu().numpy(), u32(g.d_obs_counts)
    pairs, npairs = u32(reg.pairs)[:F], u32(reg.npairs)[:F]
    originals, noriginals = u32(reg.originals)[:F].copy(), u32(reg.noriginals)[:F].copy()
    for f in range(F):
        n = int(w.counts[g.frames[f]])                                # (the tables behind a frame's count are an earlier call's)
        want = M.landmark_pairs(best[f, :n], decision[f, :n], mask[f, :n], world, n_world, n_world + f * L.CAP, obs_counts)
        assert npairs[f] == len(want) and np.array_equal(pairs[f, :npairs[f]], want), ("pairs", f, int(npairs[f]), len(want))
        want = M.landmark_pairs(best[f, :n], decision[f, :n], mask[f, :n], None, n_world, n_world + f * L.CAP, obs_counts)
        assert noriginals[f] == len(want) and np.array_equal(originals[f, :noriginals[f]], want), ("originals", f)
    n_rows = int(u32(g.added.counts_out)[0])
    return L.SimpleNamespace(frames=g.frames, rows_before=rows, best=best.copy(), decision=decision.copy(), mask=mask, pairs=[pairs[f, :npairs[f]].copy() for f in range(F)], matches=originals,
                             nmatches=noriginals, final=g.out.final.cpu().numpy()[:F].copy(), verdict=u32(g.out.verdict)[:F].copy(),
                             rows_after=L.rows_of(u32(g.added.obs_start_out), u32(g.added.obs_out).reshape(-1, 2), max(n_rows, n_world)))


def grown_state(g, d_poses):
    from cv_amd import _lib
    from cv_amd.reconstruction import stopped_at
    out, added, result = g.out, g.added, g.result
    assert u32(out.verdict)[:added.n_frames].tolist() == [_lib.RS_SV_OK] * added.n_frames, u32(out.verdict).tolist()
    assert u32(added.frame_verdict).tolist() == [0] * added.n_frames and u32(added.call_verdict).tolist() == [0]
    assert stopped_at(u32(result.verdict)[0]) is None, stopped_at(u32(result.verdict)[0])
    n_rows = int(u32(added.counts_out)[0])
    kept, split = (int(v) for v in u32(result.filter.counts)[:2])
    table_rows = L.rows_of(u32(added.obs_start_out), u32(added.obs_out).reshape(-1, 2), n_rows)
    rows = L.rows_of(u32(result.filter.obs_start_out), u32(result.filter.obs_out).reshape(-1, 2), n_rows)
    old = L.rows_of(u32(g.table.d_start)[:g.n_world + 1], u32(g.table.d_obs).reshape(-1, 2))
    assert sum(len(x) for x in rows) == kept and all(not r for r in L.rows_of(u32(added.obs_start_out), u32(added.obs_out).reshape(-1, 2))[n_rows:])
    return L.SimpleNamespace(poses=d_poses.cpu().numpy().copy(), rows=rows, world=result.world.cpu().numpy()[:n_rows],
                             reason=result.world_reason.cpu().numpy()[:n_rows], table_rows=table_rows,
                             table_map=u32(added.landmarks_out).reshape(L.N_VIEWS, L.CAP), views=sorted({b for r in rows for b, _ in r}),
                             tombstones=[l for l in range(min(len(old), n_rows)) if old[l] and not table_rows[l]],
                             split=u32(result.filter.split_out).reshape(-1, 2)[:split])


def hold(scene, phase, w, st, view_range):
    """the invariants and aligned_errors against the searched BOUNDS; every figure is printed before it is asserted"""
    broken = L.invariants(st.table_rows, view_range, st.table_map, st.tombstones) + L.invariants(st.rows, view_range, tombstones=st.tombstones)
    e = L.aligned_errors(st.poses, st.world, st.reason, L.truth_of(w, st.rows, st.views))
    bounds = S.BOUNDS[scene][phase]
    print(scene, w.seed, phase, view_range, {k: "%.3e (bound %.3e)" % (e[k], 4 * bounds[k]) for k in ("rotation", "centre", "point")},
          "left out %.3f" % e["left_out"], "scale %.4f" % e["similarity"][0], "broken", broken[:3])
    assert broken == []
    assert len(st.views) == S.VIEWS_AFTER[phase], st.views                       # no view may be left out
    assert e["left_out"] <= L.LEFT_OUT_CAP[scene], e["left_out"]
    for k in ("rotation", "centre", "point"):
        assert e[k] <= 4 * bounds[k], (k, e[k], 4 * bounds[k])
    return e


def held_conditions(scene, w, phase, call):
    c = S.conditions(w, call)
    print(scene, w.seed, phase, "frames", call.frames, {k: (v if isinstance(v, int) else len(v)) for k, v in c.items()})
    assert c["stray_mask"] == []
    if scene == "exact":
        assert all(not c[k] for k in S.MUST_BE_EMPTY), c
    return c


def life(torch, cons, reg, w, scene, monkeypatch, tmp_path):
    from cv_amd import _lib
    from cv_amd.export import read_ply
    from cv_amd.reconstruction import export_reconstruction, merge_reconstructions, stopped_at
    prm = G.parameters()
    d_kps, d_counts, d_poses = G.pools(torch, w)
    d_descs = torch.from_numpy(w.descs).to(d_kps.device)
    waits = G.Waits(torch, monkeypatch, cons, reg.cons)
    side = {}
    for name, triple, frames, view_range in (("A", L.A_START, L.A_GROW, L.A_VIEWS), ("B", L.B_START, L.B_GROW, L.B_VIEWS)):
        lo = view_range[0]
        waits.take()
        r, d_pairs, d_npairs = start(torch, cons, reg, w, prm, d_kps, d_descs, d_counts, d_poses, triple, lo)
        assert waits.take() == ["rs_sync"]
        pairs, npairs = u32(d_pairs), u32(d_npairs)
        want_pairs, want_n = S.searched_pair_lists(w, triple)
        assert np.array_equal(npairs, want_n) and all(np.array_equal(pairs[k, :npairs[k]], want_pairs[k, :npairs[k]]) for k in range(2)), "pair lists"
        wrong, missing = S.wrong_pairs(w, triple, pairs, npairs)
        print(scene, w.seed, name, "pair lists", npairs.tolist(), "wrong", wrong, "missing", missing)
        assert scene != "exact" or (wrong, missing) == (0, 0)
        st = G.started_state(r, d_poses, view_range)
        hold(scene, "start", w, st, view_range)
        # call 1: one frame against the start views, over the map and counts add_reconstruction wrote
        g1 = grow(torch, reg, w, prm, d_kps, d_descs, d_counts, d_poses, r.filter.table(torch), r.world, r.filter.split_out, r.filter.counts[1:2],
                  r.start.landmarks_out, r.start.obs_counts_out, frames[:1], triple, (lo, lo + 4))
        assert waits.take() == ["rs_sync"]
        c1 = held_conditions(scene, w, name + " grow1", bytes_of_the_call(reg, w, g1))
        hold(scene, "grow1", w, grown_state(g1, d_poses), (lo, lo + 4))
        # call 2: two frames against four views, the one just added among them, over the map and counts call 1 wrote
        res = g1.result
        g2 = grow(torch, reg, w, prm, d_kps, d_descs, d_counts, d_poses, res.filter.table(torch), res.world, res.filter.split_out,
                  res.filter.counts[1:2], g1.added.landmarks_out, g1.added.obs_counts_out, frames[1:], list(triple) + list(frames[:1]), view_range)
        assert waits.take() == ["rs_sync"]
        c2 = held_conditions(scene, w, name + " grow", bytes_of_the_call(reg, w, g2))
        grown = grown_state(g2, d_poses)
        hold(scene, "grow", w, grown, view_range)
        side[name] = (g2, grown, c1, c2)
    # both sides normalised, the bridging frame registered by search in B (regenerated over [6, 13)) and in A (add_views alone)
    norm = {}
    waits.take()
    for name, view_range in (("A", L.A_VIEWS), ("B", L.B_VIEWS)):
        g2, grown = side[name][:2]
        norm[name] = G.normalized(torch, cons, w, prm, d_kps, d_poses, grown, g2.result, view_range)
        assert waits.take() == ["rs_sync"]
    (g2, grown), (table, world) = side["B"][:2], norm["B"]
    gb = grow(torch, reg, w, prm, d_kps, d_descs, d_counts, d_poses, table, world, g2.result.filter.split_out, g2.result.filter.counts[1:2],
              g2.added.landmarks_out, g2.added.obs_counts_out, [L.BRIDGE], list(range(*L.B_VIEWS)), L.B_WITH_BRIDGE)
    assert waits.take() == ["rs_sync"]
    bridged = {"B": held_conditions(scene, w, "bridge in B", bytes_of_the_call(reg, w, gb))}
    b = grown_state(gb, d_poses)
    hold(scene, "bridge", w, b, L.B_WITH_BRIDGE)
    src_pose = b.poses[L.BRIDGE].copy()                              # the frame's pose in B, before A's add_views writes the block's row
    (g2, grown), (table, world) = side["A"][:2], norm["A"]
    ga = grow(torch, reg, w, prm, d_kps, d_descs, d_counts, d_poses, table, world, g2.result.filter.split_out, g2.result.filter.counts[1:2],
              g2.added.landmarks_out, g2.added.obs_counts_out, [L.BRIDGE], list(range(*L.A_VIEWS)), L.A_VIEWS, regenerated=False)
    assert waits.take() == ["rs_sync"]
    bridged["A"] = held_conditions(scene, w, "bridge in A", bytes_of_the_call(reg, w, ga))
    if scene == "exact":        # on both sides: the mask non-empty, merges applied and demoted, merged rows with a point in the consensus
        assert [S.exact_side(*side[name][2:], bridged[name]) for name in "AB"] == [[], []]
    assert u32(ga.out.verdict)[:1].tolist() == [_lib.RS_SV_OK] and u32(ga.added.frame_verdict).tolist() == [0]
    merge_map, merged, _, mres = merge_reconstructions(
        torch, cons, ga.added.table(torch), gb.added.table(torch), d_kps, L.CAP, cons.camera(L.CAM6), d_poses, L.A_VIEWS, L.B_WITH_BRIDGE, L.BRIDGE, src_pose,
        0, reg.originals, reg.noriginals, reg.refined.final, d_counts, gb.added.landmarks_out, best=reg.best, n_world=table.n_landmarks,
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
    print(scene, w.seed, "merge: |ln relative scale| %.3e (bound %.3e); map entries applied %d;" % (scale, 4 * S.BOUNDS[scene]["merge"]["scale"], int(u32(merged.counts_out)[2])),
          "shared points in one row %d, in several %d, rows of one point sharing a view %d" % (one, many, sharing))
    assert scale <= 4 * S.BOUNDS[scene]["merge"]["scale"]
    assert sharing == 0 and one >= L.SHARED_MERGED_AT_LEAST[scene]
    path = tmp_path / "life.ply"
    res = export_reconstruction(torch, cons, mres.filter.table(torch), mres.world, w.colours, list(range(L.N_VIEWS)), w.counts, merged.landmarks_out, L.CAP,
                                d_poses, path)
    assert waits.take() == ["rs_sync"] and res.verdict == 0
    xyz, rgb, faces, _ = read_ply(path)
    x = L.exported_errors(w, m, xyz, rgb, res.key, e["similarity"])
    bounds = S.BOUNDS[scene]["export"]
    print(scene, w.seed, "export:", {k: "%.3e (bound %.3e)" % (x[k], 4 * bounds[k]) for k in ("centre", "point")}, "points", len(res.key), "wrong colours", x["wrong_colours"])
    assert len(xyz) == 5 * L.N_VIEWS + len(res.key) and len(res.key) == int((m.world[:, 3] > 0).sum()) and len(faces) == 4 * L.N_VIEWS
    assert x["wrong_colours"] == 0 and x["centre"] <= 4 * bounds["centre"] and x["point"] <= 4 * bounds["point"]


@pytest.mark.parametrize("seed", S.SEEDS["exact"])
def test_the_exact_world_searched_from_the_first_pair_to_the_file(gpu, cons, reg, monkeypatch, tmp_path, seed):
    life(gpu, cons, reg, S.searched_world(seed, *S.SCENES["exact"]), "exact", monkeypatch, tmp_path)


@pytest.mark.parametrize("seed", S.SEEDS["noisy"])
def test_the_noisy_world_searched_from_the_first_pair_to_the_file(gpu, cons, reg, monkeypatch, tmp_path, seed):
    life(gpu, cons, reg, S.searched_world(seed, *S.SCENES["noisy"]), "noisy", monkeypatch, tmp_path)
