"""A chain that never waits, bounded by a repack: add_views twice on a designed map without reading a count back (so that the
rooms are the table's sizes and every refused slot costs cap_per_img empty rows), then cv_amd.reconstruction.repack with one view
removed, then the next add_views from the repacked table — next to the same call from the table a host would have trimmed,
with that view's observations removed by the statement (tests/repack_statement.py).  The two next generations hold the same rows
in the same order, the same per-feature map and the same world bits, through the key map.  Run with -m gpu.

The map is designed, not the life statement's smallest scene (that one needs a matcher, a consensus and a refinement in front of
every add_views); the calls are add_views_and_regenerate's own: rs_add_views_device on designed slots, then
cv_amd.reconstruction.regenerate with the rooms as the table's sizes.  The repack itself continues into regenerate
(graph_start), and so does the host-trimmed side."""
import numpy as np
import pytest

import repack_catalogue as cat
import repack_statement as stmt
import observation_filter_checker as F

pytestmark = pytest.mark.gpu

CAP, N_BLOCKS, GONE = 352, 7, 1
SV_OK, SV_REFUSED = 0, 2


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
    c = EssentialConsensus(64, 64)
    yield c
    c.close()


def slot_arrays(slots):
    """(blocks, matches [F][cap][2], nmatches [F], final [F][cap], verdict [F], pose_out [F][12]) of a call's slots"""
    F = len(slots)
    matches, final = np.zeros((F, CAP, 2), np.uint32), np.zeros((F, CAP), np.uint8)
    nmatches, verdict, pose_out = np.zeros(F, np.uint32), np.zeros(F, np.uint32), np.zeros((F, 12))
    for f, (block, ms, v, pose) in enumerate(slots):
        matches[f, :len(ms)] = np.array(ms, np.uint32).reshape(-1, 2)
        final[f, :len(ms)] = 1
        nmatches[f], verdict[f], pose_out[f] = len(ms), v, pose
    return [s[0] for s in slots], matches, nmatches, final, verdict, pose_out


def rows_of(start, obs, n):
    return [[tuple(int(v) for v in o) for o in obs[int(start[r]):int(start[r + 1])]] for r in range(n)]


def test_a_chain_that_never_waits_is_bounded_by_a_repack(gpu, cons):
    from cv_amd import _lib, reconstruction
    from cv_amd._device import host_u32 as u32
    from cv_amd.landmark_table import LandmarkUpdate
    from cv_amd.covisibility import Covisibility
    from cv_amd.reconstruction import ObservationFilter, regenerate
    from cv_amd.triangulation import LandmarkTable
    torch = gpu
    dev = torch.device("cuda", 0)
    sc = F.scene(7, n_views=N_BLOCKS, n_landmarks=400, lengths=(4, 7), outlier_fraction=0.0)      # every landmark in 4 to 7 of the 7 views
    cam = _lib.Camera(sc["cam"].fx, sc["cam"].fy, sc["cam"].cx, sc["cam"].cy, sc["cam"].skew, sc["cam"].k1, sc["cam"].use_k1, 0)
    start, obs, poses = sc["start"], sc["obs"], sc["poses"]
    assert int(obs[:, 1].max()) < CAP
    kps = np.ascontiguousarray(sc["kps"][:, :CAP])
    lists = rows_of(start, obs, len(start) - 1)                              # the whole map; views 4, 5 and 6 arrive later
    counts = np.array([1 + max([f for l in lists for b, f in l if b == blk], default=-1) for blk in range(N_BLOCKS)], np.uint32)
    first = [[o for o in l if o[0] < 4] for l in lists]
    n0 = len(first)
    table = LandmarkTable(torch, lists=first)
    d_kps = _lib.device_bytes(torch, kps, dev).view(torch.uint8).reshape(N_BLOCKS, CAP * 28)
    d_poses = torch.zeros((N_BLOCKS, 12), dtype=torch.float64, device=dev)
    d_poses[:4] = torch.from_numpy(poses[:4]).to(dev)
    d_counts = torch.from_numpy(counts.view(np.int32)).to(dev)
    up = LandmarkUpdate(cons)

    def matches_of(block, row_of):
        """the frame's observations of landmarks that have a row -> (feature, row); the others, and every fourth landmark (as if
        the matcher had missed it), become new rows"""
        return [(f, row_of[l]) for l, lst in enumerate(lists) for b, f in lst if b == block and l % 4 and row_of.get(l) is not None]

    # ---- two generations, no count read back: a refused slot costs cap empty rows each time
    row_of = {l: l for l, lst in enumerate(first) if lst}
    s1 = slot_arrays([(4, matches_of(4, row_of), SV_OK, poses[4]), (5, [], SV_REFUSED, poses[5]), (6, [], SV_REFUSED, poses[6])])
    g1 = up.add_views_tensors(torch, table, d_poses, CAP, s1[0], d_counts, *s1[1:])
    t1 = g1.table(torch)                                                       # lm_room rows: the rooms are the sizes
    s2 = slot_arrays([(5, matches_of(5, row_of), SV_OK, poses[5]), (6, [], SV_REFUSED, poses[6])])
    g2 = up.add_views_tensors(torch, t1, d_poses, CAP, s2[0], d_counts, *s2[1:])
    t2 = g2.table(torch)
    assert t2.n_landmarks == n0 + 5 * CAP and t2.n_obs == len(obs[obs[:, 0] < 4]) + 5 * CAP

    # ---- the repack: view GONE removed, the rest closed up; rooms n_blocks_out * cap, whatever the chain grew to
    block_map, n_out = cat.compact(N_BLOCKS, {GONE})
    block_map = np.array(block_map, np.uint32)
    prm = ObservationFilter.params(minimum_robust_landmarks=8)
    cv = Covisibility.params(optimization_robust_covisibility_minimum_landmarks=4, optimization_minimum_landmarks=4)
    graph = np.array([0, n_out], np.uint32)
    unrelaxed = d_poses.cpu().numpy().copy()
    rep = reconstruction.repack(torch, cons, t2, CAP, cam, block_map, n_out, dict(kps=d_kps, poses=d_poses, counts=d_counts.reshape(N_BLOCKS, 1)),
                                graph_start=graph, params=prm, cv_params=cv)
    assert np.array_equal(d_poses.cpu().numpy(), unrelaxed)                   # out of place: the old generation is as it was
    assert rep.table.lm_room == n_out * CAP < t2.n_landmarks and rep.table.obs_room == n_out * CAP < t2.n_obs
    assert int(u32(rep.table.call_verdict)[0]) == _lib.RS_RP_OK and all(int(u32(v)[0]) == _lib.RS_RP_OK for v in rep.pool_verdicts.values())
    assert int(u32(g1.call_verdict)[0]) == 0 and int(u32(g2.call_verdict)[0]) == 0
    assert list(u32(g1.frame_verdict)) == [0, 1, 1] and list(u32(g2.frame_verdict)) == [0, 1]

    # ---- the table a host would have trimmed, the view's observations removed by the statement
    start2, obs2, lm2 = u32(g2.obs_start_out), u32(g2.obs_out).reshape(-1, 2), u32(g2.landmarks_out).reshape(N_BLOCKS, CAP)
    s = stmt.repack(start2, obs2, t2.n_landmarks, N_BLOCKS, CAP, [int(m) for m in block_map], [GONE])
    keys = u32(rep.table.key_out)
    assert [int(k) for k in keys] == [s["key_of"].get(r, cat.NONE) for r in range(t2.n_landmarks)]
    rows3 = int(u32(rep.table.counts_out)[0])
    assert rows_of(u32(rep.table.obs_start_out), u32(rep.table.obs_out).reshape(-1, 2), rows3) == s["rows"]
    kept = [b for b in range(N_BLOCKS) if b != GONE]
    trimmed = LandmarkTable(torch, lists=s["rows"])
    h_poses = torch.from_numpy(unrelaxed[kept]).to(dev)
    h_counts = torch.from_numpy(counts[kept].view(np.int32)).to(dev)
    h_kps = _lib.device_bytes(torch, kps[kept], dev)
    # regenerate behind the repack, rooms as sizes, next to regenerate on the trimmed table: the same verdicts, poses, filtered rows, world
    held_r = regenerate(torch, cons, trimmed, h_kps, CAP, cam, h_poses, graph, np.array([0, rows3], np.uint32), params=prm, cv_params=cv)
    chain_r = rep.regenerate
    assert list(u32(chain_r.verdict)) == list(u32(held_r.verdict)) == [_lib.RS_OR_OK]
    assert np.array_equal(rep.pools["poses"].cpu().numpy().view(np.uint64), h_poses.cpu().numpy().view(np.uint64))
    assert not np.array_equal(h_poses.cpu().numpy(), unrelaxed[kept])         # the relaxation moved them
    assert np.array_equal(u32(chain_r.filter.obs_start_out)[:rows3 + 1], u32(held_r.filter.obs_start_out))
    n_f = int(u32(held_r.filter.obs_start_out)[rows3])
    assert np.array_equal(u32(chain_r.filter.obs_out).reshape(-1, 2)[:n_f], u32(held_r.filter.obs_out).reshape(-1, 2)[:n_f])
    assert np.array_equal(chain_r.world.cpu().numpy()[:rows3].view(np.uint64), held_r.world.cpu().numpy()[:rows3].view(np.uint64))
    assert np.array_equal(chain_r.world_reason.cpu().numpy()[:rows3], held_r.world_reason.cpu().numpy()[:rows3])
    assert np.all(chain_r.world_reason.cpu().numpy()[rows3:n_out * CAP] == _lib.TRI_TOO_FEW)
    assert np.array_equal(rep.pools["kps"].cpu().numpy().reshape(-1), kps[kept].view(np.uint8).reshape(-1))
    assert np.array_equal(u32(rep.pools["counts"]).reshape(-1), counts[kept])

    # ---- the next generation from both: view 6 arrives, its matches named by the new keys
    def row_in_t2(l):
        seen = [int(lm2[b, f]) for b, f in lists[l] if b < 6 and b != GONE and lm2[b, f] != cat.NONE]
        return seen[0] if seen else None
    new_key = {l: s["key_of"].get(row_in_t2(l)) for l in range(len(lists))}
    s3 = slot_arrays([(int(block_map[6]), matches_of(6, new_key), SV_OK, poses[6])])
    assert 0 < s3[2][0] < counts[6]                                          # matches and new rows both

    def next_generation(tbl, d_p, d_c, d_k):
        g = up.add_views_tensors(torch, tbl, d_p, CAP, s3[0], d_c, *s3[1:])
        t = g.table(torch)
        r = regenerate(torch, cons, t, d_k, CAP, cam, d_p, graph, np.array([0, t.n_landmarks], np.uint32), params=prm, cv_params=cv)
        world, reason = r.world, r.world_reason
        st, ob = u32(g.obs_start_out), u32(g.obs_out).reshape(-1, 2)
        full = [r for r in range(t.n_landmarks) if st[r + 1] > st[r]]        # the rows that hold something, in order
        rank = {r: k for k, r in enumerate(full)}
        lm = u32(g.landmarks_out).reshape(n_out, CAP)
        return dict(rows=[rows_of(st, ob, t.n_landmarks)[r] for r in full], lens=[int(u32(g.obs_counts_out)[r]) for r in full],
                    landmarks=[[rank.get(int(v), cat.NONE) for v in row] for row in lm], world=world.cpu().numpy()[full].view(np.uint64),
                    reason=reason.cpu().numpy()[full], verdict=list(u32(g.frame_verdict)), regenerated=list(u32(r.verdict)), counts=[int(v) for v in u32(g.counts_out)[1:]],
                    poses=d_p.cpu().numpy().view(np.uint64), n_rows=t.n_landmarks)

    chained = next_generation(rep.table.table(torch), rep.pools["poses"], rep.pools["counts"].reshape(-1), rep.pools["kps"])
    held = next_generation(trimmed, h_poses, h_counts, h_kps)
    assert chained["verdict"] == held["verdict"] == [0]
    assert chained["n_rows"] == n_out * CAP + CAP and held["n_rows"] == rows3 + CAP          # bounded, and the host's exact size
    assert chained["regenerated"] == [_lib.RS_OR_OK]
    for k in ("rows", "lens", "landmarks", "reason", "counts", "regenerated"):
        assert chained[k] == held[k] if isinstance(held[k], list) else np.array_equal(chained[k], held[k]), k
    assert np.array_equal(chained["world"], held["world"]) and np.array_equal(chained["poses"], held["poses"])
    assert len(set(held["reason"].tolist())) >= 2 and 0 in held["reason"]    # points and refusals both
