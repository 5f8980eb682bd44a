"""The repack kernels (cv_amd/csrc/rs_repack.hip) against the host build of the same header (tests/cpp/repack_host.c through
tests/repack_catalogue.py): every output buffer is compared in bytes, WHOLE — both sides start from the same fill pattern, so a
word a call should have written and did not shows, and so does one it should have left alone.  The catalogue is the CPU tests'
(tests/test_repack_math.py holds the host build to the statement on it).  Then the repacked reconstruction is put through
the stages that read it — triangulation, export, relaxation, merge_reconstructions, place recognition — next to the one it came from.
Run with -m gpu.

Shapes: T = RS_LT_TILE rows are one workgroup's tile of the scans (256 threads x 4 rows); a row of more than 64 observations
is walked by its wave; the tile sums are scanned 256 at a time by one workgroup, and so are the constraints compacted; the gather
takes 16-byte words where the row length and both pointers allow and 4-byte words elsewhere, four a lane and trip, on a grid of at
most 256 x 65 535 workgroups."""
import numpy as np
import pytest

import repack_catalogue as cat
import triangulate_checker as T

pytestmark = pytest.mark.gpu

CASES = cat.table_cases()
BY_NAME = {c.name: c for c in CASES}


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


def uploader(torch):
    from cv_amd import _lib
    dev = torch.device("cuda", 0)
    return lambda a: None if a is None else _lib.device_bytes(torch, a, dev)


def back(d, want):
    return {k: d[k].cpu().numpy().view(want[k].dtype).reshape(want[k].shape) for k in want}


def device_table(torch, cons, case):
    """rs_repack_table_device on the arrays of a case -> dict of the output buffers as the host checker shapes them"""
    from cv_amd import _lib
    from cv_amd.repack import TableRepack
    up = uploader(torch)
    want = cat.blank(case)
    d = {k: up(v) for k, v in want.items()}                            # the host's fill, byte for byte
    d_start, d_obs, d_map, d_recon = up(case.start), up(np.ascontiguousarray(case.obs)), up(case.map), up(case.recon_start)
    TableRepack(cons).table_device(d_start, d_obs, case.n_obs, case.n_landmarks, case.cap, case.n_blocks, d_map, case.n_blocks_out, d_recon,
                                   0 if case.recon_start is None else len(case.recon_start) - 1, case.obs_room, case.lm_room, d["obs_start_out"],
                                   d["obs_out"], d["obs_counts_out"], d["landmarks_out"], d["key_out"], d.get("recon_start_out"), d["counts_out"],
                                   d["call_verdict"], stream_to_wait=_lib.wait_handle(torch.cuda.current_stream(torch.device("cuda", 0))))
    cons.sync()
    return back(d, want)


def explain(got, want):
    k = cat.same(got, want)
    if k is None:
        return None
    g, w = got[k].reshape(-1), want[k].reshape(-1)
    bad = np.flatnonzero(g != w)
    return k, len(bad), bad[:10], g[bad[:10]], w[bad[:10]]


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_table_device_is_the_host_build_in_every_byte(gpu, cons, case):
    want = cat.host_table(case)
    assert int(want["call_verdict"][0]) == case.expect
    assert explain(device_table(gpu, cons, case), want) is None


def test_table_calls_back_to_back_share_the_scratch(gpu, cons):
    """a large call, a refused one and a small one on one context: what one leaves in the scratch is nothing to the next"""
    for name in ("rows_2049", "b9_shared_target", "b5_first_removed", "drop_whole_tile", "block_is_n_blocks", "rows_1"):
        assert explain(device_table(gpu, cons, BY_NAME[name]), cat.host_table(BY_NAME[name])) is None, name


@pytest.mark.parametrize("case", cat.tile_sums_cases(), ids=repr)
def test_table_rows_beyond_one_pass_of_the_tile_sums(gpu, cons, case):
    """cv_amd/csrc/rs_repack.hip:149, k_rp_scan_sums: `for (t0 = 0; t0 < n_tiles; t0 += kRpBlock)` with kRpBlock = 256 tile sums
    a trip behind a running carry.  256 x 1024 rows are 256 tiles, the last size of one trip; 256 x 1024 + 1 and + 3 rows give
    a 257th tile and the second trip, whose offsets are the carry of the first.  One observation a row, rows removed sparsely
    (every tile and every trip keeps a sum that is not zero) and on both sides of row 256 x 1024.  Every output byte against the
    host build and against the answer numpy gives directly (tests/test_repack_math.py ties the two to the statement)."""
    edge = cat.SUMS_PASS * cat.TILE
    assert cat.TILE == 1024 and case.n_landmarks in (edge, edge + 1, edge + 3)
    assert (case.n_landmarks + cat.TILE - 1) // cat.TILE == (cat.SUMS_PASS if case.n_landmarks == edge else cat.SUMS_PASS + 1)
    want = cat.host_table(case)
    assert int(want["call_verdict"][0]) == cat.OK and cat.same(want, cat.direct_table(case)) is None
    assert int(want["counts_out"][0]) == case.n_landmarks - len(case.doomed) and len(case.doomed) > 250
    assert explain(device_table(gpu, cons, case), want) is None


# ---- the pools ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offsets", [(0, 0), (4, 0), (0, 4), (4, 4)], ids=lambda o: "src+%d_dst+%d" % o)
@pytest.mark.parametrize("row_bytes", cat.GATHER_ROW_BYTES)
def test_gather_device_is_the_host_build_in_every_byte(gpu, cons, row_bytes, offsets):
    from cv_amd import _lib
    from cv_amd.repack import TableRepack
    torch = gpu
    dev = torch.device("cuda", 0)
    rp = TableRepack(cons)
    held = []
    for name, nb, block_map, out, expect in cat.gather_cases():
        src = cat.pool(nb, row_bytes)
        want, want_verdict = cat.host_gather(src, row_bytes, nb, block_map, out)
        assert int(want_verdict[0]) == expect
        # 16 bytes of fill on either side of dst: nothing is written outside it
        d_src = torch.zeros(src.size + 32, dtype=torch.uint8, device=dev)
        d_dst = torch.full((want.size + 48,), 0xA5, dtype=torch.uint8, device=dev)
        so, do = 16 + offsets[0], 16 + offsets[1]
        d_src[so:so + src.size] = torch.from_numpy(src.reshape(-1)).to(dev)
        d_verdict = torch.full((1,), -1, dtype=torch.int32, device=dev)
        d_map = None if block_map is None else _lib.device_bytes(torch, np.array(block_map, np.uint32), dev)
        rp.gather_device(d_src.data_ptr() + so, d_dst.data_ptr() + do, row_bytes, nb, d_map, out, d_verdict,
                         stream_to_wait=_lib.wait_handle(torch.cuda.current_stream(dev)))
        held.append((d_src, d_dst, d_verdict, d_map, want, do, out, name, expect))
    cons.sync()
    for d_src, d_dst, d_verdict, d_map, want, do, out, name, expect in held:
        got = d_dst.cpu().numpy()
        n = out * row_bytes
        assert np.array_equal(got[do:do + n], want.reshape(-1)[:n]), name
        assert np.all(got[:do] == 0xA5) and np.all(got[do + n:] == 0xA5), name
        assert int(d_verdict.cpu().numpy().view(np.uint32)[0]) == expect, name


def gather_once(torch, cons, src, row_bytes, nb, block_map, out, offsets):
    """one rs_gather_blocks_device call between 16-byte bands of 0xA5 -> (dst rows [out][row_bytes], the verdict); the bands
    are asserted untouched"""
    from cv_amd import _lib
    from cv_amd.repack import TableRepack
    dev = torch.device("cuda", 0)
    n = out * row_bytes
    d_src = torch.zeros(src.size + 32, dtype=torch.uint8, device=dev)
    d_dst = torch.full((n + 48,), 0xA5, dtype=torch.uint8, device=dev)
    so, do = 16 + offsets[0], 16 + offsets[1]
    d_src[so:so + src.size] = torch.from_numpy(src.reshape(-1)).to(dev)
    d_verdict = torch.full((1,), -1, dtype=torch.int32, device=dev)
    d_map = None if block_map is None else _lib.device_bytes(torch, np.asarray(block_map, np.uint32), dev)
    TableRepack(cons).gather_device(d_src.data_ptr() + so, d_dst.data_ptr() + do, row_bytes, nb, d_map, out, d_verdict,
                                    stream_to_wait=_lib.wait_handle(torch.cuda.current_stream(dev)))
    cons.sync()
    got = d_dst.cpu().numpy()
    assert np.all(got[:do] == 0xA5) and np.all(got[do + n:] == 0xA5)
    return got[do:do + n].reshape(out, row_bytes), int(d_verdict.cpu().numpy().view(np.uint32)[0])


def first_difference(got, want):
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    return None if len(bad) == 0 else (len(bad), bad[:8], got.reshape(-1)[bad[:8]], want.reshape(-1)[bad[:8]])


@pytest.mark.parametrize("row_bytes,offsets,nb", cat.GATHER_LONG_ROWS, ids=lambda v: str(v).replace(" ", ""))
def test_gather_rows_across_the_unroll_the_grid_and_its_cap(gpu, cons, row_bytes, offsets, nb):
    """cv_amd/csrc/rs_repack.hip:282-293, k_rp_gather: a workgroup of kRpBlock = 256 lanes takes kUnroll = 4 units a lane and
    trip, unit u0 + k * 256 in slot k, so a row of at most 256 units uses slot 0 alone, 257 .. 1024 the slots above it with a
    partial tail, and beyond 1024 units a second workgroup (rs_repack.hip:452, gx = ceil(units / 1024)); gx is capped at 256
    (rs_repack.hip:453), so a row of 256 x 1024 + 1 units sends workgroup 0 on a second trip of the inner loop.  Units are 16
    bytes where the row length and both pointers allow and 4 bytes elsewhere.  229 376 bytes is the workload's own row (cap 8192
    x 28 bytes: 14 336 units, gx = 14).  The map removes one view and permutes the rest."""
    wide = row_bytes % 16 == 0 and offsets == (0, 0)
    units = row_bytes // (16 if wide else 4)
    assert (row_bytes, wide) in {(16 * u, True) for u in (255, 256, 257, 1023, 1024, 1025, 14336, 262145)} | {(4 * u, False) for u in (257, 1025, 262145)}
    assert units in (255, 256, 257, 1023, 1024, 1025, 14336, 262145)
    gone = nb // 2
    order = [b for b in range(nb) if b != gone]
    block_map = np.full(nb, cat.NONE, np.uint32)
    block_map[order] = np.roll(np.arange(nb - 1)[::-1], 1)                         # reversed and turned by one
    src = cat.pool(nb, row_bytes)
    want = cat.direct_gather(src, block_map, nb - 1)
    if row_bytes <= 16 * 1025:
        host, verdict = cat.host_gather(src, row_bytes, nb, [int(m) for m in block_map], nb - 1)
        assert int(verdict[0]) == cat.OK and np.array_equal(host, want)
    got, verdict = gather_once(gpu, cons, src, row_bytes, nb, block_map, nb - 1, offsets)
    assert verdict == cat.OK and first_difference(got, want) is None


@pytest.mark.parametrize("out,mapped", [(65534, True), (65535, True), (65536, True), (65536, False)],
                         ids=lambda v: str(v))
def test_gather_row_counts_across_the_cap_of_the_grids_second_dimension(gpu, cons, out, mapped):
    """cv_amd/csrc/rs_repack.hip:453 launches min(n_blocks_out, 65535) workgroups in y and rs_repack.hip:278 strides over the rows
    with gridDim.y: at 65536 rows workgroup 0 takes a second row, row 65535.  Rows of 16 bytes; with a map (one view removed, the
    rest reversed) and, at 65536, with the null map of the identity, where n_blocks_out == n_blocks."""
    nb = out + 1 if mapped else out
    block_map = None
    if mapped:
        block_map = np.full(nb, cat.NONE, np.uint32)
        block_map[[b for b in range(nb) if b != 7]] = np.arange(out, dtype=np.uint32)[::-1]
    src = cat.pool(nb, 16)
    want = cat.direct_gather(src, block_map, out)
    host, verdict = cat.host_gather(src, 16, nb, None if block_map is None else [int(m) for m in block_map], out)
    assert int(verdict[0]) == cat.OK and np.array_equal(host, want)
    got, verdict = gather_once(gpu, cons, src, 16, nb, block_map, out, (0, 0))
    assert verdict == cat.OK and first_difference(got, want) is None
    assert np.array_equal(got[out - 1], src[0 if mapped else out - 1])              # the last row is one of the source's


# ---- the constraints -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 513])
def test_constraints_device_is_the_host_build_in_every_byte(gpu, cons, n):
    """cv_amd/csrc/rs_repack.hip:308, k_rp_constraints: ONE workgroup compacts kRpBlock = 256 constraints a trip behind a
    running carry.  0, 1, 255 and 256 constraints are one trip, 257 two, 513 three: the third starts from a carry that was
    itself added to a carry."""
    from cv_amd import _lib
    from cv_amd.repack import TableRepack
    torch = gpu
    dev = torch.device("cuda", 0)
    up = uploader(torch)
    nb = 9
    views, poses, verdict = cat.constraint_case(n, nb)
    runs = []
    for gone in ((), (0,), (4,), (8,), (1, 7), tuple(range(nb))):
        block_map, out = cat.compact(nb, set(gone))
        for start in (None, [0, n // 3, n // 3, n, n + 5]):
            want = cat.host_constraints(views, poses, verdict, block_map, nb, out, start)
            fill = dict(views_out=np.full_like(want["views_out"], cat.POISON), poses_out=np.full_like(want["poses_out"], -7.0),
                        verdict_out=np.full_like(want["verdict_out"], cat.POISON), count=np.full(1, cat.POISON, np.uint32))
            if start is not None:
                fill["start_out"] = np.full(len(start), cat.POISON, np.uint32)
            d = {k: up(v) for k, v in fill.items()}
            ins = [up(views), up(poses), up(verdict), up(np.array(block_map, np.uint32)), up(None if start is None else np.array(start, np.uint32))]
            TableRepack(cons).constraints_device(ins[0], ins[1], ins[2], n, ins[3], nb, out, ins[4], 0 if start is None else len(start) - 1,
                                                 d["views_out"], d["poses_out"], d["verdict_out"], d["count"], d.get("start_out"),
                                                 stream_to_wait=_lib.wait_handle(torch.cuda.current_stream(dev)))
            runs.append((gone, start, d, ins, want))
    cons.sync()
    for gone, start, d, ins, want in runs:
        got = back(d, want)
        for k in want:
            assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), (gone, start, k)


def test_constraints_identity_map_is_null(gpu, cons):
    from cv_amd.repack import TableRepack
    views, poses, verdict = cat.constraint_case(300)
    v, p, c, s = TableRepack(cons).run_constraints(gpu, views, poses, verdict, None, 9, 9, start=[0, 100, 300])
    assert np.array_equal(v, views) and np.array_equal(p, poses) and np.array_equal(c, verdict) and list(s) == [0, 100, 300]


# ---- the stages behind ---------------------------------------------------------------------------------------------------------
N_BLOCKS, CAP_MAP = 12, 256


@pytest.fixture(scope="module")
def scene(gpu, cons):
    """A synthetic map of 12 views with tombstones and an empty tail, repacked with two views removed and the rest reversed;
    the pools moved along."""
    from cv_amd import _lib
    from cv_amd.repack import TableRepack, to_host
    from cv_amd.triangulation import LandmarkTable
    torch = gpu
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(20)
    kps, poses, start, obs, _ = T.synthetic_map(rng, N_BLOCKS, CAP_MAP, 1500, max_len=6)
    lens = np.diff(start.astype(np.int64))
    lens = np.concatenate([lens, np.zeros(500, np.int64)])                       # the empty tail of a generation that never waited
    start = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    gone = {3, 7}
    keep = [b for b in range(N_BLOCKS) if b not in gone]
    block_map = np.full(N_BLOCKS, cat.NONE, np.uint32)
    block_map[keep] = np.arange(len(keep))[::-1]
    n_out = len(keep)
    table = LandmarkTable(torch, start=start, obs=obs)
    rp = TableRepack(cons)
    d_kps = _lib.device_bytes(torch, kps, dev).view(torch.uint8).reshape(N_BLOCKS, CAP_MAP * 28)
    d_poses = torch.from_numpy(poses).to(dev)
    t = rp.table_tensors(torch, table, CAP_MAP, N_BLOCKS, block_map, n_out, fill=-1)
    new_kps, v0 = rp.gather_tensors(torch, d_kps, block_map, n_out)
    new_poses, v1 = rp.gather_tensors(torch, d_poses, block_map, n_out)
    cons.sync()
    res = to_host(t)
    assert res.call_verdict == 0 and int(v0.cpu()[0]) == 0 and int(v1.cpu()[0]) == 0
    return dict(kps=kps, poses=poses, start=start, obs=obs, block_map=block_map, n_out=n_out, table=table, d_kps=d_kps, d_poses=d_poses,
                t=t, res=res, new_kps=new_kps, new_poses=new_poses, gone=gone)


def camera():
    from cv_amd import _lib
    return _lib.Camera(1000.0, 1000.0, 960.0, 540.0, 0.0, 0.0, 0, 0)


def triangulate(torch, cons, table, d_kps, n_blocks, d_poses):
    from cv_amd import triangulation
    world = table.new_world()
    reason = torch.full((max(table.n_landmarks, 1),), 0xEE, dtype=torch.uint8, device=table.dev)
    triangulation.triangulate_landmarks_device(cons._h, table, d_kps, CAP_MAP, n_blocks, d_poses, camera(), triangulation.make_params(), world, reason,
                                               torch.cuda.current_stream(table.dev))
    cons.sync()
    return world.cpu().numpy(), reason.cpu().numpy()


def test_the_repacked_table_triangulates_to_the_same_bits(gpu, cons, scene):
    """Old table with the removed views' observations taken out on the host (the statement's table, old keys and blocks) and the
    repacked table with renumbered pools: d_world and d_reason equal bit for bit through d_key_out."""
    from cv_amd.triangulation import LandmarkTable
    s = scene
    keep = s["block_map"][s["obs"][:, 0]] != cat.NONE
    lens = np.array([int(keep[a:b].sum()) for a, b in zip(s["start"][:-1], s["start"][1:])], np.int64)
    old = LandmarkTable(gpu, start=np.concatenate([[0], np.cumsum(lens)]), obs=s["obs"][keep])
    w_old, r_old = triangulate(gpu, cons, old, s["d_kps"], N_BLOCKS, s["d_poses"])
    # without counts: lm_room rows, the rows behind the kept ones empty
    w_new, r_new = triangulate(gpu, cons, s["t"].table(gpu), s["new_kps"], s["n_out"], s["new_poses"])
    keys = s["res"].keys
    kept = np.flatnonzero(keys != cat.NONE)
    assert len(kept) == int(s["res"].counts[0]) == int(np.count_nonzero(lens)) and 0 < len(kept) < len(lens)
    assert np.array_equal(keys[kept], np.arange(len(kept)))                       # ascending order is preserved
    assert np.array_equal(w_new[keys[kept]].view(np.uint64), w_old[kept].view(np.uint64))
    assert np.array_equal(r_new[keys[kept]], r_old[kept])
    assert len({int(r) for r in r_old[kept]}) >= 2                                 # points and refusals both
    assert np.all(r_new[len(kept):s["t"].lm_room] == 1)                           # RS_TRI_TOO_FEW behind the kept rows
    # with the counts read back: the same bytes on the kept rows
    w_cut, r_cut = triangulate(gpu, cons, s["t"].table(gpu, s["res"].counts), s["new_kps"], s["n_out"], s["new_poses"])
    assert np.array_equal(w_cut.view(np.uint64), w_new[:len(kept)].view(np.uint64)) and np.array_equal(r_cut, r_new[:len(kept)])


def test_frames_follow_the_map_and_a_removed_views_frame_is_free(gpu, cons, scene):
    """FrameIndex.remap_views == the host build; then hm_find_frames_batch_device: the removed view's frame is in d_free, the
    others' views are the mapped ones."""
    from cv_amd import _lib, place_recognition
    from cv_amd.knn import Matcher
    torch = gpu
    m = Matcher(max_descriptors=256)
    try:
        n = N_BLOCKS + 2
        idx = place_recognition.FrameIndex(torch, m, n, hash_bytes=16)
        rng = np.random.default_rng(5)
        idx.append_rows(np.zeros(n, np.uint32), np.arange(n, dtype=np.uint32), rng.integers(0, 256, (n, 16)).astype(np.uint8))
        recon = np.array([0] * N_BLOCKS + [1, 0], np.uint32)
        view = np.array(list(range(N_BLOCKS)) + [3, N_BLOCKS], np.uint32)          # another reconstruction's view 3; a view outside
        idx.set_views(np.arange(n), recon, view)
        flags = idx.remap_views(0, scene["block_map"])
        prm = place_recognition.params(num_recent=n, num_similar=0)
        found = idx.find(np.array([0], np.uint32), prm)
        _lib.check(_lib.lib().hm_sync(m.handle), "hm_sync")
        want_recon, want_view, want_flags = cat.host_frames(recon, view, 0, scene["block_map"], N_BLOCKS)
        assert int(flags.cpu()[0]) == 1 == int(want_flags[0])
        assert np.array_equal(idx.recon.cpu().numpy().view(np.uint32), want_recon) and np.array_equal(idx.view.cpu().numpy().view(np.uint32), want_view)
        counts = found.counts.cpu().numpy()[0]
        free = set(found.free.cpu().numpy()[0][:counts[_lib.HM_PL_C_FREE]].tolist())
        assert free == set(scene["gone"])                                          # rows 3 and 7 held the removed views
        views_out = found.views_out.cpu().numpy()[0][:counts[_lib.HM_PL_C_RECENT] - counts[_lib.HM_PL_C_FREE]].view(np.uint32)
        assert set(scene["block_map"][[b for b in range(1, N_BLOCKS) if b not in scene["gone"]]].tolist()) <= set(views_out.tolist())
    finally:
        m.close()


def trimmed_old(scene):
    """the old table with the removed views' observations taken out on the host: old keys, old blocks -> (start, obs)"""
    keep = scene["block_map"][scene["obs"][:, 0]] != cat.NONE
    lens = np.array([int(keep[a:b].sum()) for a, b in zip(scene["start"][:-1], scene["start"][1:])], np.int64)
    return np.concatenate([[0], np.cumsum(lens)]), scene["obs"][keep]


def test_the_repacked_reconstruction_exports_the_same_vertices(gpu, cons, scene):
    """Old and new through rs_export_reconstruction_device: the vertex arrays are byte-equal — cameras and points, ascending order
    preserved —, the key column mapped through d_key_out."""
    from cv_amd.export import ReconstructionExport
    from cv_amd.repack import TableRepack
    from cv_amd.triangulation import LandmarkTable
    torch = gpu
    s = scene
    dev = s["d_poses"].device
    start, obs = trimmed_old(s)
    old = LandmarkTable(torch, start=start, obs=obs)
    w_old, _ = triangulate(torch, cons, old, s["d_kps"], N_BLOCKS, s["d_poses"])
    new = s["t"].table(torch)
    w_new, _ = triangulate(torch, cons, new, s["new_kps"], s["n_out"], s["new_poses"])
    colors = ((np.arange(N_BLOCKS * CAP_MAP * 3, dtype=np.uint32) * 2654435761 >> 11) & 0xFF).astype(np.uint8).reshape(N_BLOCKS, CAP_MAP, 3)
    counts = np.full(N_BLOCKS, CAP_MAP, np.uint32)
    lm_old = np.full((N_BLOCKS, CAP_MAP), cat.NONE, np.uint32)
    for key in range(len(start) - 1):
        for b, f in obs[start[key]:start[key + 1]]:
            lm_old[b, f] = key
    rp = TableRepack(cons)
    d_colors = torch.from_numpy(colors).to(dev)
    d_counts = torch.from_numpy(counts.view(np.int32).reshape(N_BLOCKS, 1)).to(dev)
    new_colors, _ = rp.gather_tensors(torch, d_colors, s["block_map"], s["n_out"])
    new_counts, _ = rp.gather_tensors(torch, d_counts, s["block_map"], s["n_out"])
    views_old = [b for b in range(N_BLOCKS) if b not in s["gone"]]
    views_new = [int(s["block_map"][b]) for b in views_old]
    ex = ReconstructionExport(cons)
    a = ex.run_export(torch, old, w_old, d_colors, views_old, counts, lm_old, CAP_MAP, s["d_poses"])
    b = ex.run_export(torch, new, w_new, new_colors, views_new, new_counts.reshape(-1), s["t"].landmarks_out, CAP_MAP, s["new_poses"])
    assert a.verdict == b.verdict == 0 and list(a.counts[:1]) == list(b.counts[:1]) and int(a.counts[0]) > 100
    assert np.array_equal(a.xyz.view(np.uint64), b.xyz.view(np.uint64)) and np.array_equal(a.rgb, b.rgb)
    assert np.array_equal(a.cameras.view(np.uint64), b.cameras.view(np.uint64))
    assert np.array_equal(s["res"].keys[a.key], b.key) and np.all(np.diff(b.key.astype(np.int64)) > 0)


def test_the_relaxation_takes_the_room_for_the_count(gpu, cons, scene):
    """Relaxation over the repacked constraints: passing the room as n_constraints gives the same pose bits as passing the
    count; the rows are the count's, and rs_pose_graph_rows_device's flag word reads 1 for the triples behind it."""
    from cv_amd.pose_graph import PoseGraph
    from cv_amd.repack import TableRepack
    torch = gpu
    s = scene
    n = 60
    views, _, _ = cat.constraint_case(n, N_BLOCKS)
    P = np.concatenate([s["poses"].reshape(N_BLOCKS, 3, 4), np.tile([[[0.0, 0.0, 0.0, 1.0]]], (N_BLOCKS, 1, 1))], 1)
    rel = lambda i, j, k: (P[j] @ np.linalg.inv(P[i]) @ np.diag([1.0, 1.0, 1.0, 1.0 + 1e-3 * k]))[:3].reshape(12)
    poses = np.array([[rel(v[0], v[1], c % 5), rel(v[0], v[2], c % 3)] for c, v in enumerate(views)])
    verdict = np.array([1 if c % 11 == 5 else 0 for c in range(n)], np.uint32)
    o = TableRepack(cons).constraints_tensors(torch, views, poses, verdict, s["block_map"], N_BLOCKS, s["n_out"], fill=-1)
    cons.sync()
    k = int(o.count.cpu()[0])
    assert 3 < k < n
    pg = PoseGraph(cons)
    out = []
    for m in (k, n):
        d_views = o.views_out[:m].contiguous()
        edges = pg.edges(torch, d_views, (o.poses_out[:m].contiguous(), o.verdict_out[:m].contiguous()))
        rows = pg.rows(torch, d_views, s["n_out"])
        d_poses = s["new_poses"].clone()
        r = pg.relax(torch, d_poses, np.array([0, s["n_out"]], np.uint32), rows[0], rows[1], edges, pg.params(optimization_iterations=8))
        out.append((d_poses.cpu().numpy().view(np.uint64), rows[0].cpu().numpy(), rows[1].cpu().numpy(), int(rows[2].cpu()[0]), r))
    (p_k, rs_k, re_k, flag_k, r_k), (p_n, rs_n, re_n, flag_n, r_n) = out
    assert flag_k == 0 and flag_n == 1
    assert np.array_equal(rs_k, rs_n) and np.array_equal(re_k[:rs_k[-1]], re_n[:rs_n[-1]]) and np.all(re_n[rs_n[-1]:] == 0)
    assert list(r_k.verdicts) == list(r_n.verdicts) == [0] and np.array_equal(r_k.view_states, r_n.view_states)
    assert np.array_equal(p_k, p_n) and not np.array_equal(p_k, s["new_poses"].cpu().numpy().view(np.uint64))



def test_merge_after_renumbering_equals_the_merge_built_adjacent(gpu, cons):
    """Two designed reconstructions on view ranges that are NOT adjacent in the block pool — the destination on blocks [0, 6) with
    the bridging frame in 6, the source on 6 and [11, 16) — are repacked adjacent (tables, pools, the source's per-feature map);
    merge_reconstructions then equals, in bytes, the merge of the same rows built adjacent from the start: the map, the merged
    table, the poses, the world table and the regenerated one."""
    from test_gpu_landmark_table import rs_camera
    from test_gpu_reconstruction_merge import two_reconstructions
    from cv_amd import _lib
    from cv_amd.covisibility import Covisibility
    from cv_amd.reconstruction import ObservationFilter, merge_reconstructions
    from cv_amd.repack import TableRepack, to_host
    from cv_amd.triangulation import LandmarkTable
    torch = gpu
    dev = torch.device("cuda", 0)
    two = two_reconstructions()
    sc, cap, n_views, half, bridge = two["sc"], two["cap"], two["n_views"], two["half"], two["bridge"]
    gap, n_far = 4, n_views + 4
    far = lambda b: b if b <= bridge else b + gap                                 # where a view lies in the scattered pool
    block_map = np.full(n_far, cat.NONE, np.uint32)
    for b in range(n_views):
        block_map[far(b)] = b
    scatter = lambda a: np.concatenate([a[:bridge + 1], np.zeros((gap,) + a.shape[1:], a.dtype), a[bridge + 1:]])
    rp = TableRepack(cons)
    cam, prm = rs_camera(sc["cam"]), ObservationFilter.params(minimum_robust_landmarks=8)
    cv = Covisibility.params(optimization_robust_covisibility_minimum_landmarks=4, optimization_minimum_landmarks=4)
    src_pose = sc["poses"][bridge].copy()
    # ---- the scattered reconstructions, repacked adjacent
    repacked = []
    for rows in (two["dst_rows"], two["src_rows"]):
        t = rp.table_tensors(torch, LandmarkTable(torch, lists=[[(far(b), f) for b, f in r] for r in rows]), cap, n_far, block_map, n_views, fill=-1)
        cons.sync()
        r = to_host(t)
        assert r.call_verdict == 0 and np.array_equal(r.keys, np.arange(len(rows))) and int(r.counts[0]) == len(rows)
        repacked.append((t, t.table(torch, r.counts)))
    pools = {}
    for name, a in (("kps", sc["kps"].view(np.uint8).reshape(n_views, -1)), ("poses", sc["poses"].reshape(n_views, 12)),
                    ("counts", two["counts"].view(np.int32).reshape(n_views, 1))):
        pools[name], v = rp.gather_tensors(torch, torch.from_numpy(scatter(np.ascontiguousarray(a))).to(dev), block_map, n_views)
        cons.sync()
        assert int(v.cpu()[0]) == 0 and np.array_equal(pools[name].cpu().numpy(), a), name
    src_landmarks = repacked[1][0].landmarks_out                                  # the source's per-feature map under the new blocks
    assert np.array_equal(src_landmarks.cpu().numpy().view(np.uint32)[:n_views], two["src_landmarks"])
    # ---- the merge of each
    outs = []
    for which in (0, 1):
        if which == 0:
            dst, src = LandmarkTable(torch, lists=two["dst_rows"]), LandmarkTable(torch, lists=two["src_rows"])
            d_poses, d_kps = torch.from_numpy(sc["poses"].copy()).to(dev), _lib.device_bytes(torch, sc["kps"].view(np.uint8), dev)
            counts, lm = two["counts"], two["src_landmarks"]
        else:
            dst, src = repacked[0][1], repacked[1][1]
            d_poses, d_kps, counts, lm = pools["poses"].clone(), pools["kps"], pools["counts"].reshape(-1), src_landmarks
        merge_map, merged, (world, reason), result = merge_reconstructions(
            torch, cons, dst, src, d_kps, cap, cam, d_poses, (0, half), (half, n_views), bridge, src_pose, 0, two["matches"], two["nmatches"],
            two["final"], counts, lm, params=prm, cv_params=cv)
        u = lambda x: x.cpu().numpy().view(np.uint32)
        outs.append(dict(map=u(merge_map.map), map_count=u(merge_map.map_count), start=u(merged.obs_start_out), counts=u(merged.counts_out),
                         obs=u(merged.obs_out)[:int(u(merged.counts_out)[1])], landmarks=u(merged.landmarks_out), src_key=u(merged.src_key_out),
                         obs_counts=u(merged.obs_counts_out), verdict=u(merged.call_verdict), poses=d_poses.cpu().numpy().view(np.uint64),
                         world=world.cpu().numpy().view(np.uint64), reason=reason.cpu().numpy(),
                         regenerated=result.world.cpu().numpy().view(np.uint64), regenerated_reason=result.world_reason.cpu().numpy(),
                         or_verdict=u(result.verdict)))
    a, b = outs
    assert int(a["verdict"][0]) == 0 and int(a["map_count"][0]) == two["n_matches"] > 50 and int(a["counts"][2]) == two["n_matches"]
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert (a["reason"] == _lib.TRI_OK).sum() > 100


def test_the_native_mirror_gives_the_same_table_and_pool(gpu, cons, tmp_path):
    """cv_sfm::TableRepack of include/akaze.hpp from a process without Python (tests/cpp/repack.cpp): the printed words of a
    catalogue case and of a gathered pool equal the host build's"""
    import subprocess

    import host_build
    for name, row_words in (("rows_1025", 12), ("b9_below_removed", 3), ("b9_shared_target", 4), ("b5_identity_null", 1)):
        case = BY_NAME[name]
        assert case.recon_start is None
        want = cat.host_table(case)
        pool = cat.pool(case.n_blocks, 4 * row_words)
        moved, pool_verdict = cat.host_gather(pool, 4 * row_words, case.n_blocks, None if case.map is None else case.list_map(), case.n_blocks_out)
        path = tmp_path / (name + ".bin")
        with open(path, "wb") as fp:
            fp.write(np.array([case.n_blocks, case.cap, case.n_landmarks, case.n_obs, case.n_blocks_out, int(case.map is not None), case.lm_room,
                               case.obs_room, row_words], np.uint32).tobytes())
            for arr in (case.start, case.obs[:case.n_obs], np.array(case.list_map(), np.uint32), pool):
                fp.write(np.ascontiguousarray(arr).tobytes())
        exe = host_build.native(tmp_path, "repack.cpp", hip=True)
        r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (name, r.returncode, r.stderr[-400:])
        out = {line.split(" ", 1)[0]: np.array(line.split()[1:], np.int64) for line in r.stdout.splitlines()}
        assert out["verdict"].tolist() == [case.expect] and np.array_equal(out["counts"], want["counts_out"]), name
        assert np.array_equal(out["obs_start_out"], want["obs_start_out"]) and np.array_equal(out["obs_out"], want["obs_out"][:case.obs_room].reshape(-1)), name
        assert np.array_equal(out["obs_counts_out"], want["obs_counts_out"][:case.lm_room]), name
        assert np.array_equal(out["landmarks_out"], want["landmarks_out"][:case.n_blocks_out].reshape(-1)), name
        assert np.array_equal(out["key_out"], want["key_out"][:case.n_landmarks]), name
        assert out["pool_verdict"].tolist() == [int(pool_verdict[0])], name
        assert np.array_equal(out["pool_out"], moved[:case.n_blocks_out].view(np.uint32).reshape(-1)), name
