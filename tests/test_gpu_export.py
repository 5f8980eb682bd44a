"""The export kernels (cv_amd/csrc/rs_export.hip) and the batched colour sampler (cv_amd/csrc/akz_color.hip) against the host
build of the same header (tests/export_checker.py): every output buffer is compared in bytes, WHOLE — both sides start from the
same fill pattern, so a word a call should have written and did not shows, and so does one it should have left alone.  On the
clean cases of tests/test_export_math.py the device's buffers are held to the independent statement
(tests/export_statement.py) as well, under that file's bound.  Run with -m gpu.

Shapes: T = RS_LT_TILE rows of the world table are one workgroup's tile of the scan (256 threads x 4 rows), the workgroup that
scans the tile sums takes 256 of them per pass; a view's features are summed by 256 threads of 4 waves, so 0, 1, 63, 64, 255,
256 and 257 counted features walk the sum order's boundaries."""
import numpy as np
import pytest

import export_checker as K
from test_export_math import BOUND, DESIGNED, RANDOM

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
    c = EssentialConsensus(64, 64)
    yield c
    c.close()


def tile():
    from cv_amd import _lib
    return _lib.RS_LT_TILE


def uploader(torch):
    from cv_amd import _lib
    dev = torch.device("cuda", 0)
    return lambda a: None if a is None else _lib.device_bytes(torch, a, dev)


def back(d, want, names):
    return {k: d[k].cpu().numpy().view(want[k].dtype).reshape(want[k].shape) for k in names}


INPUTS = ("world", "start", "obs", "colors", "counts", "landmarks", "poses")


def device_export(torch, cons, inp, d_in=None, over=None, before=None):
    """rs_export_reconstruction_device on the arrays of a call -> dict of the output buffers as the host checker shapes them.
    before: what to enqueue on the consensus' stream once every buffer is on the device; the export then follows it on that
    stream and names no stream to wait for."""
    from cv_amd import _lib
    from cv_amd.export import ReconstructionExport
    up = uploader(torch)
    d_in = dict({k: up(inp[k]) for k in INPUTS}, **(d_in or {}))
    want = K.outputs(inp)
    d = {k: up(want[k]) for k in K.OUTPUTS}                            # the host's fill, byte for byte
    a = dict(room=inp["room"], view_blocks=[int(b) for b in inp["view_blocks"]])
    a.update(over or {})
    if before is not None:
        before(d_in)
    ReconstructionExport(cons).export_device(
        d_in["world"], inp["n_world"], d_in["start"], d_in["obs"], inp["n_obs"], inp["n_landmarks"], d_in["colors"], a["view_blocks"], d_in["counts"],
        d_in["landmarks"], inp["cap"], inp["n_blocks"], d_in["poses"], a["room"], *(d[k] for k in K.OUTPUTS),
        stream_to_wait=None if before is not None else _lib.wait_handle(torch.cuda.current_stream(torch.device("cuda", 0))))
    cons.sync()
    return back(d, want, K.OUTPUTS)


def assert_same(got, want, names=K.OUTPUTS):
    for k in names:
        g, w = got[k].view(np.uint8).reshape(len(want[k]), -1), want[k].view(np.uint8).reshape(len(want[k]), -1)
        if not np.array_equal(g, w):
            bad = np.flatnonzero((g != w).any(1))
            raise AssertionError((k, len(bad), bad[:10], got[k][bad[:4]], want[k][bad[:4]]))


def check(torch, cons, inp, statement=False):
    """device == host build in every byte of every output buffer -> the host result"""
    want = K.export(inp)
    got = device_export(torch, cons, inp)
    assert_same(got, want)
    if statement:
        K.check_against_statement(inp, got, BOUND)
    return want


def raw_inputs(seed, n_world, n_views, keep_every=3, cap=8, room=None, world_pad=0):
    """A call over a large table made with numpy alone: every landmark has one observation; row l has a point iff l % keep_every
    == 1, else it is akz_tri_none, w == +-0, or (every 41st) a row whose first observation lies outside the colours"""
    rng = np.random.default_rng(seed)
    n_blocks = n_views + 2
    n_lm = n_world - world_pad
    l = np.arange(n_world)
    world = np.zeros((max(n_world, 1), 4))
    world[:, :3] = rng.uniform(-20.0, 20.0, (max(n_world, 1), 3))
    world[:, 3] = rng.uniform(0.5, 2.0, max(n_world, 1))
    rest = l % keep_every != 1
    world[:n_world][rest & (l % 2 == 0)] = K.NO_POINT
    world[:n_world, 3][rest & (l % 4 == 1)] = 0.0
    world[:n_world, 3][rest & (l % 4 == 3)] = -0.0
    obs = np.stack([rng.integers(0, n_blocks, n_lm), rng.integers(0, cap, n_lm)], 1).astype(np.uint32).reshape(-1, 2)
    obs[40::41, 0] = n_blocks + 3
    obs = np.concatenate([obs, np.full((2, 2), K.FILL32, np.uint32)])
    blocks = rng.permutation(n_blocks)[:n_views]
    counts = np.zeros(n_blocks, np.uint32)
    counts[blocks] = cap
    lm = rng.integers(0, max(n_world, 1) + 5, (n_blocks, cap)).astype(np.uint32)
    poses = np.stack([K.random_pose(rng) for _ in range(n_blocks)])
    inp = K.inputs(world[:n_world], None, blocks, counts, lm, poses, cap, room=room, seed=seed, start=np.arange(n_lm + 1), start_obs=obs)
    inp["n_obs"] = n_lm + 2
    return inp


@pytest.mark.parametrize("n_views", [1, 3])
@pytest.mark.parametrize("n_world", ["0", "1", "T-1", "T", "T+1"])
def test_row_counts_around_a_tile(gpu, cons, n_world, n_views):
    T = tile()
    n = {"0": 0, "1": 1, "T-1": T - 1, "T": T, "T+1": T + 1}[n_world]
    want = check(gpu, cons, raw_inputs(n + n_views, n, n_views, keep_every=2))
    assert want["verdict"][0] == K.OK and int(want["counts_out"][0]) >= (n - n // 41) // 2 - 1 and int(want["counts_out"].sum()) == n
    check(gpu, cons, raw_inputs(n + n_views, n, n_views, keep_every=2, room=n // 4))
    if n > 8:
        check(gpu, cons, raw_inputs(n + n_views, n, n_views, keep_every=2, world_pad=5))


def test_rows_beyond_one_pass_of_the_tile_sums_with_a_sparse_keep_pattern(gpu, cons):
    T = tile()
    n = 256 * T + 1
    inp = raw_inputs(5, n, 3, keep_every=T + 7)                        # fewer than one point per tile; the last row is one
    inp["world"][n - 1] = (3.0, 6.0, 12.0, 3.0)
    inp["world"][256 * T - 1] = (1.0, 2.0, 3.0, 0.5)
    want = check(gpu, cons, inp)
    points = int(want["counts_out"][0])
    assert want["verdict"][0] == K.OK and 250 <= points <= 260 and int(want["counts_out"].sum()) == n
    assert int(want["key"][points - 1]) == n - 1 and np.array_equal(want["xyz"][15 + points - 1], [1.0, 2.0, 4.0])
    short = dict(inp, room=points - 1)
    assert check(gpu, cons, short)["verdict"][0] == K.OVERFLOW


@pytest.mark.parametrize("name", list(DESIGNED))
def test_designed_cases(gpu, cons, name):
    check(gpu, cons, DESIGNED[name], statement=name not in K.BAD_TABLES)


@pytest.mark.parametrize("name", list(RANDOM))
def test_random_reconstructions(gpu, cons, name):
    """among them views with 0, 1, 63, 64, 255, 256 and 257 counted features under cap_per_img = 320"""
    inp = K.random_export(**RANDOM[name])
    want = check(gpu, cons, inp, statement=True)
    if name == "the sum order's thread counts":
        assert inp["cap"] == 320 and (want["cameras"][:, 9] == 0.0).sum() == 1


def test_the_bytes_do_not_depend_on_the_call_before(gpu, cons):
    T = tile()
    inp = raw_inputs(21, 3 * T + 5, 3)
    first = device_export(gpu, cons, inp)
    check(gpu, cons, raw_inputs(22, T + 7, 1, keep_every=5))            # another shape: the scratch is laid out differently
    assert_same(device_export(gpu, cons, inp), first)
    assert_same(first, K.export(inp))


def test_a_refused_call_launches_nothing(gpu, cons):
    from cv_amd import _lib
    inp = DESIGNED["room exact"]
    fill = K.outputs(inp)
    for over in (dict(view_blocks=[2, 2]), dict(view_blocks=[2, 3]), dict(view_blocks=[])):
        with pytest.raises(_lib.AkzError):
            device_export(gpu, cons, inp, over=over)
    up = uploader(gpu)
    d_in = {k: up(inp[k]) for k in INPUTS}
    d = {k: up(fill[k]) for k in K.OUTPUTS}
    from cv_amd.export import ReconstructionExport
    with pytest.raises(_lib.AkzError):                                  # an output over the world table
        ReconstructionExport(cons).export_device(d_in["world"], inp["n_world"], d_in["start"], d_in["obs"], inp["n_obs"], inp["n_landmarks"],
                                                 d_in["colors"], [2, 0], d_in["counts"], d_in["landmarks"], inp["cap"], inp["n_blocks"], d_in["poses"],
                                                 inp["room"], d["xyz"], d["rgb"], d["key"], d["cameras"], d["counts_out"], d_in["world"])
    cons.sync()
    assert_same(back(d, fill, K.OUTPUTS), fill)
    assert np.array_equal(back(d_in, inp, ("world",))["world"], inp["world"])


# ---- the chain -----------------------------------------------------------------------------------------------------------
def triangulated_scene(torch, seed=4, n_views=8, n_landmarks=300):
    """an observation_filter_checker scene as the arrays of a triangulation and of the export behind it"""
    import observation_filter_checker as F
    from test_gpu_landmark_table import rs_camera
    from cv_amd import _lib, triangulation
    from cv_amd.reconstruction import ObservationFilter
    dev = torch.device("cuda", 0)
    sc = F.scene(seed, n_views=n_views, n_landmarks=n_landmarks, lengths=(2, 6), outlier_fraction=0.1)
    cap = sc["kps"].shape[1]
    start, obs = sc["start"].astype(np.int64), sc["obs"].astype(np.uint32).reshape(-1, 2)
    rows = [[(int(b), int(f)) for b, f in obs[start[l]:start[l + 1]]] for l in range(n_landmarks)]
    lm = np.full((n_views, cap), K.NONE, np.uint32)
    for l, row in enumerate(rows):
        for b, f in row:
            lm[b, f] = min(lm[b, f], l)
    counts = np.array([int(obs[obs[:, 0] == b, 1].astype(np.int64).max(initial=-1)) + 1 for b in range(n_views)], np.uint32)
    table = triangulation.LandmarkTable(torch, lists=rows)
    return dict(sc=sc, cap=cap, rows=rows, landmarks=lm, counts=counts, table=table, cam=rs_camera(sc["cam"]),
                params=ObservationFilter.params(minimum_robust_landmarks=8).triangulate, d_poses=torch.from_numpy(sc["poses"].copy()).to(dev),
                d_kps=_lib.device_bytes(torch, sc["kps"].view(np.uint8), dev), view_blocks=list(range(n_views - 1, -1, -1)))


def test_triangulate_then_export_without_a_wait_between_them(gpu, cons):
    from cv_amd import _lib, triangulation
    torch = gpu
    s = triangulated_scene(torch)
    dev = torch.device("cuda", 0)
    n_views, cap, table = len(s["view_blocks"]), s["cap"], s["table"]
    runs = []
    for _ in range(2):
        world, reason = table.new_world(), torch.zeros((table.n_landmarks,), dtype=torch.uint8, device=dev)
        triangulate = lambda d_in: triangulation.triangulate_landmarks_device(
            cons._h, table, s["d_kps"], cap, n_views, s["d_poses"], s["cam"], s["params"], d_in["world"], reason,
            _lib.wait_handle(torch.cuda.current_stream(dev)))
        inp = K.inputs(np.zeros((table.n_landmarks, 4)), s["rows"], s["view_blocks"], s["counts"], s["landmarks"], s["sc"]["poses"], cap, pad=0)
        got = device_export(torch, cons, inp, d_in=dict(world=world, start=table.d_start, obs=table.d_obs, poses=s["d_poses"]), before=triangulate)
        runs.append((got, world.cpu().numpy()))
    (first, w1), (second, w2) = runs
    assert np.array_equal(w1.view(np.uint64), w2.view(np.uint64))
    assert_same(second, first)
    host = K.export(dict(inp, world=np.ascontiguousarray(w1)))         # the host build on the triangulation's own output
    assert_same(first, host)
    assert host["verdict"][0] == K.OK and int(host["counts_out"][0]) > 100 and int(host["counts_out"][1]) > 0
    assert np.all(host["cameras"][:, 9] > 0.0)


def test_export_reconstruction_waits_once_and_writes_the_host_builds_file(gpu, cons, tmp_path, monkeypatch):
    from cv_amd import _lib, export, triangulation
    from cv_amd.reconstruction import export_reconstruction
    torch = gpu
    s = triangulated_scene(torch, seed=6)
    dev = torch.device("cuda", 0)
    n_views, cap, table = len(s["view_blocks"]), s["cap"], s["table"]
    world = table.new_world()
    triangulation.triangulate_landmarks_device(cons._h, table, s["d_kps"], cap, n_views, s["d_poses"], s["cam"], s["params"], world, None,
                                               _lib.wait_handle(torch.cuda.current_stream(dev)))
    cons.sync()
    inp = K.inputs(world.cpu().numpy(), s["rows"], s["view_blocks"], s["counts"], s["landmarks"], s["sc"]["poses"], cap, pad=0)
    host = K.export(inp)
    d_colors = _lib.device_bytes(torch, inp["colors"], dev)
    torch.cuda.synchronize()
    waits = []
    monkeypatch.setattr(type(cons), "sync", lambda self, _f=type(cons).sync: (waits.append("rs_sync"), _f(self))[1])
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: waits.append("synchronize"))
    result = export_reconstruction(torch, cons, table, world, d_colors, s["view_blocks"], s["counts"], s["landmarks"], cap, s["d_poses"],
                                   tmp_path / "cloud.ply")
    assert waits == ["rs_sync"]
    monkeypatch.undo()
    n = int(host["counts_out"][0])
    assert result.verdict == K.OK and np.array_equal(result.counts, host["counts_out"]) and np.array_equal(result.key, host["key"][:n])
    xyz, rgb, faces, _ = export.read_ply(tmp_path / "cloud.ply")
    assert np.array_equal(xyz.view(np.uint64), host["xyz"][:5 * n_views + n].view(np.uint64)) and np.array_equal(rgb, host["rgb"][:5 * n_views + n])
    assert len(faces) == 4 * n_views and np.array_equal(result.cameras.view(np.uint64), host["cameras"].view(np.uint64))


def test_the_native_mirror_writes_the_same_file(gpu, cons, tmp_path):
    """cv_sfm::ReconstructionExport of include/akaze.hpp from a process without Python (tests/cpp/export.cpp)"""
    import subprocess

    import host_build
    from cv_amd import export
    inp = K.random_export(**RANDOM["mixed rows"])
    want = K.export(inp)
    path = tmp_path / "call.bin"
    with open(path, "wb") as fp:
        fp.write(np.array([inp["n_world"], inp["n_landmarks"], inp["n_obs"], inp["n_blocks"], inp["cap"], len(inp["view_blocks"]), inp["room"], 1],
                          np.uint32).tobytes())
        for a in (inp["world"][:inp["n_world"]], inp["start"], inp["obs"][:inp["n_obs"]], inp["colors"], inp["view_blocks"], inp["counts"],
                  inp["landmarks"], inp["poses"]):
            fp.write(np.ascontiguousarray(a).tobytes())
    exe = host_build.native(tmp_path, "export.cpp", hip=True)
    r = subprocess.run([exe, str(path), str(tmp_path / "native.ply")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("export ok"), (r.returncode, r.stderr[-400:])
    out = {line.split(" ", 1)[0]: [int(v) for v in line.split()[1:]] for line in r.stdout.splitlines()[:-1]}
    assert out["counts"] == [int(v) for v in want["counts_out"]] and out["verdict"] == [K.OK]
    n = 5 * len(inp["view_blocks"]) + int(want["counts_out"][0])
    xyz, rgb, faces, _ = export.read_ply(tmp_path / "native.ply")
    assert np.array_equal(xyz.view(np.uint64), want["xyz"][:n].view(np.uint64)) and np.array_equal(rgb, want["rgb"][:n])
    assert len(faces) == 4 * len(inp["view_blocks"])


# ---- colours -----------------------------------------------------------------------------------------------------------
def test_the_batched_colour_sampler_is_the_oracles_and_the_single_frame_entrys(gpu):
    from oracle import oracle
    from cv_amd import _lib
    from cv_amd.akaze import Akaze
    torch = gpu
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(12)
    n, w, h, cap, pitch = 3, 64, 48, 40, 64 * 3 + 8                     # rows of 200 bytes: 8 bytes of padding behind each
    counts = np.array([0, 5, cap], np.uint32)
    frames = rng.integers(0, 256, (n, h, pitch)).astype(np.uint8)
    kps = np.zeros((n, cap), _lib.KP_DTYPE)
    kps["x"] = rng.uniform(-2.0, w + 2.0, (n, cap)).astype(np.float32)    # some windows leave the image: the default colour
    kps["y"] = rng.uniform(-2.0, h + 2.0, (n, cap)).astype(np.float32)
    kps["x"][2, :6] = [1.0, 1.0 - 1e-3, w - 3.0, w - 3.0 - 1e-3, 20.5, 33.0]   # the window test's edges
    kps["y"][2, :6] = [1.0, 10.0, h - 3.0 - 1e-3, h - 3.0, 20.5, 7.25]
    fill = np.full((n, cap, 3), K.FILL8, np.uint8)
    d_colors = _lib.device_bytes(torch, fill, dev)
    ak = Akaze.new(0.001)
    try:
        ctx = ak.context(w, h, n)
        ctx.sample_colors_device(_lib.device_bytes(torch, frames, dev), n, w, h, pitch, _lib.device_bytes(torch, kps.view(np.uint8), dev),
                                 _lib.device_bytes(torch, counts, dev), cap, d_colors, torch.cuda.current_stream(dev))
        _lib.check(_lib.lib().akz_sync(ctx.handle))
        got = d_colors.cpu().numpy().reshape(n, cap, 3)
        inside = 0
        for f in range(n):
            c = int(counts[f])
            rgb = np.ascontiguousarray(frames[f, :, :3 * w].reshape(h, w, 3))
            want = oracle.sample_colors_rgb8(rgb, kps[f, :c])
            assert np.array_equal(got[f, :c], want), f
            assert np.array_equal(got[f, :c], ctx.sample_colors(rgb, kps[f, :c])), f
            assert np.all(got[f, c:] == K.FILL8), f                     # rows behind the count still hold the fill
            inside += int((want.reshape(-1, 3) != 0).any(1).sum())
        assert inside >= 25
    finally:
        ak.close()
