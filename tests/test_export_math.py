"""The host's execution of include/akz_export_math.h (tests/cpp/export_host.c through host_build.load) held to the independent
statement of tests/export_statement.py: which landmarks are exported, their order, the keys, the colours, the counters, the
verdicts and the faces exactly; coordinates, cameras and frustum vertices under one bound.  rs_write_ply -> read_ply gives the
f64 bits and the colours back.  No GPU needed — the device is held to this host build byte for byte in
tests/test_gpu_export.py.

The bound: the largest absolute difference from the float64 statement (numpy's inverse, matmul and cross) over every scene of
this file — rotations from random axis-angles, |t| <= 10, points at distance 1 to 20 from the origin, so coordinates up to
about 30 — was measured as MEASURED_MAX; the tests assert 4 times that, the margin for numpy's matmul order differing between
builds.  Every output is a handful of products of such numbers, so the measured maximum itself has to lie below 1e-12
(asserted)."""
import numpy as np
import pytest

import export_checker as K
import export_statement as S

MEASURED_MAX = 3.552713678800501e-15
BOUND = 4 * MEASURED_MAX

DESIGNED = K.designed_cases()
RANDOM = {
    "mixed rows": dict(seed=1, n_world=60, view_features=[5, 0, 8]),
    "one view": dict(seed=2, n_world=40, view_features=[3]),
    "no row with a point": dict(seed=3, n_world=30, view_features=[4, 4], keep=0.0),
    "every row with a point": dict(seed=4, n_world=50, view_features=[6, 2, 1, 0], keep=1.0),
    "room below the points": dict(seed=5, n_world=80, view_features=[7, 7], room=11),
    "world rows behind the table": dict(seed=6, n_world=70, view_features=[8, 1], world_pad=9),
    "views past one pass of the threads": dict(seed=7, n_world=400, view_features=[255, 256, 257, 300], cap=320),
    "the sum order's thread counts": dict(seed=9, n_world=500, view_features=[0, 1, 63, 64, 255, 256, 257], cap=320),
    "long lists": dict(seed=8, n_world=90, view_features=[2, 2, 2], max_len=9),
}


def test_the_bound_is_the_measured_one_and_small():
    assert 0.0 < MEASURED_MAX < 1e-12 and BOUND == 4 * MEASURED_MAX


@pytest.mark.parametrize("name", [n for n in DESIGNED if n not in K.BAD_TABLES])
def test_designed_cases_equal_the_statement(name):
    inp = DESIGNED[name]
    K.check_against_statement(inp, K.export(inp), BOUND)


@pytest.mark.parametrize("name", list(RANDOM))
def test_random_reconstructions_equal_the_statement(name):
    inp = K.random_export(**RANDOM[name])
    st, _ = K.check_against_statement(inp, K.export(inp), BOUND)
    if name == "room below the points":
        assert st["verdict"] == S.OVERFLOW and st["counts"][0] > 11
    if name == "no row with a point":
        assert st["counts"][0] == 0 and all(c["focal_length"] == 0.0 for c in st["cameras"])
    if name == "world rows behind the table":
        assert st["counts"][3] >= 3


def test_what_the_designed_cases_decide():
    run = lambda name: K.export(DESIGNED[name])
    counts = lambda name: [int(v) for v in run(name)["counts_out"]]
    o = run("w of 1, 1e-300, +0, -0 and -1")
    assert [int(v) for v in o["counts_out"]] == [2, 1, 2, 0] and [int(k) for k in o["key"][:2]] == [0, 1] and o["verdict"][0] == K.OK
    first = 10
    assert np.array_equal(o["xyz"][first], [1.0, 2.0, 4.0])
    assert np.array_equal(o["xyz"][first + 1], np.array([1e-300, 2e-300, 4e-300]) / 1e-300)              # one IEEE division each
    inp = DESIGNED["w of 1, 1e-300, +0, -0 and -1"]
    assert np.array_equal(o["rgb"][first], inp["colors"][0, 1]) and np.array_equal(o["rgb"][first + 1], inp["colors"][2, 0])
    assert np.all(o["rgb"][:first] == S.CAMERA_COLOR)
    assert counts("an empty list under w > 0") == [2, 0, 0, 1]
    assert counts("a first observation outside the blocks") == [2, 0, 0, 1]
    assert counts("a first observation outside the capacity") == [2, 0, 0, 1]
    assert counts("a later observation outside the colours") == [3, 0, 0, 0]
    assert counts("a world row behind the landmark table") == [3, 0, 0, 1]
    assert counts("no landmark") == [0, 0, 0, 0]
    exact, short, none = run("room exact"), run("room one short"), run("room of none")
    assert exact["verdict"][0] == K.OK and short["verdict"][0] == K.OVERFLOW == none["verdict"][0]
    assert [int(v) for v in short["counts_out"]] == [3, 0, 0, 0] == [int(v) for v in none["counts_out"]]      # the true number
    assert np.array_equal(short["xyz"], exact["xyz"][:-1]) and np.array_equal(short["key"], exact["key"][:2])
    assert K.is_fill(none["key"])
    o = run("a view with no feature that has a point")
    assert np.all(o["cameras"][:, 9] == 0.0)
    for v in range(2):                                                                                    # focal length 0: every corner is the centre
        assert np.all(o["xyz"][5 * v:5 * v + 5] == o["xyz"][5 * v])
    assert np.all(run("a landmark key at and above n_world")["cameras"][:, 9] > 0.0)


@pytest.mark.parametrize("name", K.BAD_TABLES)
def test_a_broken_table_gives_no_point_and_still_the_cameras(name):
    inp = DESIGNED[name]
    o = K.export(inp)
    assert int(o["verdict"][0]) == K.BAD_TABLE and [int(v) for v in o["counts_out"]] == [0, 0, 0, 0]
    assert K.is_fill(o["key"]) and K.is_fill(o["xyz"][10:]) and K.is_fill(o["rgb"][10:])
    good = K.export(K.small(inp["world"], [[(0, 1)], [(1, 1)], [(2, 2)]]))
    assert np.array_equal(o["cameras"], good["cameras"]) and np.array_equal(o["xyz"][:10], good["xyz"][:10])
    assert np.all(o["cameras"][:, 9] > 0.0)


def test_a_camera_looks_along_its_axis():
    """a camera at (1, 2, 3) that looks along world x with world z up: pose = [R | -R c] with R's rows right, down, forward"""
    r = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]])
    c = np.array([1.0, 2.0, 3.0])
    pose = np.concatenate([r, (-r @ c)[:, None]], 1).reshape(12)
    cam, v = np.zeros(10), np.zeros(3)
    K.lib().ex_camera(pose.ctypes.data, 50.0, cam.ctypes.data)
    assert np.array_equal(cam, [1, 2, 3, 0, 0, 1, 1, 0, 0, 0.5])
    corners = []
    for k in range(5):
        K.lib().ex_camera_vertex(cam.ctypes.data, k, v.ctypes.data)
        corners.append(v.copy())
    # right = forward x up = (1, 0, 0) x (0, 0, 1) = (0, -1, 0); centre, up-right, up-left, down-left, down-right
    assert np.array_equal(corners, [[1, 2, 3], [1.5, 1.5, 3.5], [1.5, 2.5, 3.5], [1.5, 2.5, 2.5], [1.5, 1.5, 2.5]])


# ---- mutations: what a host build with one rule broken would give is caught --------------------------------------------
def mutants(inp):
    """name -> the output buffers of `inp` under one broken rule"""
    first = K.CAMERA_VERTICES * len(inp["view_blocks"])
    o = K.export(inp)
    last = K.export(inp)
    for k in range(min(int(o["counts_out"][0]), inp["room"])):
        block, feature = inp["rows"][int(o["key"][k])][-1]
        last["rgb"][first + k] = inp["colors"][block, feature]
    flipped = dict(inp, world=np.where((np.arange(4) == 3) & (inp["world"] < 0), -inp["world"], inp["world"]))
    swapped = K.export(inp)
    swapped["xyz"][2::5][:len(inp["view_blocks"])], swapped["xyz"][3::5][:len(inp["view_blocks"])] = (
        o["xyz"][3::5][:len(inp["view_blocks"])].copy(), o["xyz"][2::5][:len(inp["view_blocks"])].copy())
    return {"the last observation's colour": last, "w != 0 in the place of w > 0": K.export(flipped), "a swapped corner order": swapped}


@pytest.mark.parametrize("mutant", ["the last observation's colour", "w != 0 in the place of w > 0", "a swapped corner order"])
def test_a_broken_rule_is_caught(mutant):
    inp = K.random_export(**RANDOM["long lists"])
    K.check_against_statement(inp, K.export(inp), BOUND)                     # the rule as it is passes
    with pytest.raises(AssertionError):
        K.check_against_statement(inp, mutants(inp)[mutant], BOUND)
    if mutant == "w != 0 in the place of w > 0":                             # and so do the designed rows
        inp = DESIGNED["w of 1, 1e-300, +0, -0 and -1"]
        with pytest.raises(AssertionError):
            K.check_against_statement(inp, mutants(inp)[mutant], BOUND)


# ---- the file ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ply():
    from cv_amd.build import build
    build()
    from cv_amd import export
    return export


@pytest.mark.parametrize("faces", [True, False])
@pytest.mark.parametrize("n_cameras,n_points", [(2, 7), (0, 5), (3, 0), (0, 0)])
def test_write_ply_then_read_ply_gives_the_bits_back(ply, tmp_path, faces, n_cameras, n_points):
    rng = np.random.default_rng(n_cameras + 10 * n_points)
    n = 5 * n_cameras + n_points
    xyz = rng.normal(size=(n, 3)) * 10.0 ** rng.integers(-30, 30, (n, 3))
    xyz.reshape(-1)[:min(n * 3, 6)] = [0.0, -0.0, 1e-310, np.finfo(np.float64).max, -1.0 / 3.0, 5e-324][:min(n * 3, 6)]
    rgb = rng.integers(0, 256, (n, 3)).astype(np.uint8)
    path = tmp_path / "cloud.ply"
    ply.write_ply(path, xyz, rgb, n_cameras, camera_faces=faces)
    got_xyz, got_rgb, got_faces, comments = ply.read_ply(path)
    assert np.array_equal(got_xyz.view(np.uint64), xyz.view(np.uint64)) and np.array_equal(got_rgb, rgb)
    assert comments == ["Exported from rust-cv/vslam-sandbox"]
    if faces:
        assert [tuple(int(v) for v in f) for f in got_faces] == S.faces(n_cameras)
    else:
        assert got_faces is None
    text = open(path).read()
    head = text.split("end_header\n")[0].split("\n")
    want = ["ply", "format ascii 1.0", "comment Exported from rust-cv/vslam-sandbox", "element vertex %d" % n, "property double x",
            "property double y", "property double z", "property uchar red", "property uchar green", "property uchar blue"]
    want += ["element face %d" % (4 * n_cameras), "property list uchar int vertex_index"] if faces else []
    assert head == want + [""]
    assert text.endswith("\n") and len(text.split("end_header\n")[1].split("\n")) == n + (4 * n_cameras if faces else 0) + 1


def test_write_ply_refuses_what_it_cannot_write(ply, tmp_path):
    from cv_amd import _lib
    xyz, rgb = np.zeros((4, 3)), np.zeros((4, 3), np.uint8)
    with pytest.raises(_lib.AkzError):
        ply.write_ply(tmp_path / "a.ply", xyz, rgb, 1)                       # a camera has five vertices
    with pytest.raises(_lib.AkzError):
        ply.write_ply(tmp_path / "no" / "such" / "directory.ply", xyz, rgb, 0)
    with pytest.raises(ValueError):
        ply.write_ply(tmp_path / "b.ply", xyz, rgb[:3], 0)
