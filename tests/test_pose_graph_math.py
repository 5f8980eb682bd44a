"""include/akz_pose_graph_math.h, compiled by the host compiler (tests/pose_graph_checker.py), against an independent numpy
statement of the Rust text (tests/pose_graph_statement.py).  No GPU: the device is held to this host build bit for bit by
tests/test_gpu_pose_graph.py, and this file holds the host build to the reference's text."""
import math

import numpy as np
import pytest

import pose_graph_checker as P
import pose_graph_statement as S

# ---- measured on the host build (x86-64, glibc's libm, numpy's arccos / sin / cos), then fixed ----
ACOS_MEASURED_ULP = 3.0
# the largest difference of a pose component, host build (wave order) against the statement, after so many rounds at the
# default rate, on the two graphs of `graphs` below: the values this machine gave, asserted with a margin of 4
POSE_MEASURED = {"ring8": {1: 8.9e-16, 64: 1.7e-14, 1024: 4.1e-11}, "grid9": {1: 4.5e-16, 64: 1.2e-14, 1024: 3.9e-12}}
# the difference between the host build's and the statement's ratio of the largest edge residual after 1 024 rounds to the
# one before, measured the same way
RATIO_MEASURED = {"ring8": 7.0e-11, "grid9": 8.1e-12}
MARGIN = 4.0
ROUNDS = (1, 64, 1024)


def make_graphs():
    return {"ring8": P.Graph(11, 8),
            "grid9": P.Graph(12, 9, grid=True, triples=[(0, 1, 3), (1, 2, 4), (3, 4, 6), (4, 5, 7), (4, 7, 8), (0, 4, 8), (2, 4, 6)])}


@pytest.fixture(scope="module")
def relaxed():
    """name -> dict(graph, A, statement {rounds: poses [n][12]}, host {rounds: result}, sequential {rounds: result}), computed
    once: the statement's 1 024 rounds in numpy take a few seconds a graph"""
    out = {}
    for name, g in make_graphs().items():
        A, sg = P.batch([g]), g.statement_graph()
        sp, done, st = {v: g.poses[v] for v in range(g.n)}, 0, {}
        for rounds in ROUNDS:
            sp, ran, bad = S.relax(sp, sg, rounds - done)
            assert ran == rounds - done and not bad
            done = rounds
            st[rounds] = np.stack([sp[v] for v in range(g.n)]).reshape(-1, 12)
        out[name] = dict(graph=g, A=A, sg=sg, statement=st, host={r: P.relax(A, P.settings(r)) for r in ROUNDS},
                         sequential={r: P.relax(A, P.settings(r), sequential=True) for r in ROUNDS})
    return out


def test_six_edges_are_the_statements():
    g = P.Graph(5, 6)
    got = P.edges(g.cposes, g.cverdict)
    for c in range(len(g.views)):
        want = S.edge_constraints(g.views[c], g.cposes[c, 0], g.cposes[c, 1])
        for slot, (target, (other, expected)) in enumerate(want):
            assert target == g.views[c][P.lib().pg_slot_target(slot)] == g.views[c][P.SLOT_TARGET[slot]]
            assert other == g.views[c][P.lib().pg_slot_other(slot)] == g.views[c][P.SLOT_OTHER[slot]]
            assert np.abs(got[c, slot].reshape(3, 4) - expected).max() < 1e-14, (c, slot)
    # first and second themselves pass through untouched
    assert got[0, 2].tobytes() == g.cposes[0, 0].tobytes() and got[0, 5].tobytes() == g.cposes[0, 1].tobytes()
    # a refused constraint: six zero matrices, its (NaN) poses are not read
    r = P.Graph(5, 6, refused=[1])
    e = P.edges(r.cposes, r.cverdict)
    assert e[1].tobytes() == np.zeros((6, 12)).tobytes() and e[0].tobytes() == got[0].tobytes()


def test_log_exp_round_trip_and_the_statement():
    rng = np.random.default_rng(3)
    for scale in (1e-6, 1e-3, 0.3, 1.5, 3.0):
        for _ in range(50):
            w = scale * rng.standard_normal(3) / np.sqrt(3.0)
            if np.linalg.norm(w) >= math.pi - 1e-3:
                continue
            pose = np.hstack([P.exp(w), np.zeros((3, 1))])
            got = P.log(pose)
            # c = (trace - 1) / 2 carries the rounding of three entries near 1 and of their sum, 4 eps at the most, and
            # d(angle) = d(c) / sin(angle): the log through acos is ill-conditioned near 0 and near pi
            tol = 1e-15 + 4 * np.finfo(np.float64).eps / np.sin(np.linalg.norm(w))
            assert np.abs(got - w).max() < tol, (w, got)
            assert np.abs(got - S.log(pose[:, :3])).max() < tol
            assert np.abs(P.exp(w) - S.exp(w)).max() < 1e-15
    assert P.log(np.hstack([np.eye(3), np.ones((3, 1))])).tobytes() == np.zeros(3).tobytes()
    nan = np.hstack([np.full((3, 3), np.nan), np.zeros((3, 1))])
    assert P.log(nan).tobytes() == np.zeros(3).tobytes()              # so3.rs:268-272: a vector holding a NaN becomes zero
    delta = np.hstack([P.exp([0.1, -0.2, 0.05]), np.array([[1.0], [2.0], [3.0]])])
    assert np.abs(P.se3(delta) - S.se3(delta)).max() < 1e-15 and P.se3(delta)[:3].tolist() == [1.0, 2.0, 3.0]


def test_acos_against_libm():
    """akz_pm_acos against numpy's arccos (the host libm's acos) over 2 000 001 evenly spaced points of [-1, 1], the 4 096
    doubles next to each end and points 1e-16 .. 1e-12 away from +-1.  Measured on x86-64 with glibc: at most 3 ulp (1 303 214
    points exact, 699 086 at 1 ulp, 5 906 at 2, one at 3); that measured value, doubled, is the bound."""
    ends = [1.0]
    for _ in range(4095):
        ends.append(np.nextafter(ends[-1], -2.0))
    ends = np.array(ends)
    d = np.array([1e-16, 3e-16, 1e-15, 1e-14, 1e-13, 5e-13, 1e-12])
    c = np.concatenate([np.linspace(-1.0, 1.0, 2000001), ends, -ends, 1.0 - d, -1.0 + d])
    mine, ref = P.acos(c), np.arccos(c)
    assert P.acos([1.0])[0] == 0.0 and not np.signbit(P.acos([1.0])[0]) and P.acos([-1.0])[0] == math.pi and P.acos([0.0])[0] == math.pi / 2
    assert np.isnan(P.acos([np.nan])[0])
    assert np.all(mine[ref == 0.0] == 0.0)
    nz = ref != 0.0
    ulp = np.abs(mine[nz] - ref[nz]) / np.spacing(ref[nz])
    print("akz_pm_acos: largest distance to libm", ulp.max(), "ulp at", c[nz][ulp.argmax()])
    assert ulp.max() <= 2.0 * ACOS_MEASURED_ULP


def test_host_build_against_the_statement(relaxed):
    """The whole relaxation, host build (wave order) against the numpy statement (libm, sequential order).  Largest difference
    of a pose component measured on this machine:
        ring8 (8 views, 8 constraints, 48 edges)   1 round 8.9e-16   64 rounds 1.7e-14   1 024 rounds 4.1e-11
        grid9 (9 views, 7 constraints, 42 edges)   1 round 4.5e-16   64 rounds 1.2e-14   1 024 rounds 3.9e-12
    asserted at 4 times that.  The differences are those of libm against akz_portable_math.h and of the order of a view's
    sum; the update is a contraction towards the constraints' consensus, which does not amplify them beyond the drift along
    the graph's free rigid motion."""
    for name, r in relaxed.items():
        for rounds in ROUNDS:
            h = r["host"][rounds]
            assert h["verdict"].tolist() == [P.OK] and h["stats"][0, P.S_ROUNDS] == rounds and np.all(h["state"] == P.VIEW_UPDATED)
            diff = np.abs(h["poses"] - r["statement"][rounds]).max()
            print(name, rounds, "rounds: host build against statement", diff)
            assert diff <= MARGIN * POSE_MEASURED[name][rounds], (name, rounds, diff)


def test_wave_order_against_sequential_order(relaxed):
    """What fixing the wave's order of a view's sum costs against the reference's sequential fold, on a graph run to 1 024
    rounds.  Measured: one round 1.1e-19 (ring8) and 0 (grid9) — rows of 6 edges differ only through the butterfly's
    pairing —, 1 024 rounds 1.8e-11 and 1.2e-12, the same size as either order's distance to the statement.  The bound is
    that distance's: the sequential build is as far from the statement as the wave build is."""
    for name, r in relaxed.items():
        A = r["A"]
        for v in range(r["graph"].n):
            a, b = P.view_sum(A, v), P.view_sum(A, v, sequential=True)
            assert np.abs(a - b).max() <= 8 * np.finfo(np.float64).eps * np.abs(b).max()
        for rounds in ROUNDS:
            cost = np.abs(r["host"][rounds]["poses"] - r["sequential"][rounds]["poses"]).max()
            print(name, rounds, "rounds: wave order against sequential order", cost)
            assert cost <= MARGIN * POSE_MEASURED[name][rounds]
            assert np.abs(r["sequential"][rounds]["poses"] - r["statement"][rounds]).max() <= MARGIN * POSE_MEASURED[name][rounds]


def test_the_relaxation_reduces_the_residual(relaxed):
    """The physical check, host build alone: after 1 024 rounds at the default rate the largest edge residual
    |se3(expected * w_other * w_view^-1)| of a consistent graph is smaller than before.  Measured ratios after / before:
        ring8   statement 0.02174015602183   host build 0.02174015609141   difference 7.0e-11
        grid9   statement 0.06457952306951   host build 0.06457952307758   difference 8.1e-12
    The host build's ratio is held to the statement's own at 4 times that measured difference, the margin of the pose test."""
    for name, r in relaxed.items():
        A, g = r["A"], r["graph"]
        before = P.residual(A["poses"], A)
        after = P.residual(r["host"][1024]["poses"], A)
        s_before = S.residual({v: g.poses[v] for v in range(g.n)}, r["sg"])
        s_after = S.residual({v: p.reshape(3, 4) for v, p in enumerate(r["statement"][1024])}, r["sg"])
        print(name, "residual before", before, "after", after, "ratio", after / before, "statement's ratio", s_after / s_before)
        assert after < before and s_after < s_before
        print(name, "ratio difference", abs(after / before - s_after / s_before))
        assert abs(after / before - s_after / s_before) <= MARGIN * RATIO_MEASURED[name]


def unit(rng):
    v = rng.standard_normal(3)
    return v / np.linalg.norm(v)


def turned(truth, angle, rng):
    return np.stack([S.mul(np.hstack([S.exp(angle * unit(rng)), np.zeros((3, 1))]), p) for p in truth])


ROT = np.array([0, 1, 2, 4, 5, 6, 8, 9, 10])      # the rotation's entries of a row-major [R | t]


def test_a_rotation_below_the_floor_is_left_as_it_is():
    """a rotation below about 1.5e-8 rad has (trace - 1) / 2 == 1.0, acos gives 0 and the log is exactly zero.
    A graph of views that differ by translations only, each turned by 1e-9 rad, keeps the bits of every rotation over 64
    rounds while its translations move.
    What this test found beside that (measured, written into DESIGN.md §7 too): the floor is clean only while the trace of
    the delta is computed exactly.  Between views with general rotations the two isometry products leave the trace an ulp
    or two beside 3; when it falls below, acos reads 1.5e-8 .. 3e-8 rad along the true axis, and the rotations of such a
    graph do move: 4.7e-11 in one round, 9.6e-10 after 64 and 9.7e-10 after 1 024 rounds (largest entry)."""
    rng = np.random.default_rng(8)
    for angle in (1e-10, 1e-9, 5e-9):       # (from 1.05e-8 on a cosine rounds below 1 and the log may read as 1.5e-8)
        assert np.all(P.log(np.hstack([P.exp(angle * unit(rng)), np.zeros((3, 1))])) == 0.0)      # +0.0 or -0.0: axis * 0
    assert np.linalg.norm(P.log(np.hstack([P.exp(3e-8 * unit(rng)), np.zeros((3, 1))]))) > 2.9e-8
    g = P.Graph(21, 6, noise=0.0)
    g.truth[:, :, :3] = np.eye(3)
    for c, (v0, v1, v2) in enumerate(g.views):
        g.cposes[c, 0], g.cposes[c, 1] = S.mul(g.truth[v1], S.inverse(g.truth[v0])), S.mul(g.truth[v2], S.inverse(g.truth[v0]))
    g.poses = turned(g.truth, 1e-9, rng)
    assert np.any(g.poses[:, :, :3] != g.truth[:, :, :3])
    A = P.batch([g])
    h = P.relax(A, P.settings(64))
    assert h["verdict"].tolist() == [P.OK]
    assert h["poses"][:, ROT].tobytes() == A["poses"][:, ROT].tobytes()
    assert np.any(h["poses"][:, 3::4] != A["poses"][:, 3::4])           # the translations are not at a floor
    # the same graph 1e-6 rad off does move in rotation
    g.poses = turned(g.truth, 1e-6, rng)
    A = P.batch([g])
    assert P.relax(A, P.settings(64))["poses"][:, ROT].tobytes() != A["poses"][:, ROT].tobytes()
    # general rotations: the trace's rounding decides.  A log below the floor reads as at most acos(1 - 4 ulp) = 3e-8, so a
    # view of 6 edges moves by at most 64 rounds x 1e-3 x 6 x 3e-8 = 1.2e-8.
    g = P.Graph(21, 6, noise=0.0)
    g.poses = turned(g.truth, 1e-9, rng)
    A = P.batch([g])
    moved = np.abs(P.relax(A, P.settings(64))["poses"][:, ROT] - A["poses"][:, ROT]).max()
    print("general rotations 1e-9 rad off: the largest rotation entry moved by", moved)
    assert 0.0 < moved <= 1.2e-8


def test_from_se3_does_not_rotate_the_translation():
    """CameraToCamera::from_se3 is from_parts(translation, exp(rotation)) (pose.rs:62-66); Se3TangentSpace::isometry, which
    akz_tv_apply_delta implements, rotates the translation by exp(rotation).  This fails if that function is reused."""
    net = np.array([0.5, -0.25, 1.0, 0.3, -0.4, 0.2])
    pose = P.Graph(1, 3).truth[1]
    got = P.from_se3_mul(net, pose)
    want = S.mul(S.from_se3(net), pose)
    assert np.abs(got - want).max() < 1e-15
    ident = np.hstack([np.eye(3), np.zeros((3, 1))])
    assert P.from_se3_mul(net, ident)[:, 3].tolist() == net[:3].tolist()            # the translation as it came
    rotated = P.apply_delta(net, ident)
    assert np.abs(rotated[:, 3] - S.exp(net[3:]) @ net[:3]).max() < 1e-15
    assert np.abs(rotated[:, 3] - net[:3]).max() > 0.1                             # and the other function does rotate it
    ok, out = P.view_update(net / 1e-3, 1e-3, pose)
    assert ok == 1 and np.abs(out - want).max() < 1e-14
    ok, out = P.view_update([np.inf, 0, 0, 0, 0, 0], 1e-3, pose)
    assert ok == 0 and out.tobytes() == pose.tobytes()
    ok, out = P.view_update([0, 0, 0, 0, np.nan, 0], 1e-3, pose)
    assert ok == 0 and out.tobytes() == pose.tobytes()


def test_verdicts_of_the_host_build():
    """few views, a view without constraints, refused constraints, a NaN pose: the verdicts and stats the issue states"""
    st = P.settings(4)
    # two views updated only: decided before round 0, poses untouched
    g = P.Graph(2, 4, triples=[(0, 1, 2)], refused=[0])
    A = P.batch([g])
    h = P.relax(A, st)
    assert h["verdict"].tolist() == [P.FEW_VIEWS] and h["poses"].tobytes() == A["poses"].tobytes()
    assert h["state"].tolist() == [P.VIEW_NO_CONSTRAINT] * 4 and h["stats"][0].tolist() == [4, 0, 0, 0, 1, P.NO_VIEW, 0, 0]
    # view 3 has no constraint: untouched, the others move
    A = P.batch([P.Graph(2, 4, triples=[(0, 1, 2)])])
    h = P.relax(A, st)
    assert h["verdict"].tolist() == [P.OK] and h["state"].tolist() == [0, 0, 0, 1] and h["stats"][0].tolist() == [4, 3, 6, 4, 2, P.NO_VIEW, 0, 0]
    assert h["poses"][3].tobytes() == A["poses"][3].tobytes() and np.all(h["poses"][:3] != A["poses"][:3])
    # a NaN in view 2's pose: every view with an edge to it, and itself, is not finite in round 0
    A = P.batch([P.Graph(2, 6)])
    A["poses"][2, 7] = np.nan
    h = P.relax(A, st)
    assert h["verdict"].tolist() == [P.NONFINITE] and h["stats"][0, P.S_ROUNDS] == 1 and h["stats"][0, P.S_FIRST_BAD_VIEW] == 0
    assert h["state"].tolist() == [2, 2, 2, 2, 2, 0]          # ring of 6: views 0 - 4 share a constraint with view 2
    assert h["poses"][:5].tobytes() == A["poses"][:5].tobytes() and h["poses"][5].tobytes() != A["poses"][5].tobytes()
    # 0 rounds: nothing moves, the graph is fine
    h = P.relax(P.batch([P.Graph(2, 6)]), P.settings(0))
    assert h["verdict"].tolist() == [P.OK] and h["stats"][0, P.S_ROUNDS] == 0
