"""The order of a workgroup's sum over items (include/akz_sum_order.h), stated in numpy without the headers' loops, against the
host build's tree sums of the three-view and the single-view optimiser: equal in every byte.  No GPU needed; the kernels are
held to the host build bit for bit by tests/test_gpu_three_view.py and tests/test_gpu_single_view.py.

The statement, for 256 threads in waves of 64:
  1. thread t starts at 0 and adds the terms of items t, t + 256, ... in ascending order (a "None" item adds nothing);
  2. inside a wave the xor butterfly v[l] = v[l] + v[l ^ m], m = 32, 16, 8, 4, 2, 1;
  3. the four waves' sums in wave order, ((w0 + w1) + w2) + w3.
A term is what the host build returns for a one-item list in the reference's order (0 + g, the device of
tests/test_three_view_constraint_math.py's one-wave test)."""
import numpy as np
import pytest

import single_view_checker as V
import three_view_checker as T

THREADS, WAVE = 256, 64
# lane, wave and stride boundaries; the last of each list is the stage's maximum
SIZES = [1, 63, 64, 65, 255, 256, 257, 300]
TV_MAX, SV_MAX = 1024, 2048
SV_NONE = (0, 5, 64, 255, 256, 299, 700, 2047)      # matches whose world row has w == 0: Projective::point gives None


def block_sum(terms, width):
    """terms: one [width] array per item, or None for an item that is skipped"""
    part = np.zeros((THREADS, width))
    for t in range(THREADS):
        for i in range(t, len(terms), THREADS):
            if terms[i] is not None:
                part[t] = part[t] + terms[i]
    waves = part.reshape(THREADS // WAVE, WAVE, width)
    for m in (32, 16, 8, 4, 2, 1):
        waves = waves + waves[:, np.arange(WAVE) ^ m]
    assert all(np.all(w == w[0]) for w in waves)       # IEEE addition commutes: every lane ends with the same bits
    total = waves[0, 0]
    for w in range(1, THREADS // WAVE):
        total = total + waves[w, 0]
    return total


def invert(pose):
    r, t = pose[:, :3], pose[:, 3]
    return np.hstack([r.T, (-r.T @ t)[:, None]])


@pytest.fixture(scope="module")
def three_view():
    rig = T.Rig(21, TV_MAX, noise=0.5, perturb=2e-3)
    inv = np.stack([invert(p) for p in rig.pose_in])
    terms = [T.gradient_sum(inv, rig.common[i:i + 1], sequential=True) for i in range(TV_MAX)]
    return inv, rig.common, terms


@pytest.fixture(scope="module")
def single_view():
    rng = np.random.default_rng(22)
    pose = V.world_to_camera([0.33, -0.21, 0.4], [0.03, -0.05, 0.02])
    z = rng.uniform(4.0, 10.0, SV_MAX)
    points = np.stack([rng.uniform(-0.3, 0.3, SV_MAX) * z, rng.uniform(-0.2, 0.2, SV_MAX) * z, z], 1)
    bearing = V.bearings_of(V.project(pose, points) + 0.5 * rng.standard_normal((SV_MAX, 2)))
    world = V.homogeneous(points)
    world[list(SV_NONE), 3] = 0.0
    lm = np.hstack([bearing, np.stack([V.euclidean(w) for w in world])])
    pose = np.hstack([V.rodrigues(2e-3 * V.unit_vec(rng)) @ pose[:, :3], pose[:, 3:] + 2e-3])
    terms = [V.gradient_sum(pose, lm[i:i + 1], sequential=True) if V.landmark_delta(pose, lm[i, :3], lm[i, 3:])[0] else None
             for i in range(SV_MAX)]
    assert [i for i, t in enumerate(terms) if t is None] == sorted(SV_NONE)
    return pose, lm, terms


@pytest.mark.parametrize("n", SIZES + [TV_MAX])
def test_three_view_tree_sum_is_the_stated_order(three_view, n):
    inv, lm, terms = three_view
    assert block_sum(terms[:n], 12).tobytes() == T.gradient_sum(inv, lm[:n]).tobytes()


@pytest.mark.parametrize("n", SIZES + [SV_MAX])
def test_single_view_tree_sum_is_the_stated_order(single_view, n):
    pose, lm, terms = single_view
    assert block_sum(terms[:n], 6).tobytes() == V.gradient_sum(pose, lm[:n]).tobytes()


def test_the_order_is_not_the_sequential_one(three_view, single_view):
    """what the statement distinguishes: the reference's order gives other last bits"""
    inv, lm, _ = three_view
    assert T.gradient_sum(inv, lm).tobytes() != T.gradient_sum(inv, lm, sequential=True).tobytes()
    pose, lm, _ = single_view
    assert V.gradient_sum(pose, lm).tobytes() != V.gradient_sum(pose, lm, sequential=True).tobytes()
