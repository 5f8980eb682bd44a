"""hm_landmark_original_matches_batch_device (cv-sfm's original_matches, lib.rs:1549-1576, for the single-view refinement): the
kernel of hm_landmark_matches_ordered_batch_device with the drop of the matches without a world point disabled.  Given a world
table without "None" rows the two write the same bytes — with and without observation counts and a merge mask — and a table
with "None" rows gives the sub-list of the originals whose row has w >= 0, in order: the mapping the refinement's inlier
indices rely on.  The existing entry points still refuse a NULL table.  Run with -m gpu."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cv_amd import build
    build.build()
    return torch


@pytest.fixture(scope="module")
def rig(gpu):
    """(matcher, inputs): 4 frames of up to 1 024 features, 3 000 landmark keys and some beyond the table, collisions"""
    torch = gpu
    from cv_amd.knn import Matcher
    rng = np.random.default_rng(0x51E6)
    cap, F, n_world = 1024, 4, 3000
    nq = np.array([1024, 700, 0, 65], np.int32)
    best = np.zeros((F, cap, 3, 2), np.uint32)
    for f in range(F):
        for j in range(cap):
            best[f, j, :, 0] = rng.choice(n_world + 40, 3, replace=False)
    best[..., 1] = rng.integers(0, 300, (F, cap, 3))
    best[0, :, 0, 0] = rng.permutation(n_world)[:cap]
    best[1, 9, 1, 0] = 0xFFFFFFFF
    dec = rng.integers(0, 3, (F, cap)).astype(np.uint32)
    merge_ok = (rng.random((F, cap)) < 0.6).astype(np.uint8)
    obs = rng.integers(1, 6, n_world).astype(np.uint32)
    world = rng.standard_normal((n_world + F * cap, 4))
    world[:, 3] = np.abs(world[:, 3])
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(a).to(dev)
    d = dict(best=t(best.view(np.int32)), dec=t(dec.view(np.int32)), ok=t(merge_ok), obs=t(obs.view(np.int32)), nq=t(nq), world=t(world),
             cap=cap, F=F, n_world=n_world, world_host=world, dev=dev)
    m = Matcher(cap)
    yield m, d
    m.close()


def run(torch, m, d, original, mask, counts, world=None):
    from cv_amd import _lib
    L = _lib.lib()
    F, cap = d["F"], d["cap"]
    iq = np.arange(F, dtype=np.uint32)
    d_pairs = torch.full((F, cap, 2), -1, dtype=torch.int32, device=d["dev"])
    d_np = torch.full((F,), 77, dtype=torch.int32, device=d["dev"])
    head = (m.handle, d["best"].data_ptr(), d["dec"].data_ptr(), d["ok"].data_ptr() if mask else None, d["obs"].data_ptr() if counts else None,
            d["nq"].data_ptr(), iq.ctypes.data_as(C.c_void_p), cap, F)
    tail = (d_pairs.data_ptr(), d_np.data_ptr(), _lib.wait_handle(torch.cuda.current_stream()))
    if original:
        _lib.check(L.hm_landmark_original_matches_batch_device(*head, d["n_world"], *tail), "original_matches")
    else:
        _lib.check(L.hm_landmark_matches_ordered_batch_device(*head, (d["world"] if world is None else world).data_ptr(), d["n_world"], *tail),
                   "matches_ordered")
    _lib.check(L.hm_sync(m.handle), "hm_sync")
    return d_pairs.cpu().numpy().view(np.uint32), d_np.cpu().numpy()


@pytest.mark.parametrize("mask", [False, True])
@pytest.mark.parametrize("counts", [False, True])
def test_equal_to_the_ordered_lists_of_a_table_without_none_rows(gpu, rig, mask, counts):
    m, d = rig
    gp, gn = run(gpu, m, d, True, mask, counts)
    wp, wn = run(gpu, m, d, False, mask, counts)
    assert np.array_equal(gn, wn) and gp.tobytes() == wp.tobytes()
    assert gn[0] > 300 and gn[2] == 0 and (not mask or (gp[0, :gn[0], 1] >= d["n_world"]).any())


def test_the_consensus_list_is_the_sub_list_with_a_world_point(gpu, rig):
    m, d = rig
    world = d["world_host"].copy()
    world[np.random.default_rng(3).random(len(world)) < 0.25, 3] = -1.0
    gp, gn = run(gpu, m, d, True, True, True)
    wp, wn = run(gpu, m, d, False, True, True, world=gpu.from_numpy(world).to(d["dev"]))
    dropped = 0
    for f in range(d["F"]):
        orig = gp[f, :gn[f]]
        some = orig[world[orig[:, 1], 3] >= 0.0]
        assert wn[f] == len(some) and np.array_equal(wp[f, :wn[f]], some), f
        dropped += int(gn[f] - wn[f])
    assert dropped > 100


def test_the_existing_entry_points_still_refuse_a_null_table(gpu, rig):
    from cv_amd import _lib
    m, d = rig
    L = _lib.lib()
    iq = np.arange(d["F"], dtype=np.uint32)
    d_pairs = gpu.zeros((d["F"], d["cap"], 2), dtype=gpu.int32, device=d["dev"])
    d_np = gpu.zeros((d["F"],), dtype=gpu.int32, device=d["dev"])
    iq_p = iq.ctypes.data_as(C.c_void_p)
    assert L.hm_landmark_matches_ordered_batch_device(m.handle, d["best"].data_ptr(), d["dec"].data_ptr(), None, None, d["nq"].data_ptr(), iq_p,
                                                      d["cap"], d["F"], None, d["n_world"], d_pairs.data_ptr(), d_np.data_ptr(), None) == -1
    assert L.hm_landmark_matches_batch_device(m.handle, d["best"].data_ptr(), d["dec"].data_ptr(), None, d["nq"].data_ptr(), iq_p, d["cap"],
                                              d["F"], None, d["n_world"], d_pairs.data_ptr(), d_np.data_ptr(), None) == -1
    assert L.hm_landmark_pairs_batch_device(m.handle, d["best"].data_ptr(), d["dec"].data_ptr(), d["nq"].data_ptr(), iq_p, d["cap"], d["F"], None,
                                            d["n_world"], d_pairs.data_ptr(), d_np.data_ptr(), None) == -1
