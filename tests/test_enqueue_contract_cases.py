"""The case table of tests/enqueue_contract.py without a GPU: for every row TRUE and DECOY are calls of equal shapes and equal
scalars, both keep the bounds of the entry — indices below their sizes, starts ascending, counts at most their capacities —
and they differ, so that a call which read the wrong one could show."""
import numpy as np
import pytest

import enqueue_contract as EC


@pytest.mark.parametrize("row", EC.ROWS, ids=repr)
def test_true_and_decoy_have_equal_shapes_and_keep_the_bounds(row):
    true, decoy = row.build(EC.SEED_TRUE), row.build(EC.SEED_DECOY)
    assert true.symbol == decoy.symbol == row.name.split("#")[0]
    assert true.shapes() == decoy.shapes()
    true.check()
    decoy.check()
    assert any(not np.array_equal(true.ins[k], decoy.ins[k]) for k in true.ins)
    assert bool(true.lists) == row.host_list
    for k in true.outs:                                                            # an in-place output starts as its input
        if k in true.ins:
            assert np.array_equal(true.outs[k], true.ins[k])
    again = row.build(EC.SEED_TRUE)                                                # a seed is a call
    assert all(np.array_equal(true.ins[k], again.ins[k]) for k in true.ins)


def test_every_family_has_a_row_and_names_are_unique():
    assert len({r.name for r in EC.ROWS}) == len(EC.ROWS)
    assert {r.family for r in EC.ROWS} == {"rs", "hm", "akz"}


def test_the_staging_ring_has_the_slots_the_tests_count_on():
    """hm_ctx::kStageRing is internal to cv_amd/csrc/hm_match.hip and no symbol exports it: the back-to-back test makes one call
    more than the ring has slots, by the number stated in enqueue_contract.HM_STAGE_RING; here that number is read from the source"""
    import os
    import re
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cv_amd", "csrc", "hm_match.hip")
    with open(path) as fp:
        found = re.findall(r"static constexpr int kStageRing = (\d+);", fp.read())
    assert found == [str(EC.HM_STAGE_RING)]


@pytest.mark.parametrize("name", ["rs_incorporate_reconstruction_device", "rs_add_views_device", "hm_knn_batch_device", "hm_match_batch_device",
                                  "akz_extract_batch_device"])
def test_the_seeds_of_the_back_to_back_calls_keep_one_shape(name):
    row = EC.BY_NAME[name]
    calls = [row.build(s) for s in (1, 2, 3, 4, 5, 102, 103, 104, 105, 106)]
    for c in calls:
        c.check()
        assert c.shapes() == calls[0].shapes()
    for true, decoy in zip(calls[:5], calls[5:]):                                  # every call's DECOY is not its TRUE
        assert any(not np.array_equal(true.ins[k], decoy.ins[k]) for k in true.ins)
