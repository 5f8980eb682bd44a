"""The enqueue contract (DESIGN.md "Enqueue contract") on the MI355X: every row of tests/enqueue_contract.py
is called while the stream that produces its device inputs is still busy, and must give, in every byte of every output buffer,
what it gives on inputs that were complete before the call.  Run with -m gpu.

One test: (1) on a fresh context the call on TRUE and on DECOY inputs, both settled -> WANT and WANT_DECOY, which must differ;
(2) the input buffers hold DECOY; (3) a side stream sleeps for the calibrated delay, then copies TRUE over them and records
`done`; (4) `done` must not have happened; (5) the call with stream_to_wait = the side stream, and the moment it returns its
host lists are overwritten with DECOY's; (6) the documented sync of the context, no wait of torch's, and the outputs are WANT.
An entry that uploads no host list must have returned while the producer was busy; so must one that stages its lists through
the matcher's pinned ring, once the ring's slots are sized.  For the entries that upload a host list from pageable memory the
figure is printed, not asserted: DESIGN.md has the table.  No call is made with the wait left out and nothing races the GPU on purpose: that the inputs can tell is shown by (1) alone."""
import pytest

import enqueue_contract as EC

pytestmark = pytest.mark.gpu

RETURNED_EARLY = {}


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cv_amd import build
    build.build()
    return torch


@pytest.fixture(scope="module")
def delay(gpu):
    cycles, ms = EC.calibrate(gpu)
    print("ENQUEUE producer delay: %d cycles, %.1f ms" % (cycles, ms))
    assert ms >= 0.5 * EC.DELAY_MS
    return cycles


@pytest.fixture()
def context(gpu):
    made = []

    def make(family):
        made.append(EC.Context(family))
        return made[-1]

    yield make
    for c in made:
        c.close()


def settle(gpu, ctx, row, true, decoy):
    """step 1: WANT and WANT_DECOY on the fresh context.  A staged entry is settled twice over: the matcher sizes a slot of its
    staging ring on the slot's first use and waits for its stream when it does, so four calls leave every slot sized, as a
    context in use has them — and the same call must give the same bytes twice."""
    want, want_decoy = EC.settled(gpu, ctx, true), EC.settled(gpu, ctx, decoy)
    assert EC.differs(want, want_decoy), "TRUE and DECOY give the same outputs: the case cannot tell which was read"
    if row.staged:
        assert EC.HM_STAGE_RING == 4
        assert EC.differs(EC.settled(gpu, ctx, true), want) == [] and EC.differs(EC.settled(gpu, ctx, decoy), want_decoy) == []
    return want


@pytest.mark.parametrize("row", EC.ROWS, ids=repr)
def test_a_call_behind_a_busy_producer_gives_the_settled_bytes(gpu, delay, context, row):
    ctx = context(row.family)
    true, decoy = row.build(EC.SEED_TRUE), row.build(EC.SEED_DECOY)
    want = settle(gpu, ctx, row, true, decoy)
    (got,), (returned_early,) = EC.raced(gpu, ctx, [(true, decoy)], delay)
    print("ENQUEUE %s returned_early=%s" % (row.name, returned_early))
    assert EC.differs(got, want) == []
    if row.must_return_early:
        assert returned_early, "the entry blocked the host while the producer of its inputs was busy"


# (row, calls): N calls on one context before any sync.  hm: kStageRing + 1 calls, so that the ring of staging slots wraps
# while every call before is still stalled behind the producer; akz: three calls over the context's two buffer sets.
BACK_TO_BACK = [("rs_incorporate_reconstruction_device", 3), ("rs_add_views_device", 3), ("hm_knn_batch_device", EC.HM_STAGE_RING + 1),
                ("hm_match_batch_device", EC.HM_STAGE_RING + 1), ("akz_extract_batch_device", 3)]


@pytest.mark.parametrize("name,n", BACK_TO_BACK, ids=[b[0] for b in BACK_TO_BACK])
def test_calls_back_to_back_behind_one_busy_producer_each_give_their_own_settled_bytes(gpu, delay, context, name, n):
    """what one stalled call leaves in the context's scratch, its frame lists or its staging is nothing to the next: every call
    has inputs of its own seed and outputs of its own, and each equals its own settled answer"""
    row = EC.BY_NAME[name]
    ctx = context(row.family)
    calls = [(row.build(1 + k), row.build(102 + k)) for k in range(n)]
    wants = [settle(gpu, ctx, row, true, decoy) for true, decoy in calls]
    assert all(EC.differs(wants[0], w) for w in wants[1:]), "the calls give the same outputs: a mix-up could not show"
    gots, early = EC.raced(gpu, ctx, calls, delay)
    print("ENQUEUE %s x %d back to back returned_early=%s" % (name, n, early))
    for k, (got, want) in enumerate(zip(gots, wants)):
        assert EC.differs(got, want) == [], k
