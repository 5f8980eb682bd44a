"""The chain of statements of tests/searched_life_statement.py — the reconstruction's life with the matcher in the loop — against
the world it is fed.  On every scene and seed it stays inside the figures BOUNDS was measured as (a quarter of what the device is
held to), inside the caps of the designed life and keeps the table invariants after every phase.  In the exact worlds the searched
tables are held to the truth in integers: every bootstrap pair is right and none is missing, every decision-1 match names a
landmark of the feature's own point, every applied merge joins two landmarks of one point and leaves one row alive, at least
twelve candidates are admitted in a side's first call and reach the consensus with a world point, at least eight merges are
applied and at least one is demoted per side.  "No point has two live landmarks that a merge candidate named" is asserted for the
merges the batch rule APPLIES: a demoted merge leaves both rows alive by that rule, so the two conditions
cannot both hold for it.  The noisy worlds print the same counts.

Then the four alterations of the new glue, each on an exact world.  Two of them (the map one generation old, view_sel permuted
against the knn problems) lose the frames and are seen by the metric, over the views the phase must have.  The other two (a merged
row at n_world + j * cap + f, the mask of the batch's other frame) do NOT move a pose: a merge candidate without a world point
stays out of the consensus but still passes the consistency filter, and a dropped candidate only becomes a landmark of its own.
They are seen by the integer conditions alone — which is why the device test holds those too.

No GPU.  One world's chain takes about 65 s on one core (the merged graph of 13 views is most of it), the four worlds 4.5 min
and the alterations half a minute more; every world is run once per session and shared."""
import functools

import numpy as np
import pytest

import reconstruction_life_statement as L
import searched_life_statement as S

WORLDS = [(scene, seed) for scene in S.SCENES for seed in S.SEEDS[scene]]
SIDES = (("A", L.A_START, L.A_GROW, L.A_VIEWS), ("B", L.B_START, L.B_GROW, L.B_VIEWS))
count = lambda c: {k: (v if isinstance(v, int) else len(v)) for k, v in c.items()}


@functools.lru_cache(maxsize=None)
def states(scene, seed):
    w = S.searched_world(seed, *S.SCENES[scene])
    return w, S.life(w)


@functools.lru_cache(maxsize=None)
def chain(scene, seed):
    return S.errors_of(*states(scene, seed))


def test_the_searched_world_leaves_the_designed_world_as_it_was():
    """the 216 points, their pixels, the views and the designed lists are world()'s own; the descriptors' pad bits are clear"""
    for scene, seed in WORLDS:
        w0, w = L.world(seed, *S.SCENES[scene]), S.searched_world(seed, *S.SCENES[scene])
        assert np.array_equal(w.points[:w0.n_points], w0.points) and np.array_equal(w.poses, w0.poses) and w.seen[:w0.n_points] == w0.seen
        for v in range(L.N_VIEWS):
            assert np.array_equal(w.px[v, :w0.counts[v]], w0.px[v, :w0.counts[v]]) and np.array_equal(w.point_of[v, :w0.counts[v]], w0.point_of[v, :w0.counts[v]])
        assert not (w.descs[:, :, 60] & 0xC0).any() and not w.descs[:, :, 61:].any()
        assert all(L.A_START[0] not in s and L.B_START[0] not in s for s in w.seen[w0.n_points:])
        assert sum(L.BRIDGE in s for s in w.seen[w0.n_points:]) == 2 * (S.LATE // 4)


@pytest.mark.parametrize("scene, seed", WORLDS)
def test_the_searched_chain_stays_inside_bounds_caps_and_invariants(scene, seed):
    for (side, phase), e in chain(scene, seed).items():
        print(scene, seed, side, phase, {k: "%.3e" % e[k] for k in ("rotation", "centre", "point", "left_out")})
        assert e["broken"] == [], (side, phase)
        assert e["views"] == S.VIEWS_AFTER.get(phase, L.N_VIEWS), (side, phase)
        if phase == "merge":
            assert e["shared"][2] == 0 and e["shared"][0] >= L.SHARED_MERGED_AT_LEAST[scene], e["shared"]
        if phase == "export":
            assert e["wrong_colours"] == 0
        assert e["left_out"] <= L.LEFT_OUT_CAP[scene], (side, phase, e["left_out"])
        for kind, measured in S.BOUNDS[scene][phase].items():
            assert e[kind] <= measured, (side, phase, kind, e[kind])


def test_searched_bounds_hold_what_was_measured():
    """every entry of BOUNDS is reached (to its rounding up, at most 0.25 %) by some seed and side: a measurement, not a choice"""
    for scene in S.SCENES:
        for phase in S.PHASES:
            for kind, measured in S.BOUNDS[scene][phase].items():
                worst = max(e[kind] for seed in S.SEEDS[scene] for (_, p), e in chain(scene, seed).items() if p == phase)
                assert 0.997 * measured <= worst <= measured, (scene, phase, kind, worst)


@pytest.mark.parametrize("scene, seed", WORLDS)
def test_the_searched_tables_against_the_truth(scene, seed):
    w, st = states(scene, seed)
    for side, triple, _, _ in SIDES:
        pairs, npairs = st[side, "start"].lists
        wrong, missing = S.wrong_pairs(w, triple, pairs, npairs)
        first, second = S.conditions(w, st[side, "grow1"].call), S.conditions(w, st[side, "grow"].call)
        bridge = S.conditions(w, st[side, "bridge"].call)
        print(scene, seed, side, "pairs", npairs.tolist(), "wrong", wrong, "missing", missing, "\n  first call", count(first), "\n  second call",
              count(second), "\n  bridging frame", count(bridge), "\n  map entries that differ from the filtered rows' map:",
              [S.handover_difference(st[side, p]) for p in ("start", "grow1", "grow")])
        assert not first["stray_mask"] and not second["stray_mask"] and not bridge["stray_mask"]
        if scene == "exact":
            assert (wrong, missing) == (0, 0)
            assert S.exact_side(first, second, bridge) == []


def caught(w, view_range, first, second, bridge=None):
    """an invariant broken, an error at least ten times its bound over the views the phase must have (a bound is four times
    BOUNDS' entry; a frame that was refused has no pose), or an exact-world condition that does not hold"""
    lo, hi = view_range
    seen = []
    for phase, st, vr in (("grow1", first, (lo, lo + 4)), ("grow", second, view_range), ("bridge", bridge, L.B_WITH_BRIDGE)):
        if st is None:
            continue
        e = L.aligned_errors(st.poses, st.world, st.reason, L.truth_of(w, st.rows, list(range(*vr))))
        broken = L.invariants(st.table_rows, vr, st.table_map, st.tombstones) + L.invariants(st.rows, vr)
        ratios = {k: e[k] / (4 * S.BOUNDS["exact"][phase][k]) for k in ("rotation", "centre", "point")}
        print(phase, {k: "%.3g x" % v for k, v in ratios.items()}, "left out %.2f" % e["left_out"], broken[:2])
        seen += broken + [k for k, v in ratios.items() if v >= 10.0]
    failed = S.exact_side(S.conditions(w, first.call), S.conditions(w, second.call), bridge and S.conditions(w, bridge.call))
    print("conditions", failed)
    return seen, failed


@pytest.mark.parametrize("name", S.SEARCH_ALTERATIONS)
def test_an_altered_glue_of_the_search_is_caught(name):
    """on side B of an exact world, whose bridging frame is registered with the regeneration behind it"""
    seed = S.SEEDS["exact"][0]
    w, st = states("exact", seed)
    side, triple, frames, view_range = SIDES[1]
    lo = view_range[0]
    first = S.register(w, st[side, "start"], frames[:1], list(triple), (lo, lo + 4), alter=(name,))
    second = S.register(w, first, frames[1:], list(triple) + list(frames[:1]), view_range, alter=(name,))
    bridge = None
    if len(second.views) == S.VIEWS_AFTER["grow"]:                # (a side that lost a frame is caught already)
        bridge = S.register(w, L.normalize(w, second, view_range), [L.BRIDGE], list(range(*view_range)), L.B_WITH_BRIDGE, alter=(name,))
    seen, failed = caught(w, view_range, first, second, bridge)
    assert seen or failed
    if name in ("map_one_generation_old", "view_sel_permuted"):
        assert seen                                               # the metric itself sees these
    else:
        assert not seen and failed                                # documented above: the integer conditions alone see these


def test_the_unaltered_glue_is_not_caught():
    seed = S.SEEDS["exact"][0]
    w, st = states("exact", seed)
    assert caught(w, L.B_VIEWS, st["B", "grow1"], st["B", "grow"], st["B", "bridge"]) == ([], [])
