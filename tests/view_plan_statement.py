"""Which views a new frame is matched against, given the frames found for it: in plain Python, written from the reference's
text, on the lists place_statement.find_one returns; and a catalogue of designed calls.

Nothing here imports the product (cv_amd), the C oracle (oracle/) or ctypes.  What is stated:

  try_localize (cv-sfm/src/lib.rs:853-891) sorts the found reconstructions by views found, most first, and hands
  incorporate_frame the views of ONE reconstruction per turn of its loop: `pick` as an ordinal is the turn (None: the first).
  try_localize_and_incorporate (:926-939) takes the group of one named reconstruction out of the map with
  `.remove(&reconstruction)`: `pick` as a key.  register_frame_subset (:1472-1486) walks exactly the list it is given; the
  project's departure is take(V), the first V views of the list, reported as CUT.

  A view key is a block of the descriptor table.  A frame whose find was refused has no list (FIND_REFUSED); a frame without
  that group has none (NO_GROUP); a frame one of whose taken keys is no block has none (BAD_VIEW).  The call searches the
  distinct blocks of all lists, in ascending order; more of them than exp_blocks refuse the call (NO_ROOM): no frame keeps a
  list.
"""
import numpy as np

import place_statement as P

NONE = 0xFFFFFFFF
OK, CUT, NO_GROUP, FIND_REFUSED, BAD_VIEW, NO_ROOM = range(6)
C_BLOCKS, C_LIVE, C_VERDICT, C_FRAMES, COUNTS = range(5)
PICK_RECON = 1
MAX_VIEWS = 64


# ------------------------------------------------------------------------------------------------ the statement
def plan_one(found, pick, by_recon, V, n_blocks):
    """found: a find_one result.  -> (views, verdict)"""
    if found["verdict"] != P.OK:
        return [], FIND_REFUSED
    reconstruction_frames = found["groups"]                      # sorted by Reverse(len) (:853-855)
    if by_recon:
        views = dict(reconstruction_frames).pop(pick, None)      # .remove(&reconstruction) (:936)
    else:
        turn = 0 if pick is None else pick                       # the turn of `for (reconstruction, views) in ...` (:858)
        views = reconstruction_frames[turn][1] if turn < len(reconstruction_frames) else None
    if views is None:
        return [], NO_GROUP
    taken = list(views[:V])                                      # take(V)
    if any(view >= n_blocks for view in taken):
        return [], BAD_VIEW
    return taken, CUT if len(views) > V else OK


def plan(founds, picks, by_recon, V, n_blocks, exp_blocks):
    """-> dict(lists, verdicts, blocks = the ascending distinct target blocks of the lists as taken, call = OK / NO_ROOM)"""
    lists, verdicts = [], []
    for f, found in enumerate(founds):
        views, verdict = plan_one(found, None if picks is None else int(picks[f]), by_recon, V, n_blocks)
        lists.append(views)
        verdicts.append(verdict)
    blocks = sorted({view for views in lists for view in views})
    call = NO_ROOM if len(blocks) > exp_blocks else OK
    if call != OK:
        lists = [[] for _ in lists]
    return dict(lists=lists, verdicts=verdicts, blocks=blocks, call=call)


def founds_of(c):
    """the find_one results of a case's place call"""
    t, q, vis = c["table"], c["queries"], c["visible"]
    n = len(t["feed"])
    return [P.find_one(t, int(q[k]), n if vis is None else int(vis[k]), c["params"]) for k in range(len(q))]


def outputs(c, fill=NONE):
    """The arrays hm_view_plan_device leaves (uint32), `fill` wherever the call does not write (it writes every word)."""
    F, V = len(c["queries"]), c["V"]
    r = plan(founds_of(c), c["pick"], c["by_recon"], V, c["n_blocks"], c["exp_blocks"])
    o = dict(view_idx=np.full((F, V), fill, np.uint32), n_views=np.full(F, fill, np.uint32), verdict=np.full(F, fill, np.uint32),
             counts=np.full(COUNTS, fill, np.uint32))
    for f, views in enumerate(r["lists"]):
        o["view_idx"][f] = NONE
        o["view_idx"][f, :len(views)] = views
        o["n_views"][f] = len(views)
        o["verdict"][f] = r["verdicts"][f]
    o["counts"][:] = [len(r["blocks"]), sum(len(v) for v in r["lists"]), r["call"], sum(1 for v in r["lists"] if v)]
    return o


# ------------------------------------------------------------------------------------------------ the catalogue
def case(place, V, n_blocks, exp_blocks=None, pick=None, by_recon=False):
    """a place_statement case (table, queries, visible, params) and the plan call's own arguments"""
    F = len(place["queries"])
    return dict(place, V=V, n_blocks=n_blocks, exp_blocks=max(1, min(F * V, n_blocks)) if exp_blocks is None else exp_blocks,
                pick=None if pick is None else np.ascontiguousarray(pick, np.uint32), by_recon=by_recon)


def designed(frames, hash_bytes=8):
    """Frame f's chain is exactly frames[f], a list of (reconstruction, view): feed f holds one stored frame per entry, in chain
    order, and the query behind them; the window takes in the whole feed and nothing is searched for."""
    feed, pos, recon, view, queries = [], [], [], [], []
    for f, chain in enumerate(frames):
        for k, (rc, vw) in enumerate(chain):
            feed.append(f); pos.append(k); recon.append(rc); view.append(vw)
        queries.append(len(feed))
        feed.append(f); pos.append(len(chain)); recon.append(NONE); view.append(0)
    n = len(feed)
    longest = max(len(chain) for chain in frames)
    hashes = P._rng(n, hash_bytes).integers(0, 256, (n, hash_bytes), dtype=np.uint8)
    return P.case(P.table(hashes, feed, pos, recon, view), queries, P.params(num_similar=0, num_recent=longest + 1, search_num=1))


def one_group(views, recon=4):
    return [(recon, v) for v in views]


def cases():
    """name -> case: the catalogue both builds are held to"""
    c = {}
    three = P.groups_case("three")                               # groups (5, 4 views), (9, 4), (30, 2); view keys 1000 + row
    c["three_first"] = case(three, 4, 1100)
    for turn in (0, 1, 2, 3):                                    # 3: a pick beyond n_groups
        c[f"three_turn_{turn}"] = case(three, 4, 1100, pick=[turn])
    for key in (5, 9, 30, 77):                                   # 77: a key no group has
        c[f"three_key_{key}"] = case(three, 4, 1100, pick=[key], by_recon=True)
    c["three_cut"] = case(three, 3, 1100)
    c["three_wide"] = case(three, 64, 1100)
    c["free"] = case(P.groups_case("free"), 4, 1100)             # the find has no groups
    c["own"] = case(P.groups_case("own"), 4, 1100, pick=[9], by_recon=True)
    c["refusals"] = case(P.refusal_case(), 3, 1100)              # find verdicts OK, BAD_INDEX, BAD_TABLE
    c["growing"] = case(P.growing_case(), 3, 1100)
    c["growing_second_turn"] = case(P.growing_case(), 2, 1100, pick=np.ones(80))
    c["growing_by_key"] = case(P.growing_case(), 5, 1100, pick=7 * (1 + np.arange(80) % 3), by_recon=True)
    V = 4
    c["lengths"] = case(designed([one_group(range(10, 10 + n)) for n in (V, V - 1, V + 1, 1)]), V, 64)
    c["last_block"] = case(designed([one_group([3, 39]), one_group([40, 3]), one_group([5]), one_group([2, 1, 40, 0]), one_group([2, 1, 0, 40])]), 3, 40)
    c["same_views"] = case(designed([one_group([8, 6, 7])] * 5), V, 40)
    five = [one_group([1, 2]), one_group([2, 3]), one_group([9, 1, 5])]              # distinct blocks 1 2 3 5 9
    c["room_exact"] = case(designed(five), V, 40, exp_blocks=5)
    c["room_short"] = case(designed(five), V, 40, exp_blocks=4)
    # k_vp_scan takes 1 024 flags a pass: distinct blocks on both sides of the pass's end, counted behind the carry
    c["scan_second_pass"] = case(designed([one_group([1023, 1024, 5]), one_group([1099, 1023]), one_group([1025])]), V, 1100)
    c["two_groups_each"] = case(designed([[(3, 1), (8, 2), (8, 4), (3, 6)], [(8, 5), (3, 7), (3, 9)], [(2, 11)]]), V, 40, pick=[8, 8, 8], by_recon=True)
    for F in (1, 63, 64, 65):
        rng = P._rng(F, 0x5650)
        frames = [one_group(rng.choice(50, 1 + int(rng.integers(0, 5)), replace=False)) for _ in range(F)]
        c[f"frames_{F}"] = case(designed(frames), V, 50)
    return c
