"""Host-side mirror of cv-sfm's choice of the frames a frame is compared with, device-resident, over
hm_find_frames_batch_device of include/akz.h.

  VSlamData::find_visually_similar_and_recent_frames   cv-sfm/src/lib.rs:597-668
  try_localize: the reconstructions by views found     cv-sfm/src/lib.rs:853-855
  callers: add_frame, try_localize_and_incorporate     cv-sfm/src/lib.rs:790-806, 926-939
  the defaults                                          cv-sfm/src/settings.rs:437-451

The frame table (hash, feed, position in the feed, reconstruction and view of every frame, in insertion order) lives on the
device; hm_hash_bag_device writes a batch's hashes straight into its tail, and the search for a whole batch of frames is one call
on the matcher's stream behind it (cv_amd/csrc/hm_place.hip).  Nothing returns to the host in between and there is no CPU
fallback.  The search is exact where the reference asks an approximate index; what stays outside is that index's own answer.
"""
from dataclasses import dataclass

import numpy as np

from . import _device, _lib
from ._device import call

VERDICTS = ("ok", "bad_index", "bad_table")
PLAN_VERDICTS = ("ok", "cut", "no_group", "find_refused", "bad_view", "no_room")
NONE = _lib.HM_PL_NONE


def params(**kw):
    """hm_place_params with the reference's defaults (num_similar 0, num_recent 32, recent_threshold 0, search_num 512) and
    `kw` on top."""
    return _lib.params(_lib.PlaceParams, "hm_place_params_default", **kw)


def room(prm):
    """hm_place_room: the longest chain of these parameters, the smallest row pitch of the outputs"""
    return int(_lib.lib().hm_place_room(prm))


@dataclass
class FoundFrames:
    """What an hm_find_frames_batch_device call wrote, on the device (its outputs by their names without d_); entries past a
    count are not written: they hold `fill`."""
    found: object          # [nq][room] int32: the chain, recent then similar (stored rows)
    views_out: object      # [nq][room] int32: the view keys, groups back to back in group order
    group_recon: object    # [nq][room] int32: the reconstruction of group g
    group_start: object    # [nq][room + 1] int32: group g's views are views_out[group_start[g]:group_start[g + 1]]
    free: object           # [nq][room] int32: the chain's frames without a view
    search: object         # [nq][search_num][2] int32 {row, distance}, or None
    counts: object         # [nq][HM_PL_COUNTS] int32 {n_recent, n_similar, n_searched, n_groups, n_free}
    verdict: object        # [nq] int32 (HM_PL_*)
    room: int
    fill: int


class FrameIndex:
    """The frame table on the device, with room for `capacity` frames of `hash_bytes`-byte hashes, and its row count.  It runs
    on a Matcher's context and stream, so that a search queues behind the hash_bag that filled its rows."""

    def __init__(self, torch, matcher, capacity, hash_bytes=512, device=0):
        if hash_bytes <= 0 or hash_bytes % 4 or hash_bytes > _lib.HM_PL_MAX_HASH_BYTES:
            raise ValueError("hash_bytes: a multiple of 4, at most HM_PL_MAX_HASH_BYTES")
        self.torch, self.matcher = torch, matcher
        self.dev = torch.device("cuda", device)
        self.capacity, self.hash_bytes, self.n = int(capacity), int(hash_bytes), 0
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=self.dev)
        self.hashes = z((max(self.capacity, 1), hash_bytes), torch.uint8)
        self.feed, self.pos, self.view = (z((max(self.capacity, 1),), torch.int32) for _ in range(3))
        self.recon = torch.full((max(self.capacity, 1),), -1, dtype=torch.int32, device=self.dev)

    def _words(self, a):
        if isinstance(a, self.torch.Tensor):
            _device.require_device(a, itemsize=4)
            return a.view(self.torch.int32).reshape(-1)
        return self.torch.from_numpy(np.ascontiguousarray(a, np.uint32).reshape(-1).view(np.int32)).to(self.dev)

    def append_rows(self, feed, pos, hashes=None):
        """Frames appended in insertion order: feed / pos [k] (numpy arrays or device tensors of 4-byte words); their frames have
        no view yet.  -> the tail slice [k][hash_bytes] of the hash table: the d_hash that hm_hash_bag_device writes into (or
        `hashes` [k][hash_bytes] uint8 copied there).  The copies run on the current torch stream: name it as stream_to_wait."""
        feed, pos = self._words(feed), self._words(pos)
        k = int(feed.numel())
        if pos.numel() != k or self.n + k > self.capacity:
            raise ValueError("feed and pos of one length, inside the capacity")
        rows = slice(self.n, self.n + k)
        self.feed[rows] = feed
        self.pos[rows] = pos
        self.recon[rows] = -1
        self.n += k
        tail = self.hashes[rows]
        if hashes is not None:
            tail.copy_(hashes if isinstance(hashes, self.torch.Tensor) else
                       self.torch.from_numpy(np.ascontiguousarray(hashes, np.uint8).reshape(k, self.hash_bytes)))
        return tail

    def set_views(self, rows, recon, view):
        """Frame::view of the stored `rows`: their reconstruction keys (NONE: no view) and view keys (blocks)."""
        rows = self.torch.as_tensor(np.ascontiguousarray(rows, np.int64), device=self.dev)
        if rows.numel() and (int(rows.max()) >= self.n or int(rows.min()) < 0):
            raise ValueError("stored rows only")
        self.recon[rows] = self._words(recon)
        self.view[rows] = self._words(view)

    def remap_views(self, recon, block_map, flags=None, stream_to_wait=None):
        """hm_place_remap_views_device, in place, behind a repack of reconstruction `recon`: the view of every stored frame of
        it goes through block_map [n_blocks] (a numpy array or a device tensor of 4-byte words; 0xFFFFFFFF: the view is
        removed, the frame loses its view — remove_view's frame.view = None).  Enqueued on the matcher's stream behind the
        current torch stream (or stream_to_wait); no wait -> flags [1] int32 on the device: 1 iff a frame of `recon` names a
        view >= n_blocks (its row is untouched)."""
        m = self._words(block_map)
        if flags is None:
            flags = self.torch.zeros(1, dtype=self.torch.int32, device=self.dev)
        call("hm_place_remap_views_device", self.matcher.handle, self.recon, self.view, self.n, int(recon), m, int(m.numel()), flags,
             _device.wait_or_current(self.torch, stream_to_wait, self.dev))
        return _device.keep_alive(flags, m, self)

    def find_device(self, d_query, d_visible, nq, prm, row_pitch, d_found, d_views_out, d_group_recon, d_group_start, d_free, d_search, d_counts,
                    d_verdict, stream_to_wait=None, n_stored=None):
        """hm_find_frames_batch_device over the table's first n_stored rows (default: all): d_* and stream_to_wait as
        _device.arg / wait take them.  Enqueues and returns."""
        call("hm_find_frames_batch_device", self.matcher.handle, self.hashes, self.feed, self.pos, self.recon, self.view,
             self.n if n_stored is None else n_stored, self.hash_bytes, d_query, d_visible, nq, prm, row_pitch, d_found, d_views_out, d_group_recon,
             d_group_start, d_free, d_search, d_counts, d_verdict, _device.wait(stream_to_wait))

    def find(self, query_rows, prm=None, visible=None, stream_to_wait=None, search=False, row_pitch=None, fill=-1):
        """The frames every query is compared with.  query_rows [nq]: stored rows (a numpy array or a device tensor); visible
        [nq] or None: query q sees the rows below visible[q] (add_frame's sequence: query + 1; None: all).  search: also return
        the search lists.  Enqueued on the matcher's stream behind the current torch stream (or stream_to_wait); no wait ->
        FoundFrames, its tensors filled with `fill` where the call does not write."""
        torch = self.torch
        prm = prm or params()
        q = self._words(query_rows)
        nq = int(q.numel())
        vis = None if visible is None else self._words(visible)
        if vis is not None and vis.numel() != nq:
            raise ValueError("one visible count per query")
        R = room(prm) if row_pitch is None else int(row_pitch)
        f = lambda *shape: torch.full(shape, fill, dtype=torch.int32, device=self.dev)
        o = FoundFrames(f(nq, max(R, 1)), f(nq, max(R, 1)), f(nq, max(R, 1)), f(nq, R + 1), f(nq, max(R, 1)),
                        f(nq, max(prm.search_num, 1), 2) if search else None, f(nq, _lib.HM_PL_COUNTS), f(nq), R, fill)
        if nq == 0:
            return o
        self.find_device(q, vis, nq, prm, R, o.found, o.views_out, o.group_recon, o.group_start, o.free, o.search, o.counts, o.verdict,
                         _device.wait_or_current(torch, stream_to_wait, self.dev))
        if R == 0:      # (rows of pitch 0: the call still took an address for each)
            o.found, o.views_out, o.group_recon, o.free = (t[:, :0] for t in (o.found, o.views_out, o.group_recon, o.free))
        return _device.keep_alive(o, q, vis, self)


@dataclass
class ViewPlan:
    """What an hm_view_plan_device call wrote, on the device: the views every frame is matched against, for
    hm_knn_planned_batch_device and hm_best_of_views_planned_batch_device (Registration.match_found)."""
    view_idx: object       # [F][V] int32: the frame's list, NONE at and behind its length
    n_views: object        # [F] int32: the length
    verdict: object        # [F] int32 (HM_VP_*)
    counts: object         # [HM_VP_COUNTS] int32 {distinct target blocks, live problems, the call's verdict, frames with a view}
    V: int
    n_blocks: int
    exp_blocks: int


def plan_views(found, V, n_blocks, pick=None, by_recon=False, exp_blocks=None, matcher=None, stream_to_wait=None):
    """hm_view_plan_device over a FoundFrames (FrameIndex.find): every frame takes the views of ONE of its groups — group 0, the
    reconstruction with most views found (try_localize's first turn, cv-sfm/src/lib.rs:858); pick [F] ordinals: the pick[f]-th
    turn; by_recon: pick [F] reconstruction keys (.remove(&reconstruction), :936) — the first min(V, length) of them.  n_blocks:
    the blocks of the descriptor table (a view key is a block); exp_blocks: the room for distinct target blocks (default: as
    many as there can be).  Enqueued on the matcher's stream, where the find is, behind the current torch stream (or
    stream_to_wait), which fills the outputs; no wait -> ViewPlan."""
    import torch
    dev = found.verdict.device
    F, V, n_blocks = int(found.verdict.shape[0]), int(V), int(n_blocks)
    if exp_blocks is None:
        exp_blocks = max(1, min(F * V, n_blocks, 65535 - F))
    f = lambda *shape: torch.full(shape, -1, dtype=torch.int32, device=dev)
    plan = ViewPlan(f(F, V), torch.zeros(F, dtype=torch.int32, device=dev), f(F), torch.zeros(_lib.HM_VP_COUNTS, dtype=torch.int32, device=dev),
                    V, n_blocks, int(exp_blocks))
    d_pick = None
    if pick is not None:
        d_pick = pick if isinstance(pick, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(pick, np.uint32).view(np.int32)).to(dev)
        _device.require_device(d_pick, itemsize=4)
        if d_pick.numel() != F:
            raise ValueError("one pick per frame")
    elif by_recon:
        raise ValueError("by_recon names the reconstructions in pick")
    if F == 0:
        return plan
    if found.room == 0:
        raise ValueError("a find of room 0 holds no views")
    if matcher is None:         # the index the find ran on keeps itself alive behind its result
        matcher = next(m for m in getattr(found, "_inputs", ()) if isinstance(m, FrameIndex)).matcher
    call("hm_view_plan_device", matcher.handle, found.views_out, found.group_recon, found.group_start, found.counts, found.verdict, found.room,
         d_pick, _lib.HM_VP_PICK_RECON if by_recon else 0, F, V, n_blocks, plan.exp_blocks, plan.view_idx, plan.n_views, plan.verdict, plan.counts,
         _device.wait_or_current(torch, stream_to_wait, dev))
    return _device.keep_alive(plan, found, d_pick)


def view_blocks(result, V, pad=None):
    """The host `view_blocks` [nq][V] of Registration.match_views from a FoundFrames whose stream has been waited for: the first
    V view keys of every query in group order, the one small copy (nq x V words) of the chain.  A query with fewer views found
    repeats its last one (`pad`: that block instead; a query with none needs it)."""
    n = result.group_start.shape[0]
    V = int(V)
    take = min(V, result.room)
    views = _device.host_u32(result.views_out[:, :take].contiguous()).reshape(n, take)
    counts = _device.host_u32(result.counts).reshape(n, _lib.HM_PL_COUNTS)
    out = np.zeros((n, V), np.uint32)
    for q in range(n):
        have = min(int(counts[q, _lib.HM_PL_C_RECENT] + counts[q, _lib.HM_PL_C_SIMILAR] - counts[q, _lib.HM_PL_C_FREE]), V)
        if have == 0 and pad is None:
            raise ValueError(f"query {q} found no view and there is no pad block")
        out[q, :have] = views[q, :have]
        out[q, have:] = views[q, have - 1] if pad is None else pad
    return out
