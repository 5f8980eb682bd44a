"""Host-side mirror of the landmark bookkeeping cv-sfm keeps around the registration of a frame, over
rs_landmarks_sharing_view_device and rs_add_views_device of include/akz.h.

  VSlam::are_landmarks_sharing_view          cv-sfm/src/lib.rs:1435-1449
  VSlamData::add_view / add_landmark         cv-sfm/src/lib.rs:432-500
  VSlamData::merge_landmarks                 cv-sfm/src/lib.rs:699-721

Both run on the device (cv_amd/csrc/rs_landmark_table.hip); there is no CPU fallback.  The mask goes to
Registration.triangulate_merged / consensus as d_merge_ok; the next generation of the table — CSR lists, the per-feature
landmark map hm_best_of_views_batch_device reads, the row lengths hm_landmark_matches_ordered_batch_device sorts by and the
poses of the new views — stays on the device, so that a micro-batch goes from pixels to the next world table without a host
step: add_views_and_regenerate below chains the stages with one wait.  The one rule that is not the reference's (two frames
of a call that name one landmark) is in DESIGN.md §7.
"""
from dataclasses import dataclass

import numpy as np

from . import _device, _lib
from ._device import call, host_u32 as u32
from .triangulation import LandmarkTable

VERDICTS = ("ok", "not_accepted", "bad_index", "bad_table")


@dataclass
class AddViewsTensors:
    """What an rs_add_views_device call wrote, on the device (its outputs by their names without d_)."""
    obs_start_out: object    # [lm_room + 1] int32
    obs_out: object          # [obs_room][2] int32, rows [0, counts_out[1]) written
    counts_out: object       # [RS_AV_COUNTS] int32 {rows filled, observations filled, merges applied, merges demoted}
    landmarks_out: object    # [n_blocks][cap] int32: the landmark of every feature, -1 (0xFFFFFFFF) for none
    obs_counts_out: object   # [lm_room] int32: the row lengths
    frame_verdict: object    # [n_frames] int32 (RS_AV_*)
    stats: object            # [n_frames][RS_AV_STATS] int32
    call_verdict: object     # [1] int32: RS_AV_OK or RS_AV_BAD_TABLE
    poses: object            # [n_blocks][12] float64, the caller's tensor, updated in place
    lm_room: int
    obs_room: int
    n_frames: int

    def table(self, torch, counts=None):
        """The new table as a LandmarkTable over these tensors.  Without `counts` nothing is waited for: the table has lm_room
        rows and room for obs_room observations, the rows behind the filled ones are empty lists (RS_TRI_TOO_FEW for the
        triangulation, RS_OF_SINGLE for the filter).  counts = (rows, observations) as a caller that has waited read them from
        counts_out: the table of exactly the filled rows — the same bytes on those."""
        n_lm, n_obs = (self.lm_room, self.obs_room) if counts is None else (int(counts[0]), int(counts[1]))
        return LandmarkTable.from_device(torch, self.obs_start_out, self.obs_out, n_lm, n_obs, d_obs_counts=self.obs_counts_out)


@dataclass
class AddViewsResult:
    obs_start: np.ndarray      # [rows + 1] the new table, filled rows only
    obs: np.ndarray            # [observations][2]
    counts: np.ndarray         # [RS_AV_COUNTS] u32
    landmarks: np.ndarray      # [n_blocks][cap] u32
    obs_counts: np.ndarray     # [rows] u32
    frame_verdicts: np.ndarray  # [n_frames] u32
    stats: np.ndarray          # [n_frames][RS_AV_STATS] u32
    call_verdict: int
    tensors: object            # the AddViewsTensors it was read from


class LandmarkUpdate:
    """The landmark bookkeeping on the context (and stream) of an EssentialConsensus, so that it queues behind that object's
    other calls."""

    def __init__(self, consensus):
        self._cons = consensus

    def sharing_view_device(self, d_obs_start, d_obs, n_obs, n_landmarks, d_best, d_decision, cap, n_frames, d_merge_ok, stream_to_wait=None):
        """rs_landmarks_sharing_view_device: d_* and stream_to_wait as _device.arg / wait take them.  Enqueues and returns."""
        call("rs_landmarks_sharing_view_device", self._cons._h, d_obs_start, d_obs, n_obs, n_landmarks, d_best, d_decision, cap, n_frames,
             d_merge_ok, _device.wait(stream_to_wait))

    def add_views_device(self, d_obs_start, d_obs, n_obs, n_landmarks, n_world, d_split, d_split_count, split_room, cap, n_blocks, ik, d_counts,
                         d_matches, d_nmatches, d_final, d_verdict, d_pose_out, d_best, d_skip, obs_room, lm_room, d_poses, d_obs_start_out,
                         d_obs_out, d_counts_out, d_landmarks_out, d_obs_counts_out, d_frame_verdict, d_stats, d_call_verdict,
                         stream_to_wait=None):
        """rs_add_views_device: d_* and stream_to_wait as _device.arg / wait take them, ik a sequence of blocks.  Enqueues and returns."""
        blocks, n = _device.index_list(ik)
        call("rs_add_views_device", self._cons._h, d_obs_start, d_obs, n_obs, n_landmarks, n_world, d_split, d_split_count, split_room,
             cap, n_blocks, blocks, n, d_counts, d_matches, d_nmatches, d_final, d_verdict, d_pose_out, d_best, d_skip, obs_room, lm_room,
             d_poses, d_obs_start_out, d_obs_out, d_counts_out, d_landmarks_out, d_obs_counts_out, d_frame_verdict, d_stats,
             d_call_verdict, _device.wait(stream_to_wait))

    def sharing_view_tensors(self, torch, table, best, decision, out=None, stream_to_wait=None):
        """The mask of the merge candidates over `table` (a LandmarkTable): best [F][cap][3][2] and decision [F][cap] as
        hm_best_of_views_batch_device leaves them (numpy arrays or 4-byte device tensors).  Enqueued behind the current torch
        stream (or stream_to_wait); no wait -> d_merge_ok [F][cap] uint8 on the device."""
        dev = table.dev
        F, cap = int(decision.shape[0]), int(decision.shape[1])
        d_best, d_decision = _device.tensor(torch, best, np.uint32, dev), _device.tensor(torch, decision, np.uint32, dev)
        if out is None:
            out = torch.zeros((max(F, 1), cap), dtype=torch.uint8, device=dev)
        self.sharing_view_device(table.d_start, table.d_obs, table.n_obs, table.n_landmarks, d_best, d_decision, cap, F, out,
                                 _device.wait_or_current(torch, stream_to_wait, dev))
        # the caller gets a bare tensor back: the consensus holds what was uploaded for this call
        _device.keep_alive(self._cons, *(d for d, a in ((d_best, best), (d_decision, decision)) if d is not a))
        return out

    def add_views_tensors(self, torch, table, d_poses, cap, frame_blocks, counts, matches, nmatches, final, verdict, pose_out, best=None,
                          skip=None, split=None, split_count=None, split_room=None, n_world=None, obs_room=None, lm_room=None,
                          stream_to_wait=None):
        """add_view for the frames in `frame_blocks` over `table` (a LandmarkTable).  d_poses [n_blocks][12] float64 device
        tensor, updated in place; counts [n_blocks], matches [F][cap][2], nmatches [F], final [F][cap] uint8, verdict [F],
        pose_out [F][12] float64, best [F][cap][3][2] (optional), skip [F] (optional): numpy arrays or device tensors, as
        Registration.refine() leaves them.  split [split_room][2] / split_count [1]: the split list of the filter that wrote
        `table` (ObservationFilterTensors.split_out and counts[1:2]).  The rooms default to the least the call accepts.
        Enqueued behind the current torch stream (or stream_to_wait); no wait -> AddViewsTensors."""
        dev = table.dev
        F = len(frame_blocks)
        n_blocks = int(d_poses.shape[0])
        t = lambda a, dt: None if a is None else _device.tensor(torch, a, dt, dev)
        ins = [t(counts, np.uint32), t(matches, np.uint32), t(nmatches, np.uint32), t(final, np.uint8), t(verdict, np.uint32),
               t(pose_out, np.float64), t(best, np.uint32), t(skip, np.uint32), t(split, np.uint32), t(split_count, np.uint32)]
        if split is None:
            split_room = 0
        elif split_room is None:
            split_room = int(np.prod(split.shape)) // 2
        grow = split_room + F * cap
        obs_room = table.n_obs + grow if obs_room is None else obs_room
        lm_room = table.n_landmarks + grow if lm_room is None else lm_room
        z32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)
        o = AddViewsTensors(z32(lm_room + 1), z32(max(obs_room, 1), 2), z32(_lib.RS_AV_COUNTS), z32(n_blocks, cap), z32(max(lm_room, 1)),
                            z32(max(F, 1)), z32(max(F, 1), _lib.RS_AV_STATS), z32(1), d_poses, lm_room, obs_room, F)
        self.add_views_device(table.d_start, table.d_obs, table.n_obs, table.n_landmarks, table.n_landmarks if n_world is None else n_world,
                              ins[8], ins[9], split_room, cap, n_blocks, frame_blocks, *ins[:8], obs_room, lm_room, d_poses, o.obs_start_out,
                              o.obs_out, o.counts_out, o.landmarks_out, o.obs_counts_out, o.frame_verdict, o.stats, o.call_verdict,
                              _device.wait_or_current(torch, stream_to_wait, dev))
        return _device.keep_alive(o, ins, table)

    def run_sharing_view(self, torch, table, best, decision):
        """sharing_view_tensors, then WAITS and copies to the host -> mask [F][cap] uint8."""
        out = self.sharing_view_tensors(torch, table, best, decision)
        self._cons.sync()
        return out.cpu().numpy()[:int(decision.shape[0])]

    def run_add_views(self, torch, table, d_poses, cap, frame_blocks, *args, **kw):
        """add_views_tensors, then WAITS and copies to the host -> AddViewsResult."""
        o = self.add_views_tensors(torch, table, d_poses, cap, frame_blocks, *args, **kw)
        self._cons.sync()
        return to_host(o)


def to_host(o):
    """An AddViewsTensors whose stream has been waited for -> AddViewsResult."""
    counts = u32(o.counts_out)
    rows, n = int(counts[0]), int(counts[1])
    return AddViewsResult(u32(o.obs_start_out)[:rows + 1], u32(o.obs_out)[:n], counts, u32(o.landmarks_out), u32(o.obs_counts_out)[:rows],
                          u32(o.frame_verdict)[:o.n_frames], u32(o.stats)[:o.n_frames], int(u32(o.call_verdict)[0]), o)


def add_views_and_regenerate(torch, registration, table, d_kps, d_poses, graph_start, d_split=None, d_split_count=None, skip=None, **kw):
    """What VSlam::add_frame does behind a successful registration (cv-sfm/src/lib.rs:680-693: add_view, then
    regenerate_reconstruction), for the frames of registration.refine(), with ONE wait at the end: add_views on the table the
    refinement read -> the new table with (lm_room, obs_room) as its sizes, so that nothing is read back -> the robust
    triangulation of its rows -> reconstruction.regenerate (covisibility, constraints, record, pose graph, filter, world table).
    The table holds one reconstruction: recon_start = [0, lm_room]; graph_start [2] = [0, views of it].  d_poses [blocks][12] is
    updated by add_views and relaxed in place.  kw: regenerate's parameter arguments.  -> (AddViewsTensors, RegenerateResult);
    the next match_views() takes landmarks_out, the next consensus obs_counts_out and the result's world table."""
    from .reconstruction import regenerate
    added = registration.add_views(table, d_poses, d_split, d_split_count, skip)
    new_table = added.table(torch)
    with torch.cuda.stream(registration._rs_s):          # regenerate orders itself behind the current torch stream
        result = regenerate(torch, registration.cons, new_table, d_kps, registration.cap, registration.cam, d_poses, graph_start,
                            np.array([0, added.lm_room], np.uint32), **kw)
    return added, result
