"""Host-side mirror of cv-sfm's loop closure between two reconstructions and of its normalisation, over rs_merge_map_device,
rs_incorporate_reconstruction_device and rs_normalize_reconstruction_device of include/akz.h.

  VSlam::try_merge_reconstructions (the map)   cv-sfm/src/lib.rs:2116-2193
  VSlam::incorporate_reconstruction            cv-sfm/src/lib.rs:1817-1887
  VSlam::normalize_reconstruction              cv-sfm/src/lib.rs:2241-2283

All three run on the device (cv_amd/csrc/rs_reconstruction_merge.hip); there is no CPU fallback.  The merged table — CSR lists,
the per-feature landmark map, the row lengths, the carried-over views' poses — stays on the device in rs_add_views_device's
shapes, so that the stages behind take it unchanged: reconstruction.merge_reconstructions chains the map, the incorporation,
the triangulation of the new table and regenerate with one wait.  The rules that are not the reference's (a map that is not
one-to-one, the order of a row, stable keys) are in DESIGN.md §7.
"""
from dataclasses import dataclass

import numpy as np

from . import _device, _lib
from ._device import call, host_u32 as u32
from .triangulation import LandmarkTable

VERDICTS = ("ok", "bad_table", "bad_index", "shared_block")
NORMALIZE_VERDICTS = ("ok", "not_normal", "bad_index")


@dataclass
class MergeMapTensors:
    """What an rs_merge_map_device call wrote, on the device."""
    map: object          # [cap][2] int32 {source landmark, destination landmark}, entries [0, map_count) written
    map_count: object    # [1] int32
    map_room: int


@dataclass
class IncorporateTensors:
    """What an rs_incorporate_reconstruction_device call wrote, on the device (its outputs by their names without d_)."""
    obs_start_out: object    # [lm_room + 1] int32
    obs_out: object          # [obs_room][2] int32, rows [0, counts_out[1]) written
    counts_out: object       # [RS_IR_COUNTS] int32 {rows, observations, entries applied, entries demoted, new rows, observations dropped}
    landmarks_out: object    # [n_blocks][cap] int32: the landmark of every feature, -1 (0xFFFFFFFF) for none
    obs_counts_out: object   # [lm_room] int32: the row lengths
    src_key_out: object      # [n_src_landmarks] int32: the destination key of every source landmark, -1 for none
    call_verdict: object     # [1] int32 (RS_IR_*)
    poses: object            # [n_blocks][12] float64, the caller's tensor, updated in place
    lm_room: int
    obs_room: int
    n_src_landmarks: int

    def table(self, torch, counts=None):
        """The merged table as a LandmarkTable over these tensors.  Without `counts` nothing is waited for: the table has lm_room
        rows and room for obs_room observations, the rows behind the filled ones are empty lists.  counts = (rows, observations)
        as a caller that has waited read them from counts_out: the table of exactly the filled rows — the same bytes on those."""
        n_lm, n_obs = (self.lm_room, self.obs_room) if counts is None else (int(counts[0]), int(counts[1]))
        return LandmarkTable.from_device(torch, self.obs_start_out, self.obs_out, n_lm, n_obs, d_obs_counts=self.obs_counts_out)


@dataclass
class IncorporateResult:
    obs_start: np.ndarray      # [rows + 1] the merged table, filled rows only
    obs: np.ndarray            # [observations][2]
    counts: np.ndarray         # [RS_IR_COUNTS] u32
    landmarks: np.ndarray      # [n_blocks][cap] u32
    obs_counts: np.ndarray     # [rows] u32
    src_key: np.ndarray        # [n_src_landmarks] u32
    call_verdict: int
    tensors: object            # the IncorporateTensors it was read from


@dataclass
class NormalizeTensors:
    """What an rs_normalize_reconstruction_device call wrote, on the device."""
    stats: object              # [2] float64 {mean distance, features it ran over}
    verdict: object            # [1] int32 (RS_NR_*)
    poses: object              # the caller's tensor, updated in place
    constraint_poses: object   # the caller's tensor (or None), updated in place


class ReconstructionMerge:
    """The merge of two reconstructions on the context (and stream) of an EssentialConsensus, so that it queues behind that
    object's other calls."""

    def __init__(self, consensus):
        self._cons = consensus

    def merge_map_device(self, d_matches, d_nmatches, d_final, d_best, n_world, n_dst_landmarks, cap, slot, d_counts, d_src_landmarks, n_blocks,
                         bridge_block, d_map, d_map_count, stream_to_wait=None):
        """rs_merge_map_device: d_* and stream_to_wait as _device.arg / wait take them.  Enqueues and returns."""
        call("rs_merge_map_device", self._cons._h, d_matches, d_nmatches, d_final, d_best, n_world, n_dst_landmarks, cap, slot, d_counts,
             d_src_landmarks, n_blocks, bridge_block, d_map, d_map_count, _device.wait(stream_to_wait))

    def incorporate_device(self, d_dst_start, d_dst_obs, n_dst_obs, n_dst_landmarks, d_src_start, d_src_obs, n_src_obs, n_src_landmarks, d_map,
                           d_map_count, map_room, cap, n_blocks, src_blocks, bridge_block, d_src_pose, d_skip, obs_room, lm_room, d_poses,
                           d_obs_start_out, d_obs_out, d_counts_out, d_landmarks_out, d_obs_counts_out, d_src_key_out, d_call_verdict,
                           stream_to_wait=None):
        """rs_incorporate_reconstruction_device: d_* and stream_to_wait as _device.arg / wait take them, src_blocks a sequence of
        blocks.  Enqueues and returns."""
        blocks, n = _device.index_list(src_blocks)
        call("rs_incorporate_reconstruction_device", self._cons._h, d_dst_start, d_dst_obs, n_dst_obs, n_dst_landmarks, d_src_start, d_src_obs,
             n_src_obs, n_src_landmarks, d_map, d_map_count, map_room, cap, n_blocks, blocks, n, bridge_block, d_src_pose, d_skip, obs_room,
             lm_room, d_poses, d_obs_start_out, d_obs_out, d_counts_out, d_landmarks_out, d_obs_counts_out, d_src_key_out, d_call_verdict,
             _device.wait(stream_to_wait))

    def normalize_device(self, view_blocks, d_counts, d_landmarks, cap, n_blocks, d_world, n_world, d_poses, d_constraint_poses, n_constraints,
                         d_stats, d_verdict, stream_to_wait=None):
        """rs_normalize_reconstruction_device: d_* and stream_to_wait as _device.arg / wait take them, view_blocks a sequence of
        blocks, the first the reference's first view.  Enqueues and returns."""
        blocks, n = _device.index_list(view_blocks)
        call("rs_normalize_reconstruction_device", self._cons._h, blocks, n, d_counts, d_landmarks, cap, n_blocks, d_world, n_world, d_poses,
             d_constraint_poses, n_constraints, d_stats, d_verdict, _device.wait(stream_to_wait))

    def merge_map_tensors(self, torch, matches, nmatches, final, cap, slot, counts, src_landmarks, bridge_block, n_dst_landmarks, best=None,
                          n_world=None, stream_to_wait=None):
        """The landmark map of the bridging frame: matches [F][cap][2], nmatches [F], final [F][cap] uint8 and best
        [F][cap][3][2] (optional) as Registration.refine() over the destination leaves them, counts [n_blocks], src_landmarks
        [n_blocks][cap] the source's per-feature landmark map: numpy arrays or device tensors.  Enqueued behind the current
        torch stream (or stream_to_wait); no wait -> MergeMapTensors."""
        dev = torch.device("cuda", torch.cuda.current_device()) if not isinstance(src_landmarks, torch.Tensor) else src_landmarks.device
        t = lambda a, dt: None if a is None else _device.tensor(torch, a, dt, dev)
        ins = [t(matches, np.uint32), t(nmatches, np.uint32), t(final, np.uint8), t(best, np.uint32), t(counts, np.uint32), t(src_landmarks, np.uint32)]
        n_blocks = int(np.prod(src_landmarks.shape)) // cap
        o = MergeMapTensors(torch.zeros((cap, 2), dtype=torch.int32, device=dev), torch.zeros((1,), dtype=torch.int32, device=dev), cap)
        self.merge_map_device(ins[0], ins[1], ins[2], ins[3], n_dst_landmarks if n_world is None else n_world, n_dst_landmarks, cap, slot, ins[4],
                              ins[5], n_blocks, bridge_block, o.map, o.map_count, _device.wait_or_current(torch, stream_to_wait, dev))
        return _device.keep_alive(o, ins)

    def incorporate_tensors(self, torch, dst_table, src_table, merge_map, d_poses, cap, src_blocks, bridge_block, src_pose, skip=None,
                            obs_room=None, lm_room=None, stream_to_wait=None):
        """incorporate_reconstruction of `src_table` into `dst_table` (LandmarkTables; the destination after the bridging frame's
        add_views).  merge_map: a MergeMapTensors, or a host array [n][2] of {source landmark, destination landmark}.  d_poses
        [n_blocks][12] float64 device tensor, updated in place; src_blocks the source's other views; src_pose [12] the bridging
        frame's pose in the source (numpy or a device tensor: copy it before add_views overwrites that row of d_poses); skip
        [n_src_views] (optional).  The rooms default to the least the call accepts.  Enqueued behind the current torch stream
        (or stream_to_wait); no wait -> IncorporateTensors."""
        dev = dst_table.dev
        n_blocks = int(d_poses.shape[0])
        if not isinstance(merge_map, MergeMapTensors):
            pairs = np.ascontiguousarray(merge_map, np.uint32).reshape(-1, 2)
            merge_map = MergeMapTensors(_lib.device_bytes(torch, pairs, dev), _lib.device_bytes(torch, np.array([len(pairs)], np.uint32), dev), len(pairs))
        t = lambda a, dt: None if a is None else _device.tensor(torch, a, dt, dev)
        ins = [t(src_pose, np.float64), t(skip, np.uint32)]
        obs_room = dst_table.n_obs + src_table.n_obs if obs_room is None else obs_room
        lm_room = dst_table.n_landmarks + src_table.n_landmarks if lm_room is None else lm_room
        z32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)
        o = IncorporateTensors(z32(lm_room + 1), z32(max(obs_room, 1), 2), z32(_lib.RS_IR_COUNTS), z32(n_blocks, cap), z32(max(lm_room, 1)),
                               z32(max(src_table.n_landmarks, 1)), z32(1), d_poses, lm_room, obs_room, src_table.n_landmarks)
        self.incorporate_device(dst_table.d_start, dst_table.d_obs, dst_table.n_obs, dst_table.n_landmarks, src_table.d_start, src_table.d_obs,
                                src_table.n_obs, src_table.n_landmarks, merge_map.map, merge_map.map_count, merge_map.map_room, cap, n_blocks,
                                src_blocks, bridge_block, ins[0], ins[1], obs_room, lm_room, d_poses, o.obs_start_out, o.obs_out, o.counts_out,
                                o.landmarks_out, o.obs_counts_out, o.src_key_out, o.call_verdict,
                                _device.wait_or_current(torch, stream_to_wait, dev))
        return _device.keep_alive(o, ins, dst_table, src_table, merge_map)

    def normalize_tensors(self, torch, view_blocks, counts, landmarks, cap, world, d_poses, d_constraint_poses=None, n_world=None,
                          stream_to_wait=None):
        """normalize_reconstruction for the views in `view_blocks` (the first is the reference's first view): counts [n_blocks],
        landmarks [n_blocks][cap] (a landmarks_out), world [n_world][4] float64: numpy arrays or device tensors.  d_poses
        [n_blocks][12] and d_constraint_poses [n][2][12] (optional) float64 device tensors, updated in place.  Enqueued behind
        the current torch stream (or stream_to_wait); no wait -> NormalizeTensors."""
        dev = d_poses.device
        _device.require_device(d_poses, itemsize=8)
        n_constraints = 0
        if d_constraint_poses is not None:
            _device.require_device(d_constraint_poses, itemsize=8)
            n_constraints = int(d_constraint_poses.numel()) // 24
        ins = [_device.tensor(torch, counts, np.uint32, dev), _device.tensor(torch, landmarks, np.uint32, dev), _device.tensor(torch, world, np.float64, dev)]
        n_world = int(np.prod(world.shape)) // 4 if n_world is None else n_world
        o = NormalizeTensors(torch.zeros((2,), dtype=torch.float64, device=dev), torch.zeros((1,), dtype=torch.int32, device=dev), d_poses,
                             d_constraint_poses)
        self.normalize_device(view_blocks, ins[0], ins[1], cap, int(d_poses.shape[0]), ins[2], n_world, d_poses,
                              d_constraint_poses if n_constraints else None, n_constraints, o.stats, o.verdict,
                              _device.wait_or_current(torch, stream_to_wait, dev))
        return _device.keep_alive(o, ins)

    def run_merge_map(self, torch, *args, **kw):
        """merge_map_tensors, then WAITS and copies to the host -> [n][2] uint32"""
        o = self.merge_map_tensors(torch, *args, **kw)
        self._cons.sync()
        return u32(o.map)[:int(u32(o.map_count)[0])]

    def run_incorporate(self, torch, *args, **kw):
        """incorporate_tensors, then WAITS and copies to the host -> IncorporateResult"""
        o = self.incorporate_tensors(torch, *args, **kw)
        self._cons.sync()
        return to_host(o)

    def run_normalize(self, torch, *args, **kw):
        """normalize_tensors, then WAITS -> (mean, count, verdict)"""
        o = self.normalize_tensors(torch, *args, **kw)
        self._cons.sync()
        stats = o.stats.cpu().numpy()
        return float(stats[0]), int(stats[1]), int(u32(o.verdict)[0])


def to_host(o):
    """An IncorporateTensors whose stream has been waited for -> IncorporateResult."""
    counts = u32(o.counts_out)
    rows, n = int(counts[0]), int(counts[1])
    return IncorporateResult(u32(o.obs_start_out)[:rows + 1], u32(o.obs_out)[:n], counts, u32(o.landmarks_out), u32(o.obs_counts_out)[:rows],
                             u32(o.src_key_out)[:o.n_src_landmarks], int(u32(o.call_verdict)[0]), o)
