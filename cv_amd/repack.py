"""Host-side mirror of the repacking of a reconstruction, over rs_repack_table_device, rs_gather_blocks_device and
rs_repack_constraints_device of include/akz.h.

  VSlamData::remove_view                     cv-sfm/src/lib.rs:517-546
  callers: apply_bundle_adjust               cv-sfm/src/lib.rs:502-515
           incorporate_reconstruction        cv-sfm/src/lib.rs:1880-1884
           try_merge_reconstructions         cv-sfm/src/lib.rs:2147

All of it runs on the device (cv_amd/csrc/rs_repack.hip); there is no CPU fallback.  One block map — the new block of every old
block, 0xFFFFFFFF for a removed view — drives the table, every per-block pool, the constraints and (FrameIndex.remap_views) the
frame table.  The repacked table always fits n_blocks_out * cap rows and observations, so a chain that never reads a count
back runs in bounded memory: reconstruction.repack chains the stages with one wait.  What is not the reference's (stable order,
the empty table on a refusal, the constraint tail) is in DESIGN.md §7.
"""
from dataclasses import dataclass

import numpy as np

from . import _device, _lib
from ._device import call, host_u32 as u32
from .triangulation import LandmarkTable

VERDICTS = ("ok", "bad_table", "bad_index", "bad_map", "no_room")
NONE = 0xFFFFFFFF


@dataclass
class RepackTensors:
    """What an rs_repack_table_device call wrote, on the device (its outputs by their names without d_)."""
    obs_start_out: object    # [lm_room + 1] int32
    obs_out: object          # [obs_room][2] int32, rows [0, counts_out[1]) written
    obs_counts_out: object   # [lm_room] int32: the row lengths
    landmarks_out: object    # [n_blocks_out][cap] int32: the landmark of every feature, -1 (0xFFFFFFFF) for none
    key_out: object          # [n_landmarks] int32: the new key of every old row, -1 for a dropped one
    recon_start_out: object  # [n_recons + 1] int32, or None
    counts_out: object       # [RS_RP_COUNTS] int32
    call_verdict: object     # [1] int32 (RS_RP_*)
    lm_room: int
    obs_room: int
    n_blocks_out: int

    def table(self, torch, counts=None):
        """The new table as a LandmarkTable over these tensors.  Without `counts` nothing is waited for: the table has lm_room
        rows, the rows behind the kept ones are empty lists.  counts = (rows, observations) as a caller that has waited read
        them from counts_out: the table of exactly the kept rows — the same bytes on those."""
        n_lm, n_obs = (self.lm_room, self.obs_room) if counts is None else (int(counts[0]), int(counts[1]))
        return LandmarkTable.from_device(torch, self.obs_start_out, self.obs_out, n_lm, n_obs, d_obs_counts=self.obs_counts_out)


@dataclass
class RepackResult:
    obs_start: np.ndarray      # [rows + 1] the new table, kept rows only
    obs: np.ndarray            # [observations][2]
    obs_counts: np.ndarray     # [rows]
    landmarks: np.ndarray      # [n_blocks_out][cap] u32
    keys: np.ndarray           # [n_landmarks] u32
    recon_start: object        # [n_recons + 1] u32 or None
    counts: np.ndarray         # [RS_RP_COUNTS] u32
    call_verdict: int
    tensors: object            # the RepackTensors it was read from


@dataclass
class ConstraintTensors:
    """What an rs_repack_constraints_device call wrote, on the device."""
    views_out: object          # [n][3] int32, -1 behind the count
    poses_out: object          # [n][2][12] float64, 0 behind the count
    verdict_out: object        # [n] int32, RS_TVC_BAD_INDEX behind the count
    count: object              # [1] int32
    start_out: object          # [n_ranges + 1] int32, or None
    room: int


def _words(a):
    """how many elements a numpy array, a sequence or a tensor holds"""
    return int(a.numel()) if hasattr(a, "numel") else int(np.size(a))


class TableRepack:
    """The repacking on the context (and stream) of an EssentialConsensus, so that it queues behind that object's other calls."""

    def __init__(self, consensus):
        self._cons = consensus

    def table_device(self, d_obs_start, d_obs, n_obs, n_landmarks, cap, n_blocks, d_block_map, n_blocks_out, d_recon_start, n_recons, obs_room,
                     lm_room, d_obs_start_out, d_obs_out, d_obs_counts_out, d_landmarks_out, d_key_out, d_recon_start_out, d_counts_out,
                     d_call_verdict, stream_to_wait=None):
        """rs_repack_table_device: d_* and stream_to_wait as _device.arg / wait take them.  Enqueues and returns."""
        call("rs_repack_table_device", self._cons._h, d_obs_start, d_obs, n_obs, n_landmarks, cap, n_blocks, d_block_map, n_blocks_out,
             d_recon_start, n_recons, obs_room, lm_room, d_obs_start_out, d_obs_out, d_obs_counts_out, d_landmarks_out, d_key_out,
             d_recon_start_out, d_counts_out, d_call_verdict, _device.wait(stream_to_wait))

    def gather_device(self, d_src, d_dst, row_bytes, n_blocks, d_block_map, n_blocks_out, d_verdict, stream_to_wait=None):
        """rs_gather_blocks_device.  Enqueues and returns."""
        call("rs_gather_blocks_device", self._cons._h, d_src, d_dst, row_bytes, n_blocks, d_block_map, n_blocks_out, d_verdict,
             _device.wait(stream_to_wait))

    def constraints_device(self, d_views, d_poses, d_verdict, n, d_block_map, n_blocks, n_blocks_out, d_start, n_ranges, d_views_out, d_poses_out,
                           d_verdict_out, d_count, d_start_out, stream_to_wait=None):
        """rs_repack_constraints_device.  Enqueues and returns."""
        call("rs_repack_constraints_device", self._cons._h, d_views, d_poses, d_verdict, n, d_block_map, n_blocks, n_blocks_out, d_start,
             n_ranges, d_views_out, d_poses_out, d_verdict_out, d_count, d_start_out, _device.wait(stream_to_wait))

    @staticmethod
    def _map(torch, block_map, dev):
        """the block map on the device as 4-byte words (what a later call of the chain takes again as it is)"""
        if block_map is None or isinstance(block_map, torch.Tensor):
            return _device.tensor(torch, block_map, np.uint32, dev) if block_map is not None else None
        return torch.from_numpy(np.ascontiguousarray(block_map, np.uint32).reshape(-1).view(np.int32)).to(dev)

    def table_tensors(self, torch, table, cap, n_blocks, block_map, n_blocks_out, recon_start=None, obs_room=None, lm_room=None, fill=0,
                      stream_to_wait=None):
        """`table` (a LandmarkTable) without the views block_map removes ([n_blocks] u32, a numpy array or a device tensor; None:
        the identity).  recon_start [n_recons + 1] (optional): the reconstructions' row ranges.  The rooms default to
        n_blocks_out * cap, which a valid table cannot outgrow.  The output tensors start as `fill`.  Enqueued behind the current
        torch stream (or stream_to_wait); no wait -> RepackTensors."""
        dev = table.dev
        d_map = self._map(torch, block_map, dev)
        d_recon = None if recon_start is None else _device.tensor(torch, recon_start, np.uint32, dev)
        n_recons = 0 if recon_start is None else _words(recon_start) - 1
        obs_room = n_blocks_out * cap if obs_room is None else obs_room
        lm_room = n_blocks_out * cap if lm_room is None else lm_room
        f32 = lambda *shape: torch.full(shape, fill, dtype=torch.int32, device=dev)
        o = RepackTensors(f32(lm_room + 1), f32(max(obs_room, 1), 2), f32(max(lm_room, 1)), f32(max(n_blocks_out, 1), cap),
                          f32(max(table.n_landmarks, 1)), None if recon_start is None else f32(n_recons + 1), f32(_lib.RS_RP_COUNTS), f32(1),
                          lm_room, obs_room, n_blocks_out)
        self.table_device(table.d_start, table.d_obs, table.n_obs, table.n_landmarks, cap, n_blocks, d_map, n_blocks_out, d_recon, n_recons,
                          obs_room, lm_room, o.obs_start_out, o.obs_out, o.obs_counts_out, o.landmarks_out, o.key_out, o.recon_start_out,
                          o.counts_out, o.call_verdict, _device.wait_or_current(torch, stream_to_wait, dev))
        return _device.keep_alive(o, d_map, d_recon, table)

    def gather_tensors(self, torch, src, block_map, n_blocks_out, out=None, verdict=None, stream_to_wait=None):
        """A per-block pool `src` [n_blocks][...] (a contiguous device tensor whose rows are a multiple of 4 bytes) moved through
        the map -> (dst [n_blocks_out][...], verdict [1] int32), every byte of dst written.  No wait."""
        _device.require_device(src)
        dev = src.device
        n_blocks = int(src.shape[0])
        row_bytes = src.element_size() * int(np.prod(src.shape[1:], dtype=np.int64))
        d_map = self._map(torch, block_map, dev)
        if out is None:
            out = torch.empty((max(n_blocks_out, 1),) + tuple(src.shape[1:]), dtype=src.dtype, device=dev)
        if verdict is None:
            verdict = torch.zeros(1, dtype=torch.int32, device=dev)
        self.gather_device(src, out, row_bytes, n_blocks, d_map, n_blocks_out, verdict, _device.wait_or_current(torch, stream_to_wait, dev))
        _device.keep_alive(self._cons, d_map, src)
        return out[:n_blocks_out], verdict

    def constraints_tensors(self, torch, views, poses, verdict, block_map, n_blocks, n_blocks_out, start=None, fill=0, stream_to_wait=None):
        """The constraints that keep all three views, in order, views mapped: views [n][3], poses [n][2][12] float64, verdict
        [n] (numpy arrays or device tensors), start [n_ranges + 1] optional ranges of constraints.  No wait -> ConstraintTensors
        with room n; behind the count: triples no stage takes."""
        dev = torch.device("cuda", torch.cuda.current_device()) if not isinstance(views, torch.Tensor) else views.device
        d_views, d_verdict = _device.tensor(torch, views, np.uint32, dev), _device.tensor(torch, verdict, np.uint32, dev)
        d_poses = _device.tensor(torch, poses, np.float64, dev)
        n = _words(verdict)
        d_map = self._map(torch, block_map, dev)
        d_start = None if start is None else _device.tensor(torch, start, np.uint32, dev)
        n_ranges = 0 if start is None else _words(start) - 1
        o = ConstraintTensors(torch.full((max(n, 1), 3), fill, dtype=torch.int32, device=dev),
                              torch.full((max(n, 1), 2, 12), float(fill), dtype=torch.float64, device=dev),
                              torch.full((max(n, 1),), fill, dtype=torch.int32, device=dev), torch.full((1,), fill, dtype=torch.int32, device=dev),
                              None if start is None else torch.full((n_ranges + 1,), fill, dtype=torch.int32, device=dev), n)
        self.constraints_device(d_views, d_poses, d_verdict, n, d_map, n_blocks, n_blocks_out, d_start, n_ranges, o.views_out, o.poses_out,
                                o.verdict_out, o.count, o.start_out, _device.wait_or_current(torch, stream_to_wait, dev))
        return _device.keep_alive(o, d_views, d_poses, d_verdict, d_map, d_start)

    def run_table(self, torch, table, cap, n_blocks, block_map, n_blocks_out, **kw):
        """table_tensors, then WAITS and copies to the host -> RepackResult."""
        o = self.table_tensors(torch, table, cap, n_blocks, block_map, n_blocks_out, **kw)
        self._cons.sync()
        return to_host(o)

    def run_gather(self, torch, src, block_map, n_blocks_out):
        """gather_tensors, then WAITS -> (dst on the host, verdict)."""
        dst, verdict = self.gather_tensors(torch, src, block_map, n_blocks_out)
        self._cons.sync()
        return dst.cpu().numpy(), int(u32(verdict)[0])

    def run_constraints(self, torch, views, poses, verdict, block_map, n_blocks, n_blocks_out, start=None):
        """constraints_tensors, then WAITS -> (views [count][3] u32, poses [count][2][12], verdict [count] u32, start_out or None)."""
        o = self.constraints_tensors(torch, views, poses, verdict, block_map, n_blocks, n_blocks_out, start)
        self._cons.sync()
        k = int(u32(o.count)[0])
        return (u32(o.views_out)[:k], o.poses_out.cpu().numpy()[:k], u32(o.verdict_out)[:k],
                None if o.start_out is None else u32(o.start_out))


def to_host(o):
    """A RepackTensors whose stream has been waited for -> RepackResult."""
    counts = u32(o.counts_out)
    verdict = int(u32(o.call_verdict)[0])
    rows, n = (int(counts[0]), int(counts[1])) if verdict == _lib.RS_RP_OK else (0, 0)
    return RepackResult(u32(o.obs_start_out)[:rows + 1], u32(o.obs_out)[:n], u32(o.obs_counts_out)[:rows], u32(o.landmarks_out)[:o.n_blocks_out],
                        u32(o.key_out), None if o.recon_start_out is None else u32(o.recon_start_out), counts, verdict, o)
