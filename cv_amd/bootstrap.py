"""Host-side mirror of the two integer steps of cv-sfm's try_init around the three-view bootstrap, over
rs_join_pairs_batch_device and rs_add_reconstruction_batch_device of include/akz.h.

  VSlam::init_reconstruction, the join and the shuffle   cv-sfm/src/lib.rs:992-999, 1190-1191, 1216, 1234
  the two-view inlier minimum                            cv-sfm/src/lib.rs:1421
  VSlamData::add_reconstruction                          cv-sfm/src/lib.rs:377-427
  VSlamData::add_view / add_landmark                     cv-sfm/src/lib.rs:432-500

Both run on the device (cv_amd/csrc/rs_bootstrap_table.hip); there is no CPU fallback.  PairJoin turns the inlier lists two
consensuses left on the device into the three lists ThreeViewInit.init_batch_device reads; ReconstructionStart turns that call's
masks, poses and verdicts into the first generation of the landmark table — CSR lists, the per-feature landmark map, the row
lengths, the three poses and the first ThreeViewConstraint of every new reconstruction — in rs_add_views_device's shapes, so
that reconstruction.start_reconstructions goes from two consensuses to an optimised reconstruction with one wait.
three_view.join_pairs stays as the host form of the join.  The rules that are not the reference's are in DESIGN.md §7.
"""
from dataclasses import dataclass

import numpy as np

from . import _device, _lib
from ._device import call, host_u32 as u32
from .triangulation import LandmarkTable

JOIN_VERDICTS = ("ok", "no_model", "few_inliers", "bad_index")
VERDICTS = ("ok", "not_accepted", "bad_index", "taken", "bad_table")


@dataclass
class JoinTensors:
    """What an rs_join_pairs_batch_device call wrote, on the device (its outputs by their names without d_)."""
    triples: object        # [n_scenes][cap][3] int32 {centre, first, second}
    counts: object         # [3][n_scenes] int32: ntriples, nfirst, nsecond
    first_only: object     # [n_scenes][cap][2] int32
    second_only: object    # [n_scenes][cap][2] int32
    pose_first: object     # [n_scenes][12] float64
    pose_second: object    # [n_scenes][12] float64
    verdict: object        # [n_scenes] int32 (RS_JP_*)
    n_scenes: int
    cap: int

    @property
    def ntriples(self):
        return self.counts[0]

    @property
    def nfirst(self):
        return self.counts[1]

    @property
    def nsecond(self):
        return self.counts[2]


class PairJoin:
    """The join on the context (and stream) of an EssentialConsensus, so that it queues behind that object's consensus calls."""

    def __init__(self, consensus):
        self._cons = consensus

    def join_device(self, d_pairs, d_npairs, d_inliers, d_n_inliers, d_best_id, d_pose, n_slots, cap, slot_first, slot_second, d_triples,
                    d_ntriples, d_first_only, d_nfirst, d_second_only, d_nsecond, d_pose_first, d_pose_second, d_verdict,
                    minimum=_lib.RS_JP_DEFAULT_MINIMUM_ROBUST_MATCHES, shuffle=False, seed=0, stream_to_wait=None):
        """rs_join_pairs_batch_device: d_* and stream_to_wait as _device.arg / wait take them, slot_first / slot_second host lists
        of slots of the consensus call, one per scene.  Enqueues and returns."""
        (a, n), (b, nb) = _device.index_list(slot_first), _device.index_list(slot_second)
        if nb != n:
            raise ValueError("one first and one second slot per scene")
        call("rs_join_pairs_batch_device", self._cons._h, d_pairs, d_npairs, d_inliers, d_n_inliers, d_best_id, d_pose, n_slots, cap, a, b, n,
             minimum, _lib.RS_BATCH_SHUFFLE if shuffle else 0, seed, d_triples, d_ntriples, d_first_only, d_nfirst, d_second_only, d_nsecond,
             d_pose_first, d_pose_second, d_verdict, _device.wait(stream_to_wait))

    def join_tensors(self, torch, pairs, npairs, inliers, n_inliers, best_id, pose, cap, slot_first, slot_second,
                     minimum=_lib.RS_JP_DEFAULT_MINIMUM_ROBUST_MATCHES, shuffle=False, seed=0, stream_to_wait=None, device=0):
        """The join for the scenes (slot_first[s], slot_second[s]): pairs [n_slots][cap][2], npairs [n_slots], inliers
        [n_slots][cap], n_inliers, best_id [n_slots], pose [n_slots][12] float64 as numpy arrays or device tensors (what the
        matcher and rs_essential_arrsac_batch_device left).  Enqueued behind the current torch stream (or stream_to_wait); no
        wait -> JoinTensors."""
        dev = next((a.device for a in (pairs, inliers, pose) if isinstance(a, torch.Tensor)), torch.device("cuda", device))
        n_slots, n = int(np.prod(npairs.shape)), len(slot_first)
        ins = [_device.tensor(torch, a, dt, dev) for a, dt in ((pairs, np.uint32), (npairs, np.uint32), (inliers, np.uint32),
                                                                (n_inliers, np.uint32), (best_id, np.uint32), (pose, np.float64))]
        z32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)
        z64 = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)
        m = max(n, 1)
        o = JoinTensors(z32(m, cap, 3), z32(3, m), z32(m, cap, 2), z32(m, cap, 2), z64(m, 12), z64(m, 12), z32(m), n, cap)
        self.join_device(*ins, n_slots, cap, slot_first, slot_second, o.triples, o.counts[0], o.first_only, o.counts[1], o.second_only,
                         o.counts[2], o.pose_first, o.pose_second, o.verdict, minimum, shuffle, seed,
                         _device.wait_or_current(torch, stream_to_wait, dev))
        return _device.keep_alive(o, ins)

    def run(self, torch, *args, **kw):
        """join_tensors, then WAITS and copies to the host -> per scene (verdict, triples [n][3], first_only [m][2], second_only
        [k][2]) u32."""
        o = self.join_tensors(torch, *args, **kw)
        self._cons.sync()
        counts, t, f, g, v = u32(o.counts), u32(o.triples), u32(o.first_only), u32(o.second_only), u32(o.verdict)
        return [(int(v[s]), t[s, :counts[0, s]].copy(), f[s, :counts[1, s]].copy(), g[s, :counts[2, s]].copy()) for s in range(o.n_scenes)]


@dataclass
class StartTensors:
    """What an rs_add_reconstruction_batch_device call wrote, on the device (its outputs by their names without d_)."""
    obs_start_out: object           # [lm_room + 1] int32
    obs_out: object                 # [obs_room][2] int32, rows [0, counts_out[1]) written
    obs_counts_out: object          # [lm_room] int32: the row lengths
    counts_out: object              # [RS_AR_COUNTS] int32 {rows filled, observations filled, reconstructions, scenes accepted}
    landmarks_out: object           # [n_blocks][cap] int32: the landmark of every feature, -1 (0xFFFFFFFF) for none
    recon_start_out: object         # [n_recons + n_scenes + 1] int32
    view_start_out: object          # [n_recons + n_scenes + 1] int32
    views_out: object               # [n_scenes][3] int32
    constraint_poses_out: object    # [n_scenes][24] float64
    constraint_verdict_out: object  # [n_scenes] int32: RS_TVC_OK or RS_CV_NOT_RECORDED
    frame_verdict: object           # [n_scenes] int32 (RS_AR_*)
    stats: object                   # [n_scenes][RS_AR_STATS] int32
    call_verdict: object            # [1] int32: RS_AR_OK or RS_AR_BAD_TABLE
    kps_dst: object                 # the caller's destination pool, [n_blocks][cap] keypoints
    counts_dst: object              # [n_blocks] int32
    poses: object                   # [n_blocks][12] float64, the caller's tensor, updated in place
    lm_room: int
    obs_room: int
    n_scenes: int
    n_recons: int

    def table(self, torch, counts=None):
        """The new table as a LandmarkTable over these tensors.  Without `counts` nothing is waited for: the table has lm_room
        rows and room for obs_room observations, the rows behind the filled ones are empty lists.  counts = (rows,
        observations) as a caller that has waited read them from counts_out: the table of exactly the filled rows."""
        n_lm, n_obs = (self.lm_room, self.obs_room) if counts is None else (int(counts[0]), int(counts[1]))
        return LandmarkTable.from_device(torch, self.obs_start_out, self.obs_out, n_lm, n_obs, d_obs_counts=self.obs_counts_out)


@dataclass
class StartResult:
    obs_start: np.ndarray             # [rows + 1] the new table, filled rows only
    obs: np.ndarray                   # [observations][2]
    obs_counts: np.ndarray            # [rows]
    counts: np.ndarray                # [RS_AR_COUNTS] u32
    landmarks: np.ndarray             # [n_blocks][cap] u32
    recon_start: np.ndarray           # [n_recons + n_scenes + 1] u32
    view_start: np.ndarray            # [n_recons + n_scenes + 1] u32
    views: np.ndarray                 # [n_scenes][3] u32
    constraint_poses: np.ndarray      # [n_scenes][2][3][4]
    constraint_verdicts: np.ndarray   # [n_scenes] u32
    frame_verdicts: np.ndarray        # [n_scenes] u32
    stats: np.ndarray                 # [n_scenes][RS_AR_STATS] u32
    call_verdict: int
    tensors: object                   # the StartTensors it was read from


class ReconstructionStart:
    """add_reconstruction on the context (and stream) of an EssentialConsensus, so that it queues behind that object's other
    calls."""

    def __init__(self, consensus):
        self._cons = consensus

    def add_device(self, d_triples, d_ntriples, d_first_only, d_nfirst, d_second_only, d_nsecond, d_combined, d_first_ok, d_second_ok,
                   d_pose_out, d_verdict, ic, i_first, i_second, d_kps, d_counts, n_src_blocks, cap, d_skip, d_obs_start, d_obs, n_obs,
                   n_landmarks, d_recon_start, d_view_start, n_recons, d_kps_dst, d_counts_dst, d_poses, n_blocks, view_base, obs_room, lm_room,
                   d_obs_start_out, d_obs_out, d_obs_counts_out, d_counts_out, d_landmarks_out, d_recon_start_out, d_view_start_out,
                   d_views_out, d_constraint_poses_out, d_constraint_verdict_out, d_frame_verdict, d_stats, d_call_verdict,
                   stream_to_wait=None):
        """rs_add_reconstruction_batch_device: d_* and stream_to_wait as _device.arg / wait take them, ic / i_first / i_second host
        lists of source blocks, one per scene.  Enqueues and returns."""
        (a, n), (b, nb), (c, nc) = (_device.index_list(x) for x in (ic, i_first, i_second))
        if nb != n or nc != n:
            raise ValueError("one centre, first and second block per scene")
        call("rs_add_reconstruction_batch_device", self._cons._h, d_triples, d_ntriples, d_first_only, d_nfirst, d_second_only, d_nsecond,
             d_combined, d_first_ok, d_second_ok, d_pose_out, d_verdict, a, b, c, n, d_kps, d_counts, n_src_blocks, cap, d_skip, d_obs_start,
             d_obs, n_obs, n_landmarks, d_recon_start, d_view_start, n_recons, d_kps_dst, d_counts_dst, d_poses, n_blocks, view_base, obs_room,
             lm_room, d_obs_start_out, d_obs_out, d_obs_counts_out, d_counts_out, d_landmarks_out, d_recon_start_out, d_view_start_out,
             d_views_out, d_constraint_poses_out, d_constraint_verdict_out, d_frame_verdict, d_stats, d_call_verdict,
             _device.wait(stream_to_wait))

    def add_tensors(self, torch, join, combined, first_ok, second_ok, pose_out, verdict, ic, i_first, i_second, d_kps, counts, cap, d_kps_dst,
                    d_counts_dst, d_poses, view_base, table=None, recon_start=None, view_start=None, skip=None, obs_room=None, lm_room=None,
                    stream_to_wait=None):
        """add_reconstruction for the scenes of a bootstrap call.  join: the JoinTensors the bootstrap read (or anything with
        triples, ntriples, first_only, nfirst, second_only, nsecond); combined, first_ok, second_ok [n_scenes][cap] uint8, pose_out
        [n_scenes][24] float64 and verdict [n_scenes] as ThreeViewInit.init_batch_device left them; d_kps [n_src_blocks][cap]
        keypoints and counts [n_src_blocks] the source pool; d_kps_dst, d_counts_dst [n_blocks] int32 and d_poses [n_blocks][12]
        float64 the destination pool (device tensors, written in place); table (a LandmarkTable) with recon_start / view_start
        [n_recons + 1] the existing table, or None.  The rooms default to the least the call accepts.  Enqueued behind the
        current torch stream (or stream_to_wait); no wait -> StartTensors."""
        dev = d_poses.device
        n = len(ic)
        n_blocks, n_src_blocks = int(d_poses.shape[0]), int(np.prod(counts.shape))
        t = lambda a, dt: None if a is None else _device.tensor(torch, a, dt, dev)
        ins = [t(combined, np.uint8), t(first_ok, np.uint8), t(second_ok, np.uint8), t(pose_out, np.float64), t(verdict, np.uint32),
               t(counts, np.uint32), t(skip, np.uint32), t(recon_start, np.uint32), t(view_start, np.uint32)]
        n_recons = 0 if recon_start is None else int(np.prod(recon_start.shape)) - 1
        n_lm, n_obs = (0, 0) if table is None else (table.n_landmarks, table.n_obs)
        grow = 3 * n * cap
        obs_room = n_obs + grow if obs_room is None else obs_room
        lm_room = n_lm + grow if lm_room is None else lm_room
        z32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)
        m = max(n, 1)
        o = StartTensors(z32(lm_room + 1), z32(max(obs_room, 1), 2), z32(max(lm_room, 1)), z32(_lib.RS_AR_COUNTS), z32(n_blocks, cap),
                         z32(n_recons + n + 1), z32(n_recons + n + 1), z32(m, 3), torch.zeros((m, 24), dtype=torch.float64, device=dev), z32(m),
                         z32(m), z32(m, _lib.RS_AR_STATS), z32(1), d_kps_dst, d_counts_dst, d_poses, lm_room, obs_room, n, n_recons)
        self.add_device(join.triples, join.ntriples, join.first_only, join.nfirst, join.second_only, join.nsecond, ins[0], ins[1], ins[2], ins[3],
                        ins[4], ic, i_first, i_second, d_kps, ins[5], n_src_blocks, cap, ins[6], None if table is None else table.d_start,
                        None if table is None or not n_obs else table.d_obs, n_obs, n_lm, ins[7] if n_recons else None,
                        ins[8] if n_recons else None, n_recons, d_kps_dst, d_counts_dst, d_poses, n_blocks, view_base, obs_room, lm_room,
                        o.obs_start_out, o.obs_out, o.obs_counts_out, o.counts_out, o.landmarks_out, o.recon_start_out, o.view_start_out,
                        o.views_out, o.constraint_poses_out, o.constraint_verdict_out, o.frame_verdict, o.stats, o.call_verdict,
                        _device.wait_or_current(torch, stream_to_wait, dev))
        return _device.keep_alive(o, ins, join, table, d_kps)

    def run(self, torch, *args, **kw):
        """add_tensors, then WAITS and copies to the host -> StartResult."""
        o = self.add_tensors(torch, *args, **kw)
        self._cons.sync()
        return to_host(o)


def to_host(o):
    """A StartTensors whose stream has been waited for -> StartResult."""
    counts = u32(o.counts_out)
    rows, n, s = int(counts[0]), int(counts[1]), o.n_scenes
    return StartResult(u32(o.obs_start_out)[:rows + 1], u32(o.obs_out)[:n], u32(o.obs_counts_out)[:rows], counts, u32(o.landmarks_out),
                       u32(o.recon_start_out), u32(o.view_start_out), u32(o.views_out)[:s], o.constraint_poses_out.cpu().numpy()[:s].reshape(-1, 2, 3, 4),
                       u32(o.constraint_verdict_out)[:s], u32(o.frame_verdict)[:s], u32(o.stats)[:s], int(u32(o.call_verdict)[0]), o)
