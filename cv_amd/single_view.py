"""Host-side mirror of what cv-sfm's register_frame_subset does behind its consensus, over rs_refine_poses_batch_device of
include/akz.h.

  take(single_view_optimization_num_matches) of the inliers        cv-sfm/src/lib.rs:1625-1634
  single_view_simple_optimize_l2                                   cv-optimize/src/single_view_optimizer.rs:80-135
  is_observation_consistent, the re-selection and the last run     cv-sfm/src/lib.rs:1636-1710, 2622-2655
  final_num_robust_matches, final_matches, the acceptance tests    cv-sfm/src/lib.rs:1712-1775

Every new frame of a micro-batch is worked by one persistent workgroup on the device (cv_amd/csrc/rs_single_view.hip); there
is no CPU fallback.  The pose that enters the pose graph and the observations that enter the landmark table are the outputs of
this stage, not the consensus'.
"""
from dataclasses import dataclass

from . import _device, _lib
from ._device import call, host_u32

VERDICTS = ("ok", "no_model", "few_landmarks", "lost_half", "few_robust", "bad_index")


@dataclass
class RefineOutputs:
    """Device tensors of one call, complete on the consensus' stream: pose [S][12] float64 (rows of RS_SV_OK and
    RS_SV_NO_MODEL scenes are written), verdict [S] int32 (RS_SV_*), final [S][cap] uint8 (the final_matches map over the
    original matches), n_final [S] int32, stats [S][RS_SV_STATS] int32."""
    pose: object
    verdict: object
    final: object
    n_final: object
    stats: object

    def host(self):
        """-> (pose [S][3][4], verdict [S] u32, final [S][cap] bool, n_final [S] u32, stats [S][RS_SV_STATS] u32); the caller
        has waited for the stream."""
        return (self.pose.cpu().numpy().reshape(-1, 3, 4), host_u32(self.verdict), self.final.cpu().numpy().astype(bool),
                host_u32(self.n_final), host_u32(self.stats))


class SingleViewRefiner:
    """The refinement on the context (and stream) of an EssentialConsensus, so that it queues behind that object's
    rs_p3p_arrsac_batch_device call without a host step."""

    def __init__(self, consensus):
        self._cons = consensus

    @staticmethod
    def params(**kw):
        """rs_single_view_params: the reference's defaults (cv-sfm/src/settings.rs:324-383) with `kw` on top; `triangulate`
        takes an rs_triangulate_params (cv_amd.triangulation.make_params)."""
        return _lib.params(_lib.SingleViewParams, "rs_single_view_params_default", **kw)

    def refine_batch_device(self, d_kps, cap_per_img, n_blocks, d_poses, cam, d_obs_start, d_obs, n_obs, n_landmarks, d_world, n_world, ik,
                            d_matches, d_nmatches, d_best, d_pose, d_best_id, d_inliers, d_n_inliers, params, d_pose_out, d_verdict, d_final,
                            d_n_final, d_stats, stream_to_wait=None):
        """rs_refine_poses_batch_device: d_* and stream_to_wait as _device.arg / wait take them (d_best may be None), ik a host
        list of the new frames' keypoint blocks, one per scene.  Enqueues on the consensus' stream and returns; its sync() waits."""
        blocks, n = _device.index_list(ik)
        call("rs_refine_poses_batch_device", self._cons._h, d_kps, cap_per_img, n_blocks, d_poses, cam, d_obs_start, d_obs, n_obs,
             n_landmarks, d_world, n_world, blocks, d_matches, d_nmatches, d_best, d_pose, d_best_id, d_inliers, d_n_inliers, n, params,
             d_pose_out, d_verdict, d_final, d_n_final, d_stats, _device.wait(stream_to_wait))

    def refine_tensors(self, torch, d_kps, d_poses, cam, d_obs_start, d_obs, n_landmarks, d_world, n_world, ik, d_matches, d_nmatches, d_best,
                       d_pose, d_best_id, d_inliers, d_n_inliers, params=None, out=None, stream_to_wait=None):
        """One batch from torch tensors on the device: d_kps [n_blocks][cap] keypoints (uint8 [n_blocks][cap][28] as
        akz_extract_batch_device leaves them), d_poses [n_blocks][12] float64, d_obs_start [n_landmarks + 1] and d_obs [n_obs][2]
        int32, d_world [rows][4] float64, d_matches [S][cap][2] / d_nmatches [S] the original matches, d_best [S][cap][3][2] or
        None, and the consensus' d_pose [S][12], d_best_id [S], d_inliers [S][cap], d_n_inliers [S].  Enqueues and returns
        without waiting -> RefineOutputs (`out`: one from an earlier call, to be written again)."""
        S = len(ik)
        n_blocks = int(d_kps.shape[0])
        cap = d_kps.numel() * d_kps.element_size() // (28 * n_blocks)
        dev = d_kps.device
        _device.require_device(d_kps, d_poses, d_obs_start, d_obs, d_world, d_matches, d_nmatches, d_pose, d_best_id, d_inliers, d_n_inliers)
        if d_poses.dtype != torch.float64 or d_poses.numel() != 12 * n_blocks or d_obs_start.numel() != n_landmarks + 1:
            raise ValueError("d_poses is [n_blocks][12] float64, d_obs_start [n_landmarks + 1]")
        if d_matches.numel() < 2 * S * cap or d_inliers.numel() < S * cap:
            raise ValueError("d_matches is [S][cap][2], d_inliers [S][cap]")
        rows = n_world + (S * cap if d_best is not None else 0)
        if d_world.shape[0] < rows:
            raise ValueError("d_world holds n_world rows, and S * cap more with d_best")
        if out is None:
            out = RefineOutputs(torch.zeros((max(S, 1), 12), dtype=torch.float64, device=dev),
                                torch.zeros(max(S, 1), dtype=torch.int32, device=dev),
                                torch.zeros((max(S, 1), cap), dtype=torch.uint8, device=dev),
                                torch.zeros(max(S, 1), dtype=torch.int32, device=dev),
                                torch.zeros((max(S, 1), _lib.RS_SV_STATS), dtype=torch.int32, device=dev))
        n_obs = int(d_obs.numel() // 2)
        self.refine_batch_device(d_kps, cap, n_blocks, d_poses, cam, d_obs_start, d_obs if n_obs else None, n_obs, n_landmarks, d_world,
                                 n_world, ik, d_matches, d_nmatches, d_best, d_pose, d_best_id, d_inliers, d_n_inliers,
                                 params or self.params(), out.pose, out.verdict, out.final, out.n_final, out.stats, stream_to_wait)
        return out
