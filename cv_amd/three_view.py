"""Host-side mirror of cv-sfm's three-view bootstrap over rs_three_view_init_batch_device of include/akz.h.

  VSlam::init_reconstruction, from the common matches on     cv-sfm/src/lib.rs:1002-1300
  three_view_simple_optimize_l2                               cv-optimize/src/three_view_optimizer.rs:126-200
  the join of the two pair lists (host form: join_pairs)     cv-sfm/src/lib.rs:992-998, 1190-1191, 1216, 1234

Every triple is worked by one persistent workgroup on the device (cv_amd/csrc/rs_three_view.hip); there is no CPU fallback.
The join and the shuffle of the common matches use the caller's HashMap and RNG in the reference; on the device they are
rs_join_pairs_batch_device's (cv_amd.bootstrap.PairJoin).  `join_pairs` is the host form: it builds the three index lists in the
reference's order.

And of the pose graph's three-view constraints over rs_three_view_constraint_batch_device:

  VSlam::optimize_three_view behind its shuffle and sort     cv-sfm/src/lib.rs:1939-2062
  three_view_adaptive_optimize_l2                             cv-optimize/src/three_view_optimizer.rs:203-272

One wavefront per constraint (cv_amd/csrc/rs_three_view_constraint.hip).  The shuffle and the unstable sort by observation
count use the caller's RNG and Rust's tie order in the reference and stay on the host: `order_landmarks` builds one
admissible order.
"""
from dataclasses import dataclass

import numpy as np

from . import _device, _lib
from ._device import call

VERDICTS = ("ok", "few_scales", "few_bearing_pairs", "few_matches", "lost_half", "few_robust", "bad_index")


def join_pairs(first_pairs, second_pairs, permutation=None):
    """(triples [n][3] {centre, first, second}, first_only [m][2], second_only [k][2]) u32 from the inlier lists
    [(centre, first)] and [(centre, second)] of two consensuses.  As the reference: a HashMap centre -> other feature per
    list (a centre feature that occurs twice keeps its LAST entry), triples in the order of first_pairs, the one-pair lists in
    the order of their own pair list.  `permutation` (of range(n)) is the shuffle of lib.rs:999, the caller's RNG."""
    fp = np.asarray(first_pairs, np.int64).reshape(-1, 2)
    sp = np.asarray(second_pairs, np.int64).reshape(-1, 2)
    second_map = {int(c): int(s) for c, s in sp}
    first_map = {int(c): int(f) for c, f in fp}
    triples = np.array([(c, f, second_map[c]) for c, f in fp.tolist() if c in second_map], np.uint32).reshape(-1, 3)
    if permutation is not None:
        perm = np.asarray(permutation, np.int64)
        if sorted(perm.tolist()) != list(range(len(triples))):
            raise ValueError("permutation must be a permutation of the common matches")
        triples = triples[perm]
    first_only = np.array([(c, f) for c, f in fp.tolist() if c not in second_map], np.uint32).reshape(-1, 2)
    second_only = np.array([(c, s) for c, s in sp.tolist() if c not in first_map], np.uint32).reshape(-1, 2)
    return triples, first_only, second_only


@dataclass
class ThreeViewResult:
    verdict: int
    poses: np.ndarray        # [2][3][4] CameraToCamera centre -> first / second, or None
    combined: np.ndarray     # bool per common match, or None
    first_ok: np.ndarray
    second_ok: np.ndarray
    stats: np.ndarray        # [RS_TV_STATS] u32

    @property
    def verdict_name(self):
        return VERDICTS[self.verdict]

    @property
    def median_scale(self):
        return _lib.stat_f64(self.stats, _lib.RS_TV_S_MEDIAN)


class ThreeViewInit:
    """The three-view bootstrap on the context (and stream) of an EssentialConsensus, so that it queues behind that
    object's consensus calls."""

    def __init__(self, consensus):
        self._cons = consensus

    @staticmethod
    def params(**kw):
        """rs_three_view_params: the reference's defaults (cv-sfm/src/settings.rs:320-427) with `kw` on top; `triangulate`
        takes an rs_triangulate_params (cv_amd.triangulation.make_params)."""
        return _lib.params(_lib.ThreeViewParams, "rs_three_view_params_default", **kw)

    def init_batch_device(self, d_kps, cap_per_img, n_blocks, ic, i_first, i_second, cam, d_pose_first, d_pose_second, d_triples,
                          d_ntriples, d_first_only, d_nfirst, d_second_only, d_nsecond, params, d_pose_out, d_verdict, d_combined,
                          d_first_ok, d_second_ok, d_stats, stream_to_wait=None):
        """rs_three_view_init_batch_device: d_* and stream_to_wait as _device.arg / wait take them, ic / i_first / i_second host lists of
        keypoint-block indices, one per scene.  Enqueues on the consensus' stream and returns; its sync() waits."""
        (a, n), (b, nb), (c, nc) = (_device.index_list(x) for x in (ic, i_first, i_second))
        if nb != n or nc != n:
            raise ValueError("one centre, first and second block per scene")
        call("rs_three_view_init_batch_device", self._cons._h, d_kps, cap_per_img, n_blocks, a, b, c, cam, d_pose_first,
             d_pose_second, d_triples, d_ntriples, d_first_only, d_nfirst, d_second_only, d_nsecond, n, params, d_pose_out,
             d_verdict, d_combined, d_first_ok, d_second_ok, d_stats, _device.wait(stream_to_wait))

    def init(self, torch, keypoints, cam, pose_first, pose_second, first_pairs, second_pairs, params=None, permutation=None, device=0):
        """One triple from host arrays: keypoints = (centre, first, second) KP_DTYPE arrays, the two CameraToCamera poses
        [3][4] and inlier pair lists of the consensuses.  Copies, runs the device call, waits.  -> ThreeViewResult."""
        triples, first_only, second_only = join_pairs(first_pairs, second_pairs, permutation)
        cap = max(1, max(len(k) for k in keypoints), len(triples), len(first_only), len(second_only))
        kps = np.zeros((3, cap), _lib.KP_DTYPE)
        for k in range(3):
            kps[k, :len(keypoints[k])] = np.asarray(keypoints[k], _lib.KP_DTYPE)
        dev = torch.device("cuda", device)
        up = lambda a: _lib.device_bytes(torch, a, dev)

        def padded(a, w):
            out = np.zeros((cap, w), np.uint32)
            out[:len(a)] = a
            return out

        d_kps, d_t, d_f, d_s = up(kps), up(padded(triples, 3)), up(padded(first_only, 2)), up(padded(second_only, 2))
        d_n = up(np.array([len(triples), len(first_only), len(second_only)], np.uint32))
        d_pf, d_ps = up(np.asarray(pose_first, np.float64).reshape(12)), up(np.asarray(pose_second, np.float64).reshape(12))
        d_pose = torch.zeros(24, dtype=torch.float64, device=dev)
        d_masks = torch.zeros((3, cap), dtype=torch.uint8, device=dev)
        d_out = torch.zeros(1 + _lib.RS_TV_STATS, dtype=torch.int32, device=dev)
        self.init_batch_device(d_kps, cap, 3, [0], [1], [2], cam, d_pf, d_ps, d_t, d_n, d_f, d_n.data_ptr() + 4, d_s,
                               d_n.data_ptr() + 8, params or self.params(), d_pose, d_out, d_masks[0], d_masks[1], d_masks[2],
                               d_out.data_ptr() + 4, torch.cuda.current_stream(dev))
        self._cons.sync()
        out = _device.host_u32(d_out)
        ok = int(out[0]) == _lib.RS_TV_OK
        masks = d_masks.cpu().numpy().astype(bool)
        return ThreeViewResult(int(out[0]), d_pose.cpu().numpy().reshape(2, 3, 4) if ok else None,
                               masks[0, :len(triples)] if ok else None, masks[1, :len(first_only)] if ok else None,
                               masks[2, :len(second_only)] if ok else None, out[1:].copy())


CONSTRAINT_VERDICTS = ("ok", "few_landmarks", "few_bearing_pairs", "bad_index")


def order_landmarks(obs_counts, permutation=None):
    """The positions of a constraint's landmarks in the order optimize_three_view walks them in: `permutation` (of
    range(n), the shuffle of lib.rs:1968, the caller's RNG; default none), then a STABLE descending sort by observation count.
    The reference sorts with sort_unstable_by_key, which fixes no order among landmarks with equal counts: this is one
    admissible order, not the one a given Rust build produces."""
    counts = np.asarray(obs_counts, np.int64).reshape(-1)
    perm = np.arange(len(counts)) if permutation is None else np.asarray(permutation, np.int64)
    if sorted(perm.tolist()) != list(range(len(counts))):
        raise ValueError("permutation must be a permutation of the landmarks")
    return perm[np.argsort(-counts[perm], kind="stable")]


@dataclass
class ThreeViewConstraintResult:
    verdicts: np.ndarray     # [n] u32 (RS_TVC_*)
    poses: np.ndarray        # [n][2][3][4] CameraToCamera first view -> second / third; rows of refused constraints are zero
    stats: np.ndarray        # [n][RS_TVC_STATS] u32

    def scale(self, i, which=_lib.RS_TVC_S_FINAL_SCALE):
        return _lib.stat_f64(self.stats[i], which)


class ThreeViewConstraints:
    """The three-view constraints on the context (and stream) of an EssentialConsensus, so that a batch queues behind that
    object's other calls."""

    def __init__(self, consensus):
        self._cons = consensus

    @staticmethod
    def params(**kw):
        """rs_three_view_constraint_params: the reference's defaults (cv-sfm/src/settings.rs:332-338, 465-483) with `kw` on top."""
        return _lib.params(_lib.ThreeViewConstraintParams, "rs_three_view_constraint_params_default", **kw)

    def batch_device(self, d_kps, cap_per_img, n_blocks, d_poses, cam, d_views, d_lm_start, d_lm, n_lm, n_constraints, params,
                     d_pose_out, d_verdict, d_stats, stream_to_wait=None):
        """rs_three_view_constraint_batch_device: d_* and stream_to_wait as _device.arg / wait take them.  Enqueues on the
        consensus' stream and returns; its sync() waits."""
        call("rs_three_view_constraint_batch_device", self._cons._h, d_kps, cap_per_img, n_blocks, d_poses, cam, d_views, d_lm_start,
             d_lm, n_lm, n_constraints, params, d_pose_out, d_verdict, d_stats, _device.wait(stream_to_wait))

    def run_tensors(self, torch, kps, poses, cam, views, lm_start, lm, params=None):
        """One batch from torch tensors on the device: kps [n_blocks][cap] keypoints (uint8 [n_blocks][cap][28] as
        akz_extract_batch_device leaves them), poses [n_blocks][12] float64, views [n][3], lm_start [n + 1] and lm [n_lm][3]
        int32 (read as u32).  Enqueues the device call and returns without waiting -> (verdicts [n] int32, poses [n][24]
        float64, stats [n][RS_TVC_STATS] int32) on the device, complete on the consensus' stream: what
        pose_graph.PoseGraph.edges takes."""
        n, n_blocks, n_lm = int(views.shape[0]), int(kps.shape[0]), int(lm.shape[0])
        if lm_start.numel() != n + 1 or poses.numel() != 12 * n_blocks or poses.dtype != torch.float64:
            raise ValueError("lm_start is [n + 1], poses [n_blocks][12] float64")
        _device.require_device(kps, poses, views, lm_start, lm)
        cap = kps.numel() * kps.element_size() // (28 * n_blocks)
        dev = kps.device
        d_pose = torch.zeros((max(n, 1), 24), dtype=torch.float64, device=dev)
        d_out = torch.zeros((max(n, 1), 1 + _lib.RS_TVC_STATS), dtype=torch.int32, device=dev)
        d_verdict, d_stats = d_out[:, 0].contiguous(), d_out[:, 1:].contiguous()
        self.batch_device(kps, cap, n_blocks, poses, cam, views, lm_start, lm if n_lm else None, n_lm, n, params or self.params(),
                          d_pose, d_verdict, d_stats, torch.cuda.current_stream(dev))
        return d_verdict[:n], d_pose[:n], d_stats[:n]

    def run(self, torch, kps, poses, cam, views, lm_start, lm, params=None):
        """run_tensors, waits.  -> ThreeViewConstraintResult (host arrays)."""
        d_verdict, d_pose, d_stats = self.run_tensors(torch, kps, poses, cam, views, lm_start, lm, params)
        self._cons.sync()
        return ThreeViewConstraintResult(_device.host_u32(d_verdict), d_pose.cpu().numpy().reshape(-1, 2, 3, 4),
                                         _device.host_u32(d_stats))
