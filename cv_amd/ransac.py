"""Host-side mirror of the two-view geometric-verification call sites over rs_* of include/akz.h.

  camera.calibrate(keypoint)                      cv-pinhole/src/lib.rs:108-117 (plain), :191-202 (K1 distortion)
  consensus.model_inliers(&EightPoint::new(), matches)   akaze/tests/estimate_pose.rs:63-67, tutorial ch5 main.rs:70-72
The reference's `arrsac` sampler is an un-vendored crate; here the minimal samples are an explicit argument
(`sample_idx`, 8 match indices per hypothesis) and every hypothesis is scored on the MI355X.
"""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _device, _lib
from ._device import call
from ._lib import KP_DTYPE


@dataclass
class CameraIntrinsics:
    """cv_pinhole::CameraIntrinsics (focals, principal_point, skew)."""
    focals: tuple
    principal_point: tuple
    skew: float = 0.0
    k1: float = None      # set -> CameraIntrinsicsK1Distortion

    def calibrate(self, keypoints):
        """Pixel keypoints (structured array with x, y) -> [n,3] unit bearings."""
        kps = np.ascontiguousarray(keypoints, dtype=KP_DTYPE)
        intr = np.array([self.focals[0], self.focals[1], self.principal_point[0], self.principal_point[1], self.skew],
                        np.float64)
        out = np.empty((len(kps), 3), np.float64)
        call("rs_calibrate", intr.ctypes.data, int(self.k1 is not None), float(self.k1 or 0.0), kps.ctypes.data, len(kps),
             out.ctypes.data)
        return out


def _estimator_flag(estimator):
    """"eight_point" (EightPoint) -> 0, "five_point" (NisterStewenius) -> RS_ESTIMATOR_FIVE_POINT"""
    if estimator not in ("eight_point", "five_point"):
        raise ValueError(f"estimator must be 'eight_point' or 'five_point', not {estimator!r}")
    return _lib.RS_ESTIMATOR_FIVE_POINT if estimator == "five_point" else 0


class EssentialConsensus:
    """Owns one rs_ctx.  model_inliers() is the batched Consensus::model_inliers for EightPoint."""

    def __init__(self, max_matches=8192, max_hypotheses=16384, device=0):
        self._h = C.c_void_p()
        self.max_hyp = max_hypotheses
        call("rs_create", device, max_matches, max_hypotheses, C.byref(self._h))

    def close(self):
        if self._h:
            _lib.lib().rs_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _exhaustive(self, fn, width, first, second, sample_idx, threshold):
        """The exhaustive single-scene call `fn` of include/akz.h on samples of `width` matches: (pose, inliers, best_id) or None."""
        a = np.ascontiguousarray(first, np.float64); b = np.ascontiguousarray(second, np.float64)
        si = np.ascontiguousarray(sample_idx, np.uint32).reshape(-1, width)
        n = len(a)
        pose = np.empty((3, 4), np.float64); best = C.c_uint32(); ninl = C.c_uint32()
        inl = np.empty(max(n, 1), np.uint32)
        call(fn, self._h, a.ctypes.data, b.ctypes.data, n, si.ctypes.data, len(si), float(threshold), pose.ctypes.data,
             C.byref(best), inl.ctypes.data, n, C.byref(ninl))
        if best.value == 0xFFFFFFFF:
            return None
        return pose, inl[:ninl.value].copy(), best.value

    def model_inliers(self, bearings_a, bearings_b, sample_idx, threshold):
        """Returns (pose [3,4] = [R | t], inlier indices, best_id) or None when no sample gave a model."""
        return self._exhaustive("rs_essential_batch", 8, bearings_a, bearings_b, sample_idx, threshold)

    def five_point_model_inliers(self, bearings_a, bearings_b, sample_idx, threshold):
        """Consensus::model_inliers(&NisterStewenius::new(), ...) with the sampler factored out (rs_five_point_batch):
        sample_idx [n_samples, 5]; the context needs 10 x n_samples hypothesis slots.  Returns (pose [3,4], inlier indices,
        best_id = (10 sample + solution) 4 + pose) or None when no sample gave a model."""
        return self._exhaustive("rs_five_point_batch", 5, bearings_a, bearings_b, sample_idx, threshold)

    def essentials(self, n_samples):
        """(E [n_samples, 10, 3, 3] with b^T E a = 0, unused slots zero; n_solutions [n_samples]) of the last single-scene
        five-point call (rs_debug_essentials)."""
        E = np.zeros((n_samples, 10, 3, 3), np.float64); n = np.zeros(n_samples, np.uint32)
        call("rs_debug_essentials", self._h, E.ctypes.data, n.ctypes.data, n_samples)
        return E, n

    def arrsac_model_inliers(self, bearings_a, bearings_b, threshold, n_hypotheses=8192, seed=0, sample_idx=None,
                             block_size=64, init_blocks=4, max_candidates=1024, bound=True, sprt=True, sprt_delta=0.05,
                             sprt_ratio=1e3, p3p=False, estimations_per_block=0, halve=False, estimator="eight_point"):
        """Arrsac::new(threshold, Xoshiro256PlusPlus::seed_from_u64(seed)).initialization_hypotheses(n)
        .max_candidate_hypotheses(k).model_inliers(&EightPoint::new(), matches) in this library's shape (include/akz.h:
        rs_essential_arrsac).  p3p=True: the same for LambdaTwist (bearings_a = bearings [n,3], bearings_b = world
        points [n,4]; 3-match samples; rs_p3p_arrsac).  estimations_per_block: hypotheses re-sampled from the best
        pose's inliers after every block (.estimations_per_block(e)); halve: the candidate cap halves block by block.
        The context needs room for n_hypotheses + estimations_per_block x ceil(n / block_size) hypotheses.
        estimator="five_point": NisterStewenius instead of EightPoint (RS_ESTIMATOR_FIVE_POINT): n_hypotheses and
        estimations_per_block count 5-match samples, ten hypothesis slots each; sample_idx is [n, 5].
        Returns (pose, inliers, best_id, stats dict) or None."""
        prm = self.make_params(threshold, n_hypotheses, seed, block_size, init_blocks, max_candidates, bound, sprt, sprt_delta,
                               sprt_ratio, estimations_per_block, halve, estimator)
        five = prm.flags & _lib.RS_ESTIMATOR_FIVE_POINT
        if five and p3p:
            raise ValueError("estimator applies to the two-view consensus")
        a = np.ascontiguousarray(bearings_a, np.float64); b = np.ascontiguousarray(bearings_b, np.float64)
        n = len(a)
        si = None
        if sample_idx is not None:
            si = np.ascontiguousarray(sample_idx, np.uint32).reshape(-1, 3 if p3p else (5 if five else 8))
            prm.n_hypotheses = len(si)
        pose = np.empty((3, 4), np.float64); best = C.c_uint32(); ninl = C.c_uint32()
        inl = np.empty(max(n, 1), np.uint32)
        st = _lib.ArrsacStats()
        call("rs_p3p_arrsac" if p3p else "rs_essential_arrsac", self._h, a.ctypes.data, b.ctypes.data, n,
             si.ctypes.data if si is not None else None, prm, pose.ctypes.data, C.byref(best), inl.ctypes.data, n, C.byref(ninl), st)
        if best.value == 0xFFFFFFFF:
            return None
        stats = {"poses": st.poses, "survivors": st.survivors, "blocks": st.blocks,
                 "residuals_evaluated": st.residuals_evaluated, "residuals_exhaustive": st.residuals_exhaustive}
        return pose, inl[:ninl.value].copy(), best.value, stats

    @staticmethod
    def arrsac_samples(seed, n, n_hypotheses, sample_size=8):
        """The minimal samples rs_essential_arrsac (8; 5 with the five-point estimator) / rs_p3p_arrsac (3) draw on the
        device for (seed, n)."""
        out = np.empty((n_hypotheses, sample_size), np.uint32)
        call("rs_arrsac_samples", seed, n, n_hypotheses, sample_size, out.ctypes.data)
        return out

    def p3p_model_inliers(self, bearings, world, sample_idx, threshold):
        """Consensus::model_inliers(&LambdaTwist::new(), ...): bearings [n,3], world [n,4] homogeneous
        (Projective form), sample_idx [n_hyp,3].  Returns (pose [3,4], inliers, best_id) or None."""
        return self._exhaustive("rs_p3p_batch", 3, bearings, world, sample_idx, threshold)

    def poses(self, n_hyp):
        """(poses [n_hyp,4,3,4], ok [n_hyp,4]) of the last single-scene call (rs_debug_poses)."""
        P = np.zeros((n_hyp, 4, 3, 4), np.float64); ok = np.zeros((n_hyp, 4), np.uint32)
        call("rs_debug_poses", self._h, P.ctypes.data, ok.ctypes.data, n_hyp)
        return P, ok

    # ---- micro-batch entry: every frame pair of the matcher's output in one chain of launches ----
    def reserve(self, max_scenes):
        call("rs_batch_reserve", self._h, max_scenes)

    @staticmethod
    def make_params(threshold, n_hypotheses=8192, seed=0, block_size=64, init_blocks=4, max_candidates=1024, bound=True,
                    sprt=True, sprt_delta=0.05, sprt_ratio=1e3, estimations_per_block=0, halve=False, estimator="eight_point"):
        prm = _lib.ArrsacParams()
        prm.struct_size = C.sizeof(_lib.ArrsacParams)
        prm.n_hypotheses, prm.block_size, prm.init_blocks, prm.max_candidates = n_hypotheses, block_size, init_blocks, max_candidates
        prm.flags = ((_lib.RS_PRUNE_BOUND if bound else 0) | (_lib.RS_PRUNE_SPRT if sprt else 0)
                     | (_lib.RS_PRUNE_HALVE if halve else 0) | _estimator_flag(estimator))
        prm.estimations_per_block, prm.reserved = estimations_per_block, 0
        prm.threshold, prm.sprt_delta, prm.sprt_ratio, prm.seed = float(threshold), sprt_delta, sprt_ratio, seed
        return prm

    @staticmethod
    def camera(intr):
        """CameraIntrinsics (or (fx, fy, cx, cy, skew, k1-or-None)) -> rs_camera."""
        if isinstance(intr, CameraIntrinsics):
            intr = (intr.focals[0], intr.focals[1], intr.principal_point[0], intr.principal_point[1], intr.skew, intr.k1)
        c = _lib.Camera()
        c.fx, c.fy, c.cx, c.cy, c.skew = (float(v) for v in intr[:5])
        c.k1, c.use_k1, c.reserved = float(intr[5] or 0.0), int(intr[5] is not None), 0
        return c

    def model_inliers_batch_device(self, d_kps_a, d_kps_b, cap_per_img, ia, ib, d_pairs, d_npairs, cam_a, cam_b, params,
                                   d_pose, d_best_id, d_inliers, d_n_inliers, d_stats=None, shuffle=True, stream_to_wait=None):
        """rs_essential_arrsac_batch_device: d_* and stream_to_wait as _device.arg / wait take them; ia / ib host index lists.
        Enqueues and returns; sync() waits."""
        (a, n), (b, _) = _device.index_list(ia), _device.index_list(ib)
        call("rs_essential_arrsac_batch_device", self._h, d_kps_a, d_kps_b, cap_per_img, a, b, d_pairs, d_npairs, n, cam_a, cam_b,
             params, _lib.RS_BATCH_SHUFFLE if shuffle else 0, d_pose, d_best_id, d_inliers, d_n_inliers, d_stats,
             _device.wait(stream_to_wait))

    def p3p_model_inliers_batch_device(self, d_kps, cap_per_img, ik, d_pairs, d_npairs, d_world, n_world, cam, params, d_pose,
                                       d_best_id, d_inliers, d_n_inliers, d_stats=None, shuffle=True, stream_to_wait=None):
        """rs_p3p_arrsac_batch_device: scene s = (feature of keypoint block ik[s], world point index) pairs; d_world
        [n_world][4] f64 (a scene naming a point >= n_world is refused: no model).  Enqueues and returns; sync() waits."""
        k, n = _device.index_list(ik)
        call("rs_p3p_arrsac_batch_device", self._h, d_kps, cap_per_img, k, d_pairs, d_npairs, n, d_world, n_world, cam, params,
             _lib.RS_BATCH_SHUFFLE if shuffle else 0, d_pose, d_best_id, d_inliers, d_n_inliers, d_stats,
             _device.wait(stream_to_wait))

    def triangulate_inliers(self, d_kps_a, d_kps_b, cap_per_img, ia, ib, d_pairs, d_npairs, cam_a, cam_b, d_pose, d_best_id,
                            d_inliers, d_n_inliers, d_points, d_reason=None, params=None, stream_to_wait=None):
        """rs_triangulate_pairs_batch_device behind model_inliers_batch_device (same arguments, that call's outputs): the
        CameraPoint of every inlier (cv-sfm/src/lib.rs:1023-1029, 1332) -> d_points [scenes][cap_per_img][4] f64, d_reason
        (optional) [scenes][cap_per_img] u8; scenes without a model write nothing.  Enqueues and returns."""
        from .triangulation import make_params
        (a, n), (b, _) = _device.index_list(ia), _device.index_list(ib)
        call("rs_triangulate_pairs_batch_device", self._h, d_kps_a, d_kps_b, cap_per_img, a, b, d_pairs, d_npairs, n, cam_a, cam_b,
             d_pose, d_best_id, d_inliers, d_n_inliers, params or make_params(), d_points, d_reason, _device.wait(stream_to_wait))

    def sync(self):
        call("rs_sync", self._h)
        vars(self).pop("_inputs", None)                  # _device.keep_alive: the stream has been waited for

    def stream(self):
        return _lib.lib().rs_stream(self._h)

    def scene(self, scene, cap):
        """(bearings_a, bearings_b, order) of scene `scene` of the last batched call (rs_debug_scene)."""
        n = C.c_uint32()
        a = np.zeros((cap, 3), np.float64); b = np.zeros((cap, 3), np.float64); o = np.zeros(cap, np.uint32)
        call("rs_debug_scene", self._h, scene, C.byref(n), a.ctypes.data, b.ctypes.data, o.ctypes.data, cap)
        return a[:n.value], b[:n.value], o[:n.value]

    def scene_world(self, scene, cap):
        """(bearings, world points [n][4], order) of scene `scene` of the last rs_p3p_arrsac_batch_device call."""
        n = C.c_uint32()
        a = np.zeros((cap, 3), np.float64); b = np.zeros((cap, 4), np.float64); o = np.zeros(cap, np.uint32)
        call("rs_debug_scene_world", self._h, scene, C.byref(n), a.ctypes.data, b.ctypes.data, o.ctypes.data, cap)
        return a[:n.value], b[:n.value], o[:n.value]

    def far(self, poses, bearings_a, bearings_b, thresh):
        """[n_pose, n] bool: where the device's epipolar-plane bound alone rules a match out (rs_debug_far)."""
        P = np.ascontiguousarray(poses, np.float64).reshape(-1, 12)
        a = np.ascontiguousarray(bearings_a, np.float64).reshape(-1, 3); b = np.ascontiguousarray(bearings_b, np.float64).reshape(-1, 3)
        out = np.zeros((len(P), len(a)), np.uint8)
        call("rs_debug_far", self._h, P.ctypes.data, len(P), a.ctypes.data, b.ctypes.data, len(a), float(thresh), out.ctypes.data)
        return out.astype(bool)

    def residuals(self, poses, bearings_a, bearings_b, paired=False):
        """CameraToCamera::residual of every (pose, match) as the device evaluates it (rs_debug_residuals): [n_pose, n],
        or [n_pose, 2, n] (the pose and its mirror [R | -t]) with paired=True."""
        P = np.ascontiguousarray(poses, np.float64).reshape(-1, 12)
        a = np.ascontiguousarray(bearings_a, np.float64); b = np.ascontiguousarray(bearings_b, np.float64)
        out = np.zeros((len(P), 2, len(a)) if paired else (len(P), len(a)), np.float64)
        call("rs_debug_residuals", self._h, P.ctypes.data, len(P), a.ctypes.data, b.ctypes.data, len(a), int(paired), out.ctypes.data)
        return out

    def counts(self, n_hyp):
        out = np.zeros((n_hyp, 4), np.uint32)
        call("rs_debug_counts", self._h, out.ctypes.data, out.size)
        return out
