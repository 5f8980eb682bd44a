"""Host-side mirror of cv-geom's Linear-Eigen triangulator and of the landmark table cv-sfm keeps with it, over the
rs_triangulate_* entry points of include/akz.h.

  LinearEigenTriangulator::new().epsilon(e).max_iterations(n)          cv-geom/src/triangulation.rs:45-80
  TriangulatorObservations::triangulate_observations                   cv-geom/src/triangulation.rs:82-130
  TriangulatorObservations::triangulate_observations_to_camera         cv-core/src/triangulation.rs:21-36
  TriangulatorRelative::triangulate_relative                           cv-core/src/triangulation.rs:52-67
  VSlam::triangulate_landmark_robust / triangulate_merged_landmark_robust   cv-sfm/src/lib.rs:2958-3000

Every point is computed on the device (one 4 x 4 eigen-problem per lane, cv_amd/csrc/rs_triangulate.hip); there is no CPU
fallback.  A point is returned in the reference's Projective form [x, y, z, w] (xyz a unit vector, w = 1 / distance) and
`None` where the reference returns None.  LandmarkTable holds a reconstruction's landmark -> observations lists on the
device, so that the world table of the registration chain (cv_amd/registration.py) is made where it is read.
"""
import ctypes as C

import numpy as np

from . import _device, _lib
from ._device import call


def make_params(epsilon=1e-12, max_iterations=1000, robust_minimum_observations=3, n_views=0xFFFFFFFF,
                incidence_minimum_cosine_distance=1e-3):
    """rs_triangulate_params: the triangulator's two settings and are_observations_robust's three (cv-sfm/src/settings.rs:
    344-350; n_views = views of the reconstruction, for min(robust_minimum_observations, views))."""
    p = _lib.TriangulateParams()
    p.struct_size = C.sizeof(_lib.TriangulateParams)
    # (nalgebra reads max_niter == 0 as "no limit"; the device runs RS_TRI_MAX_SWEEPS = 1024 sweeps at the most)
    p.max_sweeps = int(max_iterations) if max_iterations else 0x7FFFFFFF
    p.eps = float(epsilon)
    p.robust_minimum_observations = int(robust_minimum_observations)
    p.n_views = int(n_views)
    p.incidence_minimum_cosine_distance = float(incidence_minimum_cosine_distance)
    return p


class LinearEigenTriangulator:
    """cv_geom::triangulation::LinearEigenTriangulator.  `consensus`: an EssentialConsensus whose context (and stream) the
    calls use; without one the triangulator makes a small context of its own on `device` at the first call."""

    def __init__(self, epsilon=1e-12, max_iterations=1000, consensus=None, device=0):
        self._epsilon, self._max_iterations = float(epsilon), int(max_iterations)
        self._cons, self._device = consensus, device

    @classmethod
    def new(cls, **kw):
        return cls(**kw)

    def epsilon(self, epsilon):
        return LinearEigenTriangulator(epsilon, self._max_iterations, self._cons, self._device)

    def max_iterations(self, max_iterations):
        return LinearEigenTriangulator(self._epsilon, max_iterations, self._cons, self._device)

    def params(self, **kw):
        return make_params(self._epsilon, self._max_iterations, **kw)

    def _handle(self):
        if self._cons is None:
            from .ransac import EssentialConsensus
            self._cons = EssentialConsensus(8, 1, device=self._device)
        return self._cons._h

    def triangulate_observations_with_reason(self, pairs):
        """(point or None, reason byte) for an iterable of (WorldToCamera [3, 4] = [R | t], unit bearing [3])."""
        pairs = list(pairs)
        poses = np.ascontiguousarray([np.asarray(p, np.float64).reshape(12) for p, _ in pairs], np.float64).reshape(-1, 12)
        bearings = np.ascontiguousarray([np.asarray(b, np.float64).reshape(3) for _, b in pairs], np.float64).reshape(-1, 3)
        point = np.empty(4, np.float64)
        reason = C.c_uint8()
        prm = self.params()
        call("rs_triangulate_observations", self._handle(), poses.ctypes.data if len(pairs) else None,
             bearings.ctypes.data if len(pairs) else None, len(pairs), prm, point.ctypes.data, C.byref(reason))
        return (point if reason.value == 0 else None), reason.value

    def triangulate_observations(self, pairs):
        """WorldPoint [4] or None."""
        return self.triangulate_observations_with_reason(pairs)[0]

    def triangulate_observations_to_camera(self, center_bearing, pairs):
        """CameraPoint in the frame of the camera that saw `center_bearing`; pairs = (CameraToCamera [3, 4], bearing)."""
        ident = np.hstack([np.eye(3), np.zeros((3, 1))])
        return self.triangulate_observations([(ident, center_bearing)] + list(pairs))

    def triangulate_relative(self, relative_pose, a, b):
        """CameraPoint of the bearing pair (a, b) under the CameraToCamera pose [3, 4], or None."""
        return self.triangulate_observations_to_camera(a, [(relative_pose, b)])


class LandmarkTable:
    """The landmark -> observations lists of a reconstruction on the device, in CSR form: landmark l is observed by
    obs[start[l] : start[l + 1]], each a {block, feature} pair into the keypoint blocks (the order of a list is the order the
    triangulation walks it in).  Built from per-landmark lists or from ready CSR arrays; `d_obs_counts` is the per-landmark
    observation count hm_landmark_matches_ordered_batch_device sorts by."""

    def __init__(self, torch, lists=None, start=None, obs=None, device=0):
        if lists is not None:
            lens = np.fromiter((len(l) for l in lists), np.int64, len(lists))
            start = np.concatenate([[0], np.cumsum(lens)])
            obs = np.concatenate([np.asarray(l, np.uint32).reshape(-1, 2) for l in lists] + [np.zeros((0, 2), np.uint32)])
        start = np.ascontiguousarray(start, np.int64)
        obs = np.ascontiguousarray(obs, np.uint32).reshape(-1, 2)
        if len(start) < 1 or start[0] != 0 or np.any(np.diff(start) < 0) or start[-1] != len(obs) or len(obs) >= 2 ** 32:
            raise ValueError("start must ascend from 0 to len(obs)")
        self.torch = torch
        self.n_landmarks, self.n_obs = len(start) - 1, len(obs)
        dev = torch.device("cuda", device)
        self.d_start = torch.from_numpy(start.astype(np.uint32).view(np.int32)).to(dev)
        self.d_obs = torch.from_numpy(obs.view(np.int32).copy()).to(dev) if len(obs) else torch.zeros((1, 2), dtype=torch.int32, device=dev)
        self.d_obs_counts = torch.from_numpy(np.diff(start).astype(np.uint32).view(np.int32)).to(dev)
        self.dev = dev

    @classmethod
    def from_device(cls, torch, d_start, d_obs, n_landmarks, n_obs, d_obs_counts=None):
        """A table over arrays that are on the device already (reconstruction.ObservationFilter's filtered table): d_start
        [n_landmarks + 1] and d_obs [n_obs][2], 4-byte integer tensors that are kept, not copied.  n_obs is the room of d_obs; how
        many rows the table fills is d_start[n_landmarks], known on the device.  Nothing is brought to the host, so nothing is
        validated here: the kernels refuse a list that leaves [0, n_obs].  d_obs_counts [n_landmarks] (optional): the row lengths
        where the producer wrote them (landmark_table.AddViewsTensors); computed from d_start on the current torch stream
        otherwise."""
        _device.require_device(d_start, d_obs, itemsize=4)
        if d_start.numel() < n_landmarks + 1 or d_obs.numel() < 2 * n_obs:
            raise ValueError("d_start is [n_landmarks + 1], d_obs [n_obs][2]")
        t = cls.__new__(cls)
        t.torch, t.n_landmarks, t.n_obs, t.dev = torch, int(n_landmarks), int(n_obs), d_start.device
        t.d_start, t.d_obs = d_start, d_obs
        if d_obs_counts is not None:
            t.d_obs_counts = d_obs_counts
        else:
            t.d_obs_counts = (d_start.view(torch.int32)[1:n_landmarks + 1] - d_start.view(torch.int32)[:n_landmarks]).contiguous()
        return t

    def new_world(self, extra_rows=0):
        """A world table of n_landmarks + extra_rows rows, every row "None"."""
        w = self.torch.zeros((self.n_landmarks + extra_rows, 4), dtype=self.torch.float64, device=self.dev)
        w[:, 3] = -1.0
        return w


def triangulate_landmarks_device(handle, table, d_kps, cap, n_blocks, d_poses, cam, params, d_world, d_reason=None,
                                 stream_to_wait=None):
    """rs_triangulate_landmarks_device: rows [0, table.n_landmarks) of d_world; d_* and stream_to_wait as _device.arg / wait take them.
    Enqueues on the context's stream and returns."""
    call("rs_triangulate_landmarks_device", handle, d_kps, cap, n_blocks, d_poses, cam, table.d_start, table.d_obs, table.n_obs,
         table.n_landmarks, params, d_world, d_reason, _device.wait(stream_to_wait))


def triangulate_merged_device(handle, table, d_kps, cap, n_blocks, d_poses, cam, params, d_best, d_decision, d_merge_ok, n_frames,
                              n_world, d_world, d_reason=None, stream_to_wait=None):
    """rs_triangulate_merged_device: rows n_world + f * cap + j of d_world for the admitted merge candidates."""
    call("rs_triangulate_merged_device", handle, d_kps, cap, n_blocks, d_poses, cam, table.d_start, table.d_obs, table.n_obs,
         table.n_landmarks, params, d_best, d_decision, d_merge_ok, n_frames, n_world, d_world, d_reason, _device.wait(stream_to_wait))
