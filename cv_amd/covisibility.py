"""Host-side mirror of the covisibility search in front of cv-sfm's three-view constraints over
rs_covisibility_candidates_device and rs_covisibility_record_device of include/akz.h.

  VSlam::view_covisibilities                 cv-sfm/src/lib.rs:2535-2556
  VSlam::generate_view_constraints           cv-sfm/src/lib.rs:2438-2516
  VSlam::record_view_constraints             cv-sfm/src/lib.rs:2092-2109

One workgroup per target view on the device (cv_amd/csrc/rs_covisibility.hip); there is no CPU fallback.  The outputs are the
arrays ThreeViewConstraints.run_tensors reads (views, lm_start, lm), so the chain landmark table -> candidates -> constraints ->
record -> PoseGraph.edges / rows_device -> ReconstructionOptimizer keeps every array on the device: reconstruction.regenerate
does that.  The reference walks HashMaps here; the one admissible order the device fixes is in DESIGN.md §7.
"""
from dataclasses import dataclass

import numpy as np

from . import _device, _lib
from ._device import call

VERDICTS = ("ok", "few_constraints", "bad_index", "no_graph")


@dataclass
class CovisibilityTensors:
    """What a candidates call wrote, on the device (rs_covisibility_candidates_device's outputs by their names without d_)."""
    views: object           # [n_slots][3] int32
    lm_start: object        # [n_slots + 1] int32
    lm: object              # [n_slots * optimization_maximum_landmarks][3] int32
    slot_count: object      # [n_slots] int32
    target_verdict: object  # [n_targets] int32 (RS_CV_*)
    stats: object           # [n_targets][RS_CV_STATS] int32
    targets: object         # [n_targets] the targets, on the device
    limit: int
    n_targets: int
    graph_start: object = None   # [n_graphs + 1] on the device, once record_tensors has run

    @property
    def n_slots(self):
        return self.n_targets * self.limit


class Covisibility:
    """The covisibility search on the context (and stream) of an EssentialConsensus, so that it queues behind that object's
    other calls."""

    def __init__(self, consensus):
        self._cons = consensus

    @staticmethod
    def params(**kw):
        """rs_covisibility_params: the reference's defaults (cv-sfm/src/settings.rs:453-475) with `kw` on top."""
        return _lib.params(_lib.CovisibilityParams, "rs_covisibility_params_default", **kw)

    @staticmethod
    def limit(params):
        """slots per target"""
        return int(params.candidate_limit or params.optimization_maximum_three_view_constraints)

    def candidates_device(self, d_obs_start, d_obs, n_obs, n_landmarks, cap, n_blocks, d_reason, d_targets, n_targets, params, d_views,
                          d_lm_start, d_lm, d_slot_count, d_target_verdict, d_stats, stream_to_wait=None):
        """rs_covisibility_candidates_device: d_* and stream_to_wait as _device.arg / wait take them.  Enqueues and returns."""
        call("rs_covisibility_candidates_device", self._cons._h, d_obs_start, d_obs, n_obs, n_landmarks, cap, n_blocks, d_reason,
             d_targets, n_targets, params, d_views, d_lm_start, d_lm, d_slot_count, d_target_verdict, d_stats,
             _device.wait(stream_to_wait))

    def record_device(self, d_constraint_verdict, d_targets, n_targets, d_graph_start, n_graphs, params, d_recorded, d_target_verdict,
                      d_stats, stream_to_wait=None):
        """rs_covisibility_record_device: d_* and stream_to_wait as _device.arg / wait take them.  Enqueues and returns."""
        call("rs_covisibility_record_device", self._cons._h, d_constraint_verdict, d_targets, n_targets, d_graph_start, n_graphs,
             params, d_recorded, d_target_verdict, d_stats, _device.wait(stream_to_wait))

    def run_tensors(self, torch, table, cap, n_blocks, reason, targets, params=None):
        """The candidates of `targets` (a numpy array or a 4-byte device tensor) over `table` (a triangulation.LandmarkTable)
        with `reason` [n_landmarks] uint8 as rs_triangulate_landmarks_device wrote it.  Enqueued behind the current torch
        stream; no wait -> CovisibilityTensors."""
        dev = table.dev
        params = params or self.params()
        limit = self.limit(params)
        d_targets = _device.tensor(torch, targets, np.uint32, dev)
        n_targets = int(np.prod(targets.shape))
        n_slots = n_targets * limit
        z32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)
        o = CovisibilityTensors(z32(max(n_slots, 1), 3), z32(n_slots + 1), z32(max(n_slots * int(params.optimization_maximum_landmarks), 1), 3),
                                z32(max(n_slots, 1)), z32(max(n_targets, 1)), z32(max(n_targets, 1), _lib.RS_CV_STATS), d_targets, limit,
                                n_targets)
        self.candidates_device(table.d_start, table.d_obs, table.n_obs, table.n_landmarks, cap, n_blocks, reason, d_targets, n_targets,
                               params, o.views, o.lm_start, o.lm, o.slot_count, o.target_verdict, o.stats, torch.cuda.current_stream(dev))
        return o

    def record_tensors(self, torch, candidates, constraint_verdict, graph_start, params=None):
        """The record behind the constraint stage's verdicts [n_slots] of `candidates` (a CovisibilityTensors, whose
        target_verdict and stats are updated in place).  No wait -> d_recorded [n_slots] int32, what PoseGraph.edges and the
        relaxation take as the constraints' verdicts."""
        dev = candidates.views.device
        d_gs = _device.tensor(torch, graph_start, np.uint32, dev)
        d_recorded = torch.zeros((max(candidates.n_slots, 1),), dtype=torch.int32, device=dev)
        self.record_device(constraint_verdict, candidates.targets, candidates.n_targets, d_gs, int(np.prod(graph_start.shape)) - 1,
                           params or self.params(), d_recorded, candidates.target_verdict, candidates.stats,
                           torch.cuda.current_stream(dev))
        candidates.graph_start = d_gs             # a field of what the caller holds: _device.keep_alive's rule
        return d_recorded
