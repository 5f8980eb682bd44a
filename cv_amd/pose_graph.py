"""Host-side mirror of the relaxation of cv-sfm's pose graph over rs_pose_graph_edges_device and
rs_pose_graph_relax_batch_device of include/akz.h.

  ThreeViewConstraint::edge_constraints               cv-sfm/src/lib.rs:167-180
  VSlam::constrain_view                               cv-sfm/src/lib.rs:1892-1936
  apply_constraints / compute_momentum_bundle_adjust  cv-sfm/src/lib.rs:2358-2414
  flatten_constraints                                 cv-sfm/src/lib.rs:2519-2532

One wavefront per view and round on the device (cv_amd/csrc/rs_pose_graph.hip); there is no CPU fallback.  The chain
ThreeViewConstraints.run_tensors -> PoseGraph.edges -> PoseGraph.relax -> Registration.triangulate keeps every array on
the device (relax waits and brings the verdicts to the host; relax_batch_device only enqueues on rs_stream()).
flatten_constraints walks a HashMap in the reference, which defines no order of a view's edges: `flatten` builds one
admissible order on the host.
"""
from dataclasses import dataclass

import numpy as np

from . import _device, _lib
from ._device import call

VERDICTS = ("ok", "few_views", "nonfinite", "bad_index")
VIEW_STATES = ("updated", "no_constraint", "nonfinite")
SLOT_TARGET = (0, 0, 1, 1, 2, 2)     # edge slot s of a constraint: its target is the constraint's view SLOT_TARGET[s],
SLOT_OTHER = (2, 1, 0, 2, 1, 0)      # its other view SLOT_OTHER[s] (lib.rs:167-180)


def flatten(views, n_views, order=None):
    """(row_start [n_views + 1], row_edges [6 n]) u32 from the constraints' view triples `views` [n][3]: view v's row holds the
    edge ids 6 * constraint + slot whose target is v, constraint index ascending, slot order within a constraint — THE
    documented admissible order.  `order` (a permutation of range(n)) walks the constraints in another order instead.  A
    refused constraint's entries stay in the rows: the device skips them through the constraint's verdict.  A triple with a
    view >= n_views raises ValueError."""
    views = np.asarray(views, np.int64).reshape(-1, 3)
    walk = np.arange(len(views)) if order is None else np.asarray(order, np.int64)
    if sorted(walk.tolist()) != list(range(len(views))):
        raise ValueError("order must be a permutation of the constraints")
    if views.size and (views.min() < 0 or views.max() >= n_views):
        raise ValueError("a constraint names a view outside [0, n_views)")
    rows = [[] for _ in range(n_views)]
    for c in walk.tolist():
        for slot in range(6):
            rows[int(views[c, SLOT_TARGET[slot]])].append(6 * c + slot)
    row_start = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint32)
    row_edges = np.array([e for r in rows for e in r], np.uint32)
    return row_start, row_edges


@dataclass
class PoseGraphResult:
    verdicts: np.ndarray      # [n_graphs] u32 (RS_PG_*)
    view_states: np.ndarray   # [n_views] u32 (RS_PG_VIEW_*); views of a refused graph or of none: 0xFFFFFFFF
    stats: np.ndarray         # [n_graphs][RS_PG_STATS] u32
    poses: object             # what was handed in: the relaxed table, in place (a torch tensor) or a new numpy array

    def rounds(self, g=0):
        return int(self.stats[g, _lib.RS_PG_S_ROUNDS])


class PoseGraph:
    """The pose-graph relaxation on the context (and stream) of an EssentialConsensus, so that it queues behind that
    object's constraint calls."""

    def __init__(self, consensus):
        self._cons = consensus

    @staticmethod
    def params(**kw):
        """rs_pose_graph_params: the reference's defaults (cv-sfm/src/settings.rs:461-463, 477-479) with `kw` on top."""
        return _lib.params(_lib.PoseGraphParams, "rs_pose_graph_params_default", **kw)

    def resident_views(self, views=_lib.RS_PG_DEFAULT_RESIDENT_VIEWS):
        """parity tap: graphs of more than `views` views (at most RS_PG_RESIDENT_VIEWS) take the swept form from now on (0:
        every graph; a limit of at most 8 holds for the call's views in all); without an argument: the default again"""
        call("rs_pose_graph_debug_resident_views", self._cons._h, views)

    def edges_device(self, d_views, d_constraint_poses, d_constraint_verdict, n_constraints, d_edges, stream_to_wait=None):
        """rs_pose_graph_edges_device: d_* and stream_to_wait as _device.arg / wait take them.  Enqueues and returns."""
        call("rs_pose_graph_edges_device", self._cons._h, d_views, d_constraint_poses, d_constraint_verdict, n_constraints, d_edges,
             _device.wait(stream_to_wait))

    def relax_batch_device(self, d_poses, n_views, d_graph_start, n_graphs, d_row_start, d_row_edges, n_rows, d_views,
                           d_constraint_verdict, d_edges, n_constraints, params, d_graph_verdict, d_view_state, d_stats,
                           stream_to_wait=None):
        """rs_pose_graph_relax_batch_device: d_* and stream_to_wait as _device.arg / wait take them.  Enqueues on the consensus'
        stream and returns; its sync() waits."""
        call("rs_pose_graph_relax_batch_device", self._cons._h, d_poses, n_views, d_graph_start, n_graphs, d_row_start, d_row_edges,
             n_rows, d_views, d_constraint_verdict, d_edges, n_constraints, params, d_graph_verdict, d_view_state, d_stats,
             _device.wait(stream_to_wait))

    def rows_device(self, d_views, n_constraints, n_views, d_row_start, d_row_edges, d_flags, stream_to_wait=None):
        """rs_pose_graph_rows_device: `flatten` with order=None on the device; d_* and stream_to_wait as _device.arg / wait take them.
        Enqueues and returns."""
        call("rs_pose_graph_rows_device", self._cons._h, d_views, n_constraints, n_views, d_row_start, d_row_edges, d_flags,
             _device.wait(stream_to_wait))

    def rows(self, torch, views, n_views):
        """rows_device on a device tensor views [n][3] (4-byte integers).  Enqueued behind the current torch stream; no wait ->
        (d_row_start [n_views + 1], d_row_edges [6 n], d_flags [1]) int32: d_flags is 1 when a triple named a view >= n_views
        (it is in no row then)."""
        dev = views.device
        n = int(np.prod(views.shape)) // 3
        d_row_start = torch.zeros((n_views + 1,), dtype=torch.int32, device=dev)
        d_row_edges = torch.zeros((max(6 * n, 1),), dtype=torch.int32, device=dev)
        d_flags = torch.zeros((1,), dtype=torch.int32, device=dev)
        self.rows_device(views, n, n_views, d_row_start, d_row_edges, d_flags, torch.cuda.current_stream(dev))
        return d_row_start, d_row_edges[:6 * n], d_flags

    def edges(self, torch, views, constraints, device=0):
        """The edge table [n][6][12] float64 on the device of the constraints (views [n][3], and `constraints`: a
        three_view.ThreeViewConstraintResult or a pair (poses [n][24] float64, verdicts [n])) — numpy arrays or torch device
        tensors.  Enqueued behind the current torch stream; no wait.  -> (d_edges, the tensors it was made from), which relax()
        takes as `edges`."""
        poses, verdicts = (constraints.poses, constraints.verdicts) if hasattr(constraints, "verdicts") else constraints
        dev = views.device if isinstance(views, torch.Tensor) else torch.device("cuda", device)
        d_views, d_poses, d_verdicts = (_device.tensor(torch, a, dt, dev)
                                        for a, dt in ((views, np.uint32), (poses, np.float64), (verdicts, np.uint32)))
        n = int(np.prod(views.shape)) // 3
        d_edges = torch.zeros((max(n, 1), 6, 12), dtype=torch.float64, device=dev)
        self.edges_device(d_views, d_poses, d_verdicts, n, d_edges, torch.cuda.current_stream(dev))
        if d_poses is not poses:                         # an upload nobody else holds; the tuple holds the other two for relax()
            _device.keep_alive(self._cons, d_poses)
        return d_edges, (d_views, d_verdicts, n)

    def relax(self, torch, poses, graph_start, row_start, row_edges, edges, params=None, device=0):
        """One batch: poses [n_views][12] float64 (a torch device tensor is relaxed in place; a numpy array is copied up and
        the result copied back), graph_start [n_graphs + 1], row_start [n_views + 1], row_edges (see `flatten`) as numpy arrays
        or int32 device tensors, `edges` what edges() returned.  Runs the device call, WAITS for it and copies verdicts, view
        states and stats to the host -> PoseGraphResult.  A chain that must not stop at the host goes through
        relax_batch_device, which enqueues and returns."""
        d_edges, (d_views, d_verdicts, n_constraints) = edges
        dev = d_edges.device
        in_place = isinstance(poses, torch.Tensor)
        d_poses = _device.tensor(torch, poses, np.float64, dev)
        n_views = int(np.prod(poses.shape)) // 12
        n_graphs, n_rows = int(np.prod(graph_start.shape)) - 1, int(np.prod(row_edges.shape))
        if int(np.prod(row_start.shape)) != n_views + 1 or n_graphs < 0:
            raise ValueError("row_start is [n_views + 1], graph_start [n_graphs + 1]")
        d_gs, d_rs, d_re = (_device.tensor(torch, a, np.uint32, dev) for a in (graph_start, row_start, row_edges))
        d_out = torch.full((max(n_graphs, 1) * (1 + _lib.RS_PG_STATS) + max(n_views, 1),), -1, dtype=torch.int32, device=dev)
        d_verdict, d_stats, d_state = d_out[:max(n_graphs, 1)], d_out[max(n_graphs, 1):max(n_graphs, 1) * (1 + _lib.RS_PG_STATS)], d_out[max(n_graphs, 1) * (1 + _lib.RS_PG_STATS):]
        self.relax_batch_device(d_poses, n_views, d_gs, n_graphs, d_rs, d_re, n_rows, d_views, d_verdicts, d_edges, n_constraints,
                                params or self.params(), d_verdict, d_state, d_stats, torch.cuda.current_stream(dev))
        self._cons.sync()
        out = _device.host_u32(d_out)
        ng = max(n_graphs, 1)
        return PoseGraphResult(out[:n_graphs].copy(), out[ng * (1 + _lib.RS_PG_STATS):][:n_views].copy(),
                               out[ng:ng * (1 + _lib.RS_PG_STATS)].reshape(ng, _lib.RS_PG_STATS)[:n_graphs].copy(),
                               poses if in_place else d_poses.cpu().numpy().view(np.float64).reshape(-1, 12)[:n_views].copy())
