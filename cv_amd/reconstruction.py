"""Host-side mirror of cv-sfm's optimize_reconstruction over rs_filter_observations_device and
rs_optimize_reconstruction_batch_device of include/akz.h.

  VSlam::optimize_reconstruction            cv-sfm/src/lib.rs:2343-2355
  VSlam::filter_non_robust_observations     cv-sfm/src/lib.rs:2657-2757
  split_landmark / split_observation        cv-sfm/src/lib.rs:2559-2568, 552-588

One lane per landmark decides and an exclusive scan over the observations compacts the table on the device
(cv_amd/csrc/rs_observation_filter.hip); there is no CPU fallback.  ObservationFilter is one pass; ReconstructionOptimizer
chains reconstruction_optimization_iterations rounds of PoseGraph's relaxation and the filter and closes with the world table
of the filtered lists.  The run_tensors methods enqueue and return device tensors — a chain that must not stop at the host
goes on from them (the filtered table as a triangulation.LandmarkTable) —, the run methods wait and copy to the host.
"""
from dataclasses import dataclass

import numpy as np

from . import _device, _lib
from ._device import call, host_u32 as u32
from .covisibility import Covisibility
from .pose_graph import PoseGraph, PoseGraphResult
from .three_view import ThreeViewConstraints
from .triangulation import LandmarkTable, triangulate_landmarks_device

LANDMARK_STATES = ("kept", "single", "pair_split", "no_point", "kicked", "bad_index", "skipped")
VERDICTS = ("ok", "few_landmarks", "bad_range", "skipped")


def stopped_at(verdict):
    """A word of ReconstructionOptimizer's verdicts -> None for a reconstruction that went through, else (round, "relax" or
    "filter", the stage's own verdict: RS_PG_* or RS_OF_*)."""
    v = int(verdict)
    if v == _lib.RS_OR_OK:
        return None
    return (v >> 16) & 0x3FFF, "relax" if (v >> 8) & 0xFF == _lib.RS_OR_STAGE_RELAX else "filter", v & 0xFF


@dataclass
class ObservationFilterTensors:
    """What one pass wrote, on the device (rs_filter_observations_device's outputs by their names without d_)."""
    keep: object            # [n_obs] uint8
    lm_state: object        # [n_landmarks] uint8 (RS_OF_*)
    tri_reason: object      # [n_landmarks] uint8
    robust: object          # [n_landmarks] uint8, bits RS_OF_ROBUST_BEFORE / _AFTER
    obs_start_out: object   # [n_landmarks + 1] int32
    obs_out: object         # [n_obs][2] int32, rows [0, counts[0]) written
    split_out: object       # [n_obs][2] int32, rows [0, counts[1]) written
    counts: object          # [2] int32 {kept, split off}
    recon_verdict: object   # [n_recons] int32 (RS_OF_OK ...)
    stats: object           # [n_recons][RS_OF_STATS] int32
    n_landmarks: int
    n_obs: int

    def table(self, torch):
        """the filtered lists as a LandmarkTable over these tensors"""
        return LandmarkTable.from_device(torch, self.obs_start_out, self.obs_out, self.n_landmarks, self.n_obs)


@dataclass
class ObservationFilterResult:
    keep: np.ndarray
    lm_state: np.ndarray
    tri_reason: np.ndarray
    robust: np.ndarray
    obs_start: np.ndarray     # [n_landmarks + 1] the filtered table
    obs: np.ndarray           # [kept][2]
    split: np.ndarray         # [split off][2]: row k is the new single-observation landmark n_landmarks + k
    verdicts: np.ndarray      # [n_recons] u32
    stats: np.ndarray         # [n_recons][RS_OF_STATS] u32
    tensors: object           # the ObservationFilterTensors it was read from


class ObservationFilter:
    """The filter on the context (and stream) of an EssentialConsensus, so that it queues behind that object's other calls."""

    def __init__(self, consensus):
        self._cons = consensus

    @staticmethod
    def params(**kw):
        """rs_observation_filter_params: the reference's defaults (cv-sfm/src/settings.rs:324-350, 429-431) with `kw` on top;
        `triangulate` takes a whole rs_triangulate_params (triangulation.make_params)."""
        return _lib.params(_lib.ObservationFilterParams, "rs_observation_filter_params_default", **kw)

    def filter_device(self, d_kps, cap, n_blocks, d_poses, cam, d_obs_start, d_obs, n_obs, n_landmarks, d_recon_start, d_view_start, n_recons,
                      d_skip, params, d_keep, d_lm_state, d_tri_reason, d_robust, d_obs_start_out, d_obs_out, d_split_out, d_counts,
                      d_recon_verdict, d_stats, stream_to_wait=None):
        """rs_filter_observations_device: d_* and stream_to_wait as _device.arg / wait take them.  Enqueues and returns."""
        call("rs_filter_observations_device", self._cons._h, d_kps, cap, n_blocks, d_poses, cam, d_obs_start, d_obs, n_obs, n_landmarks,
             d_recon_start, d_view_start, n_recons, d_skip, params, d_keep, d_lm_state, d_tri_reason, d_robust, d_obs_start_out,
             d_obs_out, d_split_out, d_counts, d_recon_verdict, d_stats, _device.wait(stream_to_wait))

    @staticmethod
    def _outputs(torch, dev, n_obs, n_landmarks, n_recons, rounds=1):
        z8 = lambda n: torch.zeros((max(n, 1),), dtype=torch.uint8, device=dev)
        z32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)
        return ObservationFilterTensors(z8(n_obs), z8(n_landmarks), z8(n_landmarks), z8(n_landmarks), z32(n_landmarks + 1), z32(max(n_obs, 1), 2),
                                        z32(rounds * max(n_obs, 1), 2), z32(rounds * 2), z32(rounds * max(n_recons, 1)),
                                        z32(rounds * max(n_recons, 1), _lib.RS_OF_STATS), n_landmarks, n_obs)

    def run_tensors(self, torch, table, d_kps, cap, n_blocks, d_poses, cam, recon_start, view_start, skip=None, params=None):
        """One pass over `table` (a LandmarkTable) under d_poses ([n_blocks][12] float64 device tensor): recon_start, view_start
        [n_recons + 1] and skip [n_recons] as numpy arrays or 4-byte device tensors.  Enqueued behind the current torch stream;
        no wait -> ObservationFilterTensors."""
        dev = table.dev
        n_recons = int(np.prod(recon_start.shape)) - 1
        if n_recons < 0 or int(np.prod(view_start.shape)) != n_recons + 1:
            raise ValueError("recon_start and view_start are [n_recons + 1]")
        d_rs, d_vs = _device.tensor(torch, recon_start, np.uint32, dev), _device.tensor(torch, view_start, np.uint32, dev)
        d_skip = None if skip is None else _device.tensor(torch, skip, np.uint32, dev)
        o = self._outputs(torch, dev, table.n_obs, table.n_landmarks, n_recons)
        self.filter_device(d_kps, cap, n_blocks, d_poses, cam, table.d_start, table.d_obs, table.n_obs, table.n_landmarks, d_rs, d_vs,
                           n_recons, d_skip, params or self.params(), o.keep, o.lm_state, o.tri_reason, o.robust, o.obs_start_out,
                           o.obs_out, o.split_out, o.counts, o.recon_verdict, o.stats, torch.cuda.current_stream(dev))
        return _device.keep_alive(o, d_rs, d_vs, d_skip)

    def run(self, torch, table, d_kps, cap, n_blocks, d_poses, cam, recon_start, view_start, skip=None, params=None):
        """run_tensors, then WAITS and copies to the host -> ObservationFilterResult."""
        o = self.run_tensors(torch, table, d_kps, cap, n_blocks, d_poses, cam, recon_start, view_start, skip, params)
        self._cons.sync()
        return _to_host(o, int(np.prod(recon_start.shape)) - 1)


def _to_host(o, n_recons, rnd=0):
    counts = u32(o.counts).reshape(-1, 2)[rnd]
    room = max(o.n_obs, 1)
    return ObservationFilterResult(
        o.keep.cpu().numpy()[:o.n_obs], o.lm_state.cpu().numpy()[:o.n_landmarks], o.tri_reason.cpu().numpy()[:o.n_landmarks],
        o.robust.cpu().numpy()[:o.n_landmarks], u32(o.obs_start_out), u32(o.obs_out)[:counts[0]],
        u32(o.split_out)[rnd * room:rnd * room + counts[1]], u32(o.recon_verdict)[rnd * max(n_recons, 1):][:n_recons],
        u32(o.stats).reshape(-1, max(n_recons, 1), _lib.RS_OF_STATS)[rnd][:n_recons], o)


@dataclass
class ReconstructionResult:
    verdicts: np.ndarray      # [n_graphs] u32: RS_OR_OK or where a reconstruction stopped (stopped_at)
    pose_graph: object        # pose_graph.PoseGraphResult of the last round each reconstruction was relaxed in
    filter: object            # ObservationFilterResult of the last round (verdicts and stats: that round's)
    world: object             # device tensor [n_landmarks][4] float64 of the final table, or None
    world_reason: object      # device tensor [n_landmarks] uint8, or None
    tensors: object           # ObservationFilterTensors holding every round's verdicts, stats, counts and split lists


class ReconstructionOptimizer:
    """optimize_reconstruction for many reconstructions at once, chained on top of a PoseGraph (and on its context)."""

    def __init__(self, pose_graph):
        self._pg = pose_graph
        self._cons = pose_graph._cons

    params = staticmethod(ObservationFilter.params)

    def optimize_device(self, d_poses, n_views, d_graph_start, n_graphs, d_row_start, d_row_edges, n_rows, d_views, d_constraint_verdict,
                        d_edges, n_constraints, pg_params, d_kps, cap, cam, d_obs_start, d_obs, n_obs, n_landmarks, d_recon_start, params,
                        d_verdict, d_graph_verdict, d_view_state, d_pg_stats, d_keep, d_lm_state, d_tri_reason, d_robust, d_obs_start_out,
                        d_obs_out, d_split_out, d_counts, d_recon_verdict, d_of_stats, d_world=None, d_world_reason=None, stream_to_wait=None):
        """rs_optimize_reconstruction_batch_device: d_* and stream_to_wait as _device.arg / wait take them.  Enqueues and returns."""
        call("rs_optimize_reconstruction_batch_device", self._cons._h, d_poses, n_views, d_graph_start, n_graphs, d_row_start,
             d_row_edges, n_rows, d_views, d_constraint_verdict, d_edges, n_constraints, pg_params, d_kps, cap, cam, d_obs_start, d_obs,
             n_obs, n_landmarks, d_recon_start, params, d_verdict, d_graph_verdict, d_view_state, d_pg_stats, d_keep, d_lm_state,
             d_tri_reason, d_robust, d_obs_start_out, d_obs_out, d_split_out, d_counts, d_recon_verdict, d_of_stats, d_world,
             d_world_reason, _device.wait(stream_to_wait))

    def run_tensors(self, torch, poses, graph_start, row_start, row_edges, edges, table, d_kps, cap, cam, recon_start, pg_params=None,
                    params=None, world=True):
        """poses [n_views][12] float64 device tensor (relaxed in place), graph_start / row_start / row_edges as PoseGraph.relax
        takes them, `edges` what PoseGraph.edges returned, `table` the LandmarkTable over the same views' keypoint blocks d_kps.
        Enqueued behind the current torch stream; no wait -> (d_verdict, pose-graph outputs (d_graph_verdict, d_view_state,
        d_pg_stats), ObservationFilterTensors, d_world, d_world_reason)."""
        d_edges, (d_views, d_verdicts, n_constraints) = edges
        dev = d_edges.device
        params, pg_params = params or self.params(), pg_params or PoseGraph.params()
        rounds = max(int(params.reconstruction_optimization_iterations), 1)
        n_views = int(np.prod(poses.shape)) // 12
        n_graphs, n_rows = int(np.prod(graph_start.shape)) - 1, int(np.prod(row_edges.shape))
        d_gs, d_rs, d_re, d_recon = (_device.tensor(torch, a, np.uint32, dev) for a in (graph_start, row_start, row_edges, recon_start))
        i32 = lambda *shape: torch.full(shape, -1, dtype=torch.int32, device=dev)
        d_verdict, d_gv, d_state, d_pg_stats = i32(max(n_graphs, 1)), i32(max(n_graphs, 1)), i32(max(n_views, 1)), i32(max(n_graphs, 1), _lib.RS_PG_STATS)
        o = ObservationFilter._outputs(torch, dev, table.n_obs, table.n_landmarks, n_graphs, rounds)
        d_world = table.new_world() if world else None
        d_reason = torch.zeros((max(table.n_landmarks, 1),), dtype=torch.uint8, device=dev) if world else None
        self.optimize_device(poses, n_views, d_gs, n_graphs, d_rs, d_re, n_rows, d_views, d_verdicts, d_edges, n_constraints, pg_params,
                             d_kps, cap, cam, table.d_start, table.d_obs, table.n_obs, table.n_landmarks, d_recon, params, d_verdict,
                             d_gv, d_state, d_pg_stats, o.keep, o.lm_state, o.tri_reason, o.robust, o.obs_start_out, o.obs_out,
                             o.split_out, o.counts, o.recon_verdict, o.stats, d_world, d_reason, torch.cuda.current_stream(dev))
        return d_verdict, (d_gv, d_state, d_pg_stats), _device.keep_alive(o, d_gs, d_rs, d_re, d_recon), d_world, d_reason

    def run(self, torch, poses, graph_start, row_start, row_edges, edges, table, d_kps, cap, cam, recon_start, pg_params=None, params=None,
            world=True):
        """run_tensors, then WAITS and copies verdicts, states and stats to the host -> ReconstructionResult (the world table
        stays on the device, where the registration chain reads it)."""
        params = params or self.params()
        d_verdict, (d_gv, d_state, d_pg_stats), o, d_world, d_reason = self.run_tensors(
            torch, poses, graph_start, row_start, row_edges, edges, table, d_kps, cap, cam, recon_start, pg_params, params, world)
        self._cons.sync()
        n_graphs, n_views = int(np.prod(graph_start.shape)) - 1, int(np.prod(poses.shape)) // 12
        last = max(int(params.reconstruction_optimization_iterations), 1) - 1
        return ReconstructionResult(u32(d_verdict)[:n_graphs], PoseGraphResult(u32(d_gv)[:n_graphs], u32(d_state)[:n_views], u32(d_pg_stats)[:n_graphs], poses),
                                    _to_host(o, n_graphs, last), d_world, d_reason, o)


@dataclass
class RegenerateResult:
    candidates: object        # covisibility.CovisibilityTensors (target verdicts and stats as the record left them)
    constraints: tuple        # (d_verdict, d_pose, d_stats) of the constraint stage over the slots
    recorded: object          # d_recorded [n_slots] int32: the constraints' verdicts the graph saw
    rows: tuple               # (d_row_start, d_row_edges, d_flags)
    verdict: object           # d_verdict [n_graphs] int32 (RS_OR_*)
    pose_graph: tuple         # (d_graph_verdict, d_view_state, d_pg_stats)
    filter: object            # ObservationFilterTensors
    world: object             # [n_landmarks][4] float64 of the filtered table
    world_reason: object      # [n_landmarks] uint8


def regenerate(torch, consensus, table, d_kps, cap, cam, poses, graph_start, recon_start, targets=None, reason=None, cv_params=None,
               tvc_params=None, pg_params=None, params=None):
    """VSlam::regenerate_reconstruction (cv-sfm/src/lib.rs:2418-2435) for the reconstructions of graph_start side by side, on
    device tensors: the covisibility candidates of `targets` (default: every view), their three-view constraints, the record,
    the edges and rows of the pose graph and optimize_reconstruction, each enqueued on the consensus' stream behind the one
    before.  poses [n_views][12] float64 is relaxed in place.  `reason` [n_landmarks] uint8: the robust triangulation's reason
    bytes; computed here under `poses` and params.triangulate when not given.  WAITS once, at the end -> RegenerateResult of
    device tensors."""
    n_views = int(np.prod(poses.shape)) // 12
    dev = table.dev
    pg = PoseGraph(consensus)
    opt = ReconstructionOptimizer(pg)
    params = params or opt.params()
    if reason is None:
        reason = torch.zeros((max(table.n_landmarks, 1),), dtype=torch.uint8, device=dev)
        first_world = table.new_world()          # the call only enqueues: the table it writes is held until the wait below
        triangulate_landmarks_device(consensus._h, table, d_kps, cap, n_views, poses, cam, params.triangulate, first_world, reason,
                                     torch.cuda.current_stream(dev))
        _device.keep_alive(consensus, first_world)
    targets = np.arange(n_views, dtype=np.uint32) if targets is None else targets
    cov = Covisibility(consensus)
    cv_params = cv_params or cov.params()
    cand = cov.run_tensors(torch, table, cap, n_views, reason, targets, cv_params)
    kps = d_kps.view(torch.uint8).reshape(n_views, cap, 28)
    constraints = ThreeViewConstraints(consensus).run_tensors(torch, kps, poses, cam, cand.views, cand.lm_start, cand.lm, tvc_params)
    recorded = cov.record_tensors(torch, cand, constraints[0], graph_start, cv_params)
    edges = pg.edges(torch, cand.views, (constraints[1], recorded))
    rows = pg.rows(torch, cand.views, n_views)
    d_verdict, pose_graph, o, d_world, d_world_reason = opt.run_tensors(torch, poses, graph_start, rows[0], rows[1], edges, table, d_kps, cap,
                                                                        cam, recon_start, pg_params, params)
    consensus.sync()
    return RegenerateResult(cand, constraints, recorded, rows, d_verdict, pose_graph, o, d_world, d_world_reason)


def merge_reconstructions(torch, consensus, dst_table, src_table, d_kps, cap, cam, d_poses, dst_views, src_views, bridge_block, src_pose, slot,
                          matches, nmatches, final, counts, src_landmarks, best=None, n_world=None, skip=None, **kw):
    """What VSlam::try_merge_reconstructions does behind the bridging frame's add_view (cv-sfm/src/lib.rs:2153-2188:
    the landmark map, incorporate_reconstruction), then regenerate_reconstruction, with ONE wait at the end: merge_map ->
    incorporate -> the robust triangulation of the merged table with (lm_room, obs_room) as its sizes, so that nothing is read
    back -> regenerate with the carried-over views as its targets.  dst_table: the destination after the bridging frame's
    add_views; src_table: the source; dst_views, src_views: (first, end) block ranges of the two reconstructions' views in the
    block pool — they must be adjacent, so that the merged graph is one range of graph_start (ValueError otherwise; renumbering
    blocks is not done here); the bridging frame's block lies in one of them.  src_pose [12]: the bridging frame's pose in the
    source, copied before add_views overwrote its row of d_poses.  slot, matches, nmatches, final, best, n_world: the
    refinement call over the destination that registered the bridging frame and its slot; counts [n_blocks]; src_landmarks
    [n_blocks][cap] the source's per-feature landmark map; skip [n_src_views] (optional) over the source's views in block order
    without the bridging frame's.  A refused record does not loop in here: the caller runs again from the old tables with
    `skip`, as with add_views.  kw: regenerate's parameter arguments.  -> (MergeMapTensors, IncorporateTensors, (world [lm_room][4], reason [lm_room]) of the
    merged table under the incorporated poses, RegenerateResult)."""
    from .reconstruction_merge import ReconstructionMerge
    (d0, d1), (s0, s1) = (int(v) for v in dst_views), (int(v) for v in src_views)
    if not (d0 <= d1 and s0 <= s1 and (d1 == s0 or s1 == d0)):
        raise ValueError("the destination's and the source's view ranges must be adjacent in the block pool")
    lo, hi = min(d0, s0), max(d1, s1)
    if not lo <= bridge_block < hi:
        raise ValueError("the bridging frame's block lies in neither range")
    src_blocks = [b for b in range(s0, s1) if b != bridge_block]
    rm = ReconstructionMerge(consensus)
    merge_map = rm.merge_map_tensors(torch, matches, nmatches, final, cap, slot, counts, src_landmarks, bridge_block, dst_table.n_landmarks,
                                     best=best, n_world=n_world)
    merged = rm.incorporate_tensors(torch, dst_table, src_table, merge_map, d_poses, cap, src_blocks, bridge_block, src_pose, skip=skip)
    table = merged.table(torch)
    params = kw.pop("params", None) or ReconstructionOptimizer.params()
    world = table.new_world()
    reason = torch.zeros((max(table.n_landmarks, 1),), dtype=torch.uint8, device=table.dev)
    rs_stream = torch.cuda.ExternalStream(consensus.stream(), device=table.dev)
    with torch.cuda.stream(rs_stream):                   # the calls below order themselves behind the current torch stream
        triangulate_landmarks_device(consensus._h, table, d_kps, cap, int(d_poses.shape[0]), d_poses, cam, params.triangulate, world, reason,
                                     torch.cuda.current_stream(table.dev))
        result = regenerate(torch, consensus, table, d_kps, cap, cam, d_poses, np.array([lo, hi], np.uint32),
                            np.array([0, merged.lm_room], np.uint32), targets=np.array(src_blocks, np.uint32), reason=reason, params=params, **kw)
    return merge_map, merged, (world, reason), result


@dataclass
class RepackedReconstruction:
    table: object             # repack.RepackTensors: the new table, (lm_room, obs_room) = n_blocks_out * cap as its sizes
    pools: dict               # name -> the pool moved through the map, [n_blocks_out][...]
    pool_verdicts: dict       # name -> d_verdict [1] int32 (RS_RP_*)
    constraints: object       # repack.ConstraintTensors, or None
    world: object             # [lm_room][4] float64: the robust triangulation of the new table under the moved poses
    world_reason: object      # [lm_room] uint8
    regenerate: object        # RegenerateResult, or None


def repack(torch, consensus, table, cap, cam, block_map, n_blocks_out, pools, constraints=None, recon_start=None, constraint_start=None,
           graph_start=None, tri_params=None, **kw):
    """VSlamData::remove_view (cv-sfm/src/lib.rs:517-546) for every view block_map removes ([n_blocks] u32, 0xFFFFFFFF: removed;
    None: the identity), the compaction of the table and the renumbering of rows and blocks, with ONE wait at the end and nothing
    read back in between: the table -> every per-block pool of `pools` (a dict of device tensors [n_blocks][...]; "kps" and
    "poses" are needed, counts, colours, descriptors ride along) -> the constraints (views, poses, verdict) when given -> the
    robust triangulation of the new table under the moved poses.  The rooms are n_blocks_out * cap, whatever the input's sizes
    were: that bounds the table of a chain that never waits.  graph_start [n_graphs + 1] over the NEW blocks: continue into
    regenerate on the new table (kw: its parameter arguments; its own wait is the one wait then).  -> RepackedReconstruction."""
    from .repack import TableRepack
    rp = TableRepack(consensus)
    dev = table.dev
    n_blocks = int(pools["poses"].shape[0])
    first = _device.wait_or_current(torch, None, dev)
    d_map = rp._map(torch, block_map, dev)               # uploaded once: every call below takes the same tensor
    t = rp.table_tensors(torch, table, cap, n_blocks, d_map, n_blocks_out, recon_start=recon_start, stream_to_wait=first)
    moved, verdicts = {}, {}
    for name, pool in pools.items():
        moved[name], verdicts[name] = rp.gather_tensors(torch, pool, d_map, n_blocks_out, stream_to_wait=first)
    cons = None
    if constraints is not None:
        cons = rp.constraints_tensors(torch, *constraints, d_map, n_blocks, n_blocks_out, start=constraint_start, stream_to_wait=first)
    new_table = t.table(torch)
    tri_params = tri_params or ReconstructionOptimizer.params().triangulate
    world = new_table.new_world()
    reason = torch.zeros((max(new_table.n_landmarks, 1),), dtype=torch.uint8, device=dev)
    triangulate_landmarks_device(consensus._h, new_table, moved["kps"], cap, n_blocks_out, moved["poses"], cam, tri_params, world, reason,
                                 torch.cuda.current_stream(dev))
    result = None
    if graph_start is not None:
        rs_stream = torch.cuda.ExternalStream(consensus.stream(), device=dev)
        with torch.cuda.stream(rs_stream):               # regenerate orders itself behind the current torch stream
            result = regenerate(torch, consensus, new_table, moved["kps"], cap, cam, moved["poses"], graph_start,
                                np.array([0, t.lm_room], np.uint32) if recon_start is None else t.recon_start_out, reason=reason, **kw)
    else:
        consensus.sync()
    return RepackedReconstruction(t, moved, verdicts, cons, world, reason, result)


@dataclass
class StartResult:
    consensus: tuple          # (d_pose [slots][12], d_best_id, d_inliers [slots][cap], d_n_inliers) of the two-view consensus
    join: object              # bootstrap.JoinTensors
    bootstrap: tuple          # (d_verdict, d_pose_out [scenes][24], d_combined, d_first_ok, d_second_ok) of the three-view bootstrap
    tv_stats: object          # [scenes][RS_TV_STATS] int32
    start: object             # bootstrap.StartTensors: the new table, maps, ranges and constraint arrays
    first_world: object       # [lm_room][4] float64 of the new table under the bootstrap's poses
    first_reason: object      # [lm_room] uint8
    edges: tuple              # PoseGraph.edges' result over the first constraints
    rows: tuple               # (d_row_start, d_row_edges, d_flags)
    verdict: object           # d_verdict [reconstructions] int32 (RS_OR_*)
    pose_graph: tuple         # (d_graph_verdict, d_view_state, d_pg_stats)
    filter: object            # ObservationFilterTensors
    world: object             # [lm_room][4] float64 of the filtered table
    world_reason: object      # [lm_room] uint8


def start_reconstructions(torch, consensus, d_kps, counts, cap, cam, d_pairs, d_npairs, ia, ib, arrsac_params, scenes, ic, i_first, i_second,
                          n_blocks, view_base, d_kps_dst=None, d_counts_dst=None, d_poses=None, table=None, recon_start=None, view_start=None,
                          skip=None, minimum=_lib.RS_JP_DEFAULT_MINIMUM_ROBUST_MATCHES, shuffle=True, seed=0, consensus_shuffle=True,
                          tv_params=None, pg_params=None, params=None):
    """What VSlam::try_init does (cv-sfm/src/lib.rs:901-990: init_reconstruction, add_reconstruction, optimize_reconstruction) for
    the scenes of a call, with ONE wait at the end: the two-view consensus of the slots (ia[k], ib[k]) over the matcher's d_pairs /
    d_npairs -> the join of the slots scenes[s] = (first, second) -> the three-view bootstrap of the source blocks ic / i_first /
    i_second -> add_reconstruction into the destination pool (d_kps_dst [n_blocks][cap] keypoints, d_counts_dst, d_poses; made
    here when not given) behind `table` (a LandmarkTable with recon_start / view_start, or None) -> the robust triangulation of
    the new table with (lm_room, obs_room) as its sizes, so that nothing is read back -> the edges and rows of the first
    constraints -> optimize_reconstruction over the ranges add_reconstruction wrote.  The consensus needs room for the slots
    (reserve).  counts [n_src_blocks]: the feature counts of d_kps.  -> StartResult of device tensors."""
    from .bootstrap import PairJoin, ReconstructionStart
    from .three_view import ThreeViewInit
    dev = d_pairs.device
    n_slots, n_scenes = len(ia), len(scenes)
    opt = ReconstructionOptimizer(PoseGraph(consensus))
    params, tv_params = params or opt.params(), tv_params or ThreeViewInit.params()
    z = lambda dt, *shape: torch.zeros(shape, dtype=dt, device=dev)
    m = max(n_scenes, 1)
    d_pose, d_best, d_inliers, d_n_inliers = z(torch.float64, n_slots, 12), z(torch.int32, n_slots), z(torch.int32, n_slots, cap), z(torch.int32, n_slots)
    consensus.model_inliers_batch_device(d_kps, d_kps, cap, ia, ib, d_pairs, d_npairs, cam, cam, arrsac_params, d_pose, d_best, d_inliers,
                                         d_n_inliers, shuffle=consensus_shuffle, stream_to_wait=torch.cuda.current_stream(dev))
    join = PairJoin(consensus).join_tensors(torch, d_pairs, d_npairs, d_inliers, d_n_inliers, d_best, d_pose, cap, [a for a, _ in scenes],
                                            [b for _, b in scenes], minimum, shuffle, seed)
    d_tv_verdict, d_pose_out, d_tv_stats = z(torch.int32, m), z(torch.float64, m, 24), z(torch.int32, m, _lib.RS_TV_STATS)
    d_masks = z(torch.uint8, 3, m, cap)
    n_src_blocks = int(np.prod(counts.shape))
    ThreeViewInit(consensus).init_batch_device(d_kps, cap, n_src_blocks, ic, i_first, i_second, cam, join.pose_first, join.pose_second, join.triples,
                                               join.ntriples, join.first_only, join.nfirst, join.second_only, join.nsecond, tv_params, d_pose_out,
                                               d_tv_verdict, d_masks[0], d_masks[1], d_masks[2], d_tv_stats, torch.cuda.current_stream(dev))
    if d_kps_dst is None:
        d_kps_dst = z(torch.uint8, n_blocks, cap, _lib.KP_DTYPE.itemsize)
    d_counts_dst = z(torch.int32, n_blocks) if d_counts_dst is None else d_counts_dst
    d_poses = z(torch.float64, n_blocks, 12) if d_poses is None else d_poses
    start = ReconstructionStart(consensus).add_tensors(torch, join, d_masks[0], d_masks[1], d_masks[2], d_pose_out, d_tv_verdict, ic, i_first,
                                                       i_second, d_kps, counts, cap, d_kps_dst, d_counts_dst, d_poses, view_base, table,
                                                       recon_start, view_start, skip)
    new_table = start.table(torch)
    first_world = new_table.new_world()
    first_reason = z(torch.uint8, max(new_table.n_landmarks, 1))
    triangulate_landmarks_device(consensus._h, new_table, d_kps_dst, cap, n_blocks, d_poses, cam, params.triangulate, first_world, first_reason,
                                 torch.cuda.current_stream(dev))
    pg = opt._pg
    edges = pg.edges(torch, start.views_out, (start.constraint_poses_out, start.constraint_verdict_out))
    rows = pg.rows(torch, start.views_out, n_blocks)
    d_verdict, pose_graph, o, d_world, d_world_reason = opt.run_tensors(torch, d_poses, start.view_start_out, rows[0], rows[1], edges, new_table,
                                                                        d_kps_dst, cap, cam, start.recon_start_out, pg_params, params)
    consensus.sync()
    return StartResult((d_pose, d_best, d_inliers, d_n_inliers), join, (d_tv_verdict, d_pose_out, d_masks[0], d_masks[1], d_masks[2]), d_tv_stats,
                       start, first_world, first_reason, edges, rows, d_verdict, pose_graph, o, d_world, d_world_reason)


def export_reconstruction(torch, consensus, table, world, colors, view_blocks, counts, landmarks, cap, d_poses, path, camera_faces=True,
                          room=None, n_world=None):
    """VSlam::export_reconstruction (cv-sfm/src/lib.rs:2285-2340): the export on rs_stream() behind the current torch stream,
    ONE wait, the copy of the used rows, then the file (rs_write_ply).  table, world, colors, view_blocks, counts, landmarks,
    cap, d_poses, room, n_world: export.ReconstructionExport.export_tensors' arguments.  With a `room` below the number of
    points the file holds the first `room` of them and the result's verdict says so.  -> export.ExportResult."""
    from .export import ReconstructionExport, write_ply
    result = ReconstructionExport(consensus).run_export(torch, table, world, colors, view_blocks, counts, landmarks, cap, d_poses, room=room,
                                                        n_world=n_world)
    write_ply(path, result.xyz, result.rgb, result.n_views, camera_faces)
    return result
