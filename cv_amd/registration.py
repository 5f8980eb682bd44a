"""Host-side mirror of cv-sfm's frame registration against recent views, for a micro-batch of new frames, device-resident.

  VSlam::add_frame -> hasher.hash_bag(descriptors)                              cv-sfm/src/lib.rs:672
  register_frame_subset: descriptor_features.knn(descriptor, 3) per view match  cv-sfm/src/lib.rs:1462-1486 (up to 32 views,
                                                                                settings.rs:449-450 tracking_recent_frames)
  landmark dedup, three best, unique-match / merge decision                     cv-sfm/src/lib.rs:1489-1532
  duplicate-landmark filter, FeatureWorldMatch list                             cv-sfm/src/lib.rs:1549-1604
  single_view_consensus.model_inliers(&LambdaTwist, matches_3d)                 cv-sfm/src/lib.rs:1619-1622
                                                                                (vslam-sandbox/src/main.rs:105-111: Arrsac,
                                                                                16384 hypotheses, 1024 candidates, 256 per block)

The reference walks this per feature on the CPU; here one call enqueues, for ALL frames of a micro-batch,
hm_hash_bag_device -> hm_knn_batch_device (k = 3, frames x views problems) -> hm_best_of_views_batch_device ->
hm_landmark_matches_batch_device -> rs_p3p_arrsac_batch_device (and, with refine(), hm_landmark_original_matches_batch_device ->
rs_refine_poses_batch_device: the single-view optimiser and consistency filter of cv-sfm/src/lib.rs:1625-1775) on the blocks where akz_extract_batch_device left them; nothing
returns to the host in between.  Which views a frame is matched against is decided on the device too
(cv_amd/place_recognition.py: FrameIndex.find over the hashes this chain writes), and match_found() takes that answer where it
lies: hm_view_plan_device picks one found reconstruction's views per frame (try_localize's turn, cv-sfm/src/lib.rs:858-891, or
the reconstruction try_localize_and_incorporate names, :926-939) and hm_knn_planned_batch_device /
hm_best_of_views_planned_batch_device plan their searches from the device lists — no wait, no copy.  match_views() with
view_blocks' host list stays for callers with lists of their own.  What stays with the caller is the reference's control plane
over that answer (try_localize's loop over the turns, expressed as `pick`).  Which landmark each stored feature observes, which features observe each landmark (a LandmarkTable) and the row
lengths come from the device too: add_views() behind refine() is VSlamData::add_view for the accepted frames of the
micro-batch (cv-sfm/src/lib.rs:432-483, merge_landmarks :699-721) and leaves the next generation of the table, the landmark
map match_views() reads and the counts consensus() sorts by where the next call takes them; sharing_view() behind
match_views() is the graph test are_landmarks_sharing_view (:1435-1449) for the merge candidates (decision 2), whose mask
triangulate_merged() and consensus() take (cv_amd/landmark_table.py; add_views_and_regenerate there chains refine ->
add_views -> triangulate -> regenerate with one wait).  A caller may still hand in a mask of its own.  The table of
triangulated landmarks is made on the device from the poses and the observation lists: triangulate() for the rows indexed
by landmark key, triangulate_merged() between match_views() and consensus() for the rows of the merge candidates
(cv-sfm/src/lib.rs:1590-1593, 2958-3000); a caller may still bring a table of its own.  There is no CPU fallback.
"""
import numpy as np

from . import _device, _lib
from ._device import call
from .knn import Matcher
from .landmark_table import LandmarkUpdate
from .ransac import EssentialConsensus
from .single_view import RefineOutputs, SingleViewRefiner
from . import triangulation


class Registration:
    """The chain for micro-batches of up to `max_frames` frames against up to `n_views` views each (feature blocks of
    `cap` entries).  The consensus parameters default to vslam-sandbox's single-view consensus."""

    def __init__(self, torch, cap, max_frames, n_views, codewords, camera, device=0, threshold=1e-5, n_hypotheses=16384,
                 max_candidates=1024, estimations_per_block=256, block_size=64, better_by=24, seed=0, max_matches=None):
        self.torch = torch
        self.dev = torch.device("cuda", device)
        self.cap, self.F, self.V, self.k = cap, max_frames, n_views, 3
        self.better_by = better_by
        cw = np.ascontiguousarray(codewords, np.uint8).reshape(-1, 64)
        if len(cw) == 0 or len(cw) % 32:
            raise ValueError("the codeword count must be a positive multiple of 32")
        self.n_codewords = len(cw)
        self.d_codewords = torch.from_numpy(cw).to(self.dev)
        # (bulk work: least urgent, so that the consensus' chain of small launches — most urgent, rs_create — finds compute units)
        self.matcher = Matcher(max(cap, self.n_codewords), device=device, low_priority=True)
        n_max = max_matches or cap
        blocks = (n_max + block_size - 1) // block_size
        self.cons = EssentialConsensus(n_max, n_hypotheses + estimations_per_block * blocks, device=device)
        self.cons.reserve(max_frames)
        self.prm = self.cons.make_params(threshold, n_hypotheses=n_hypotheses, seed=seed, block_size=block_size, init_blocks=1,
                                         max_candidates=max_candidates, halve=True, sprt=True,
                                         estimations_per_block=estimations_per_block)
        self.cam = self.cons.camera(camera)
        self.tri_prm = triangulation.make_params()       # LinearEigenTriangulator::new(), cv-sfm's robustness defaults
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=self.dev)
        F, V, k = max_frames, n_views, self.k
        self.hash = z((F, self.n_codewords // 8), torch.uint8)
        self.words = z((F, cap, 2), torch.int32)
        self.knn = z((F, V, cap, k, 2), torch.int32)
        # What the consensus reads and writes exists twice: call t + 1's matching (matcher stream) then overlaps call t's
        # consensus (its own stream); a set is reused only after the consensus that read it has finished (event).
        self._sets = [dict(best=z((F, cap, 3, 2), torch.int32), decision=z((F, cap), torch.int32), pairs=z((F, cap, 2), torch.int32),
                           npairs=z((F,), torch.int32), pose=z((F, 12), torch.float64), best_id=z((F,), torch.int32),
                           inliers=z((F, cap), torch.int32), n_inliers=z((F,), torch.int32), stats=z((F, 32), torch.uint8),
                           originals=z((F, cap, 2), torch.int32), noriginals=z((F,), torch.int32), merge_ok=z((F, cap), torch.uint8),
                           refined=RefineOutputs(z((F, 12), torch.float64), z((F,), torch.int32), z((F, cap), torch.uint8),
                                                 z((F,), torch.int32), z((F, _lib.RS_SV_STATS), torch.int32)),
                           done=torch.cuda.Event(), used=False) for _ in range(2)]
        self.refiner = SingleViewRefiner(self.cons)
        self.sv_prm = self.refiner.params()              # the reference's single-view defaults
        self.landmarks = LandmarkUpdate(self.cons)
        self._calls = 0
        self._hm_s = torch.cuda.ExternalStream(self.hm_stream(), device=self.dev)
        self._rs_s = torch.cuda.ExternalStream(self.rs_stream(), device=self.dev)
        self._select(0)

    def _select(self, i):
        for key, val in self._sets[i].items():
            if key not in ("done", "used"):
                setattr(self, key, val)

    def hm_stream(self):
        return _lib.lib().hm_stream(self.matcher.handle)

    def rs_stream(self):
        return self.cons.stream()

    def enqueue(self, d_kps, d_descs, d_counts, frame_blocks, view_blocks, d_landmarks, d_world, n_world, stream_to_wait=None,
                shuffle=None, d_merge_ok=None, d_obs_counts=None):
        """match_views() followed by consensus(): the whole chain in one go (see the two for the arguments).  With
        d_obs_counts the consensus sees the matches in register_frame_subset's own order (cv-sfm/src/lib.rs:1561-1574)."""
        self.match_views(d_descs, d_counts, frame_blocks, view_blocks, d_landmarks, stream_to_wait=stream_to_wait)
        self.consensus(d_kps, d_counts, d_world, n_world, shuffle=shuffle, d_merge_ok=d_merge_ok, d_obs_counts=d_obs_counts)

    def match_views(self, d_descs, d_counts, frame_blocks, view_blocks, d_landmarks, stream_to_wait=None):
        """frame_blocks [F]: block index (into d_descs / d_counts / d_kps, [..][cap] each) of every new frame;
        view_blocks [F][V]: the blocks of the views each frame is matched against; d_landmarks [blocks][cap] int32: the
        landmark key observed by every feature of every stored block.  All d_* are torch tensors on the device.  Enqueues
        hash_bag, the k = 3 searches and the best-of-views decision on the matcher's stream and returns.  Outputs:
        self.hash, self.best / decision (slot = position in frame_blocks) — of THIS call until the next match_views() (two
        output sets alternate)."""
        cur = self._sets[self._calls & 1]
        self._select(self._calls & 1)
        self._calls += 1
        self._cur = cur
        if cur["used"]:
            self._hm_s.wait_event(cur["done"])           # the consensus of two calls ago has read this set's pair lists
        F = len(frame_blocks)
        V = len(view_blocks[0])
        assert F <= self.F and V <= self.V and all(len(v) == V for v in view_blocks)
        fb_p, _ = _device.index_list(frame_blocks)
        fb = self._fb = fb_p[:F]
        iq_p, _ = _device.index_list(np.repeat(fb, V))
        it_p, _ = _device.index_list(view_blocks)
        h = self.matcher.handle
        # hash_bag runs over the frames' blocks where they lie: block b of d_descs -> row b of the hash table of THIS call
        # (the new frames are contiguous in every caller so far: hash the span)
        b0, b1 = min(fb), max(fb) + 1
        assert b1 - b0 <= self.F
        call("hm_hash_bag_device", h, d_descs[b0:b1], d_counts[b0:b1], self.cap, b1 - b0, self.d_codewords, self.n_codewords, self.hash,
             self.words, _device.wait(stream_to_wait))
        self.hash_block0 = b0
        call("hm_knn_batch_device", h, d_descs, d_counts, d_descs, d_counts, self.cap, iq_p, it_p, F * V, self.k, self.knn, None)
        call("hm_best_of_views_batch_device", h, self.knn, d_counts, fb_p, self.cap, it_p, F, V, self.k, d_landmarks, d_counts,
             self.better_by, self.best, self.decision, None)

    def match_found(self, d_descs, d_counts, frame_blocks, found, d_landmarks, pick=None, by_recon=False, stream_to_wait=None):
        """match_views() for the views a FrameIndex.find() found, without the host list: `found` (a FoundFrames whose query f is
        the frame of frame_blocks[f], its find already enqueued on the matcher's stream) goes through
        place_recognition.plan_views — every frame against the views of ONE reconstruction, group 0 or the one `pick` /
        `by_recon` name, at most self.V of them — and the searches and the best-of-views decision are planned on the device
        from that (hm_knn_planned_batch_device, hm_best_of_views_planned_batch_device).  Nothing is waited for and nothing
        copied.  A view key is a block of d_descs.  Outputs as match_views(), and self.plan (a ViewPlan: lists, lengths, verdicts,
        counts); a frame without a list gets no landmark and decision 0 for every feature."""
        from .place_recognition import plan_views
        cur = self._sets[self._calls & 1]
        self._select(self._calls & 1)
        self._calls += 1
        self._cur = cur
        if cur["used"]:
            self._hm_s.wait_event(cur["done"])           # the consensus of two calls ago has read this set's pair lists
        F, V, n_blocks = len(frame_blocks), self.V, int(d_descs.shape[0])
        assert 1 <= F <= self.F and found.verdict.shape[0] == F
        fb_p, _ = _device.index_list(frame_blocks)
        fb = self._fb = fb_p[:F]
        h = self.matcher.handle
        b0, b1 = min(fb), max(fb) + 1
        assert b1 - b0 <= self.F
        call("hm_hash_bag_device", h, d_descs[b0:b1], d_counts[b0:b1], self.cap, b1 - b0, self.d_codewords, self.n_codewords, self.hash,
             self.words, _device.wait(stream_to_wait))
        self.hash_block0 = b0
        plan = self.plan = plan_views(found, V, n_blocks, pick=pick, by_recon=by_recon, matcher=self.matcher)
        call("hm_knn_planned_batch_device", h, d_descs, d_counts, d_descs, d_counts, self.cap, fb_p, plan.view_idx, plan.n_views, F, V, n_blocks,
             plan.exp_blocks, self.k, self.knn, None)
        call("hm_best_of_views_planned_batch_device", h, self.knn, d_counts, fb_p, self.cap, plan.view_idx, plan.n_views, F, V, n_blocks, self.k,
             d_landmarks, d_counts, self.better_by, self.best, self.decision, None)

    def triangulate(self, table, d_kps, d_poses, d_world=None, d_reason=None, params=None, stream_to_wait=None):
        """The world table on the device: row l of d_world = triangulate_landmark_robust(landmark l) (cv-sfm/src/lib.rs:
        2990-3000) for the landmarks of `table` (a triangulation.LandmarkTable), from the keypoint blocks d_kps [blocks][cap]
        and their WorldToCamera poses d_poses [blocks][12] f64.  A row without a robust triangulation is {0, 0, 0, -1}.
        d_world: at least table.n_landmarks rows (default: a new table with room for the merge candidates' rows, all
        "None"); d_reason (optional) [n_landmarks] uint8.  Enqueued on rs_stream() after stream_to_wait (the stream d_kps /
        d_poses were written on); returns d_world.  Pass rs_stream() as consensus()'s stream_to_wait."""
        if d_world is None:
            d_world = table.new_world(self.F * self.cap)
        assert d_world.shape[0] >= table.n_landmarks and d_poses.shape[0] == d_kps.shape[0]
        triangulation.triangulate_landmarks_device(self.cons._h, table, d_kps, self.cap, d_kps.shape[0], d_poses, self.cam,
                                                   params or self.tri_prm, d_world, d_reason, stream_to_wait)
        return d_world

    def triangulate_merged(self, table, d_kps, d_poses, d_merge_ok, d_world, n_world, d_reason=None, params=None):
        """The rows of the merge candidates of the last match_views(): for slot f, feature j with decision 2 and
        d_merge_ok[f][j] != 0, row n_world + f * cap + j of d_world = triangulate_merged_landmark_robust([best0, best1])
        (cv-sfm/src/lib.rs:2958-2972).  Reads self.best / decision where match_views() left them: enqueued on rs_stream()
        behind the matcher's stream, no host step.  d_merge_ok must be complete when this is called (or written on the
        matcher's stream)."""
        F = len(self._fb)
        assert d_world.shape[0] >= n_world + F * self.cap
        triangulation.triangulate_merged_device(self.cons._h, table, d_kps, self.cap, d_kps.shape[0], d_poses, self.cam,
                                                params or self.tri_prm, self.best, self.decision, d_merge_ok, F, n_world, d_world,
                                                d_reason, self.hm_stream())

    def consensus(self, d_kps, d_counts, d_world, n_world, shuffle=None, d_merge_ok=None, stream_to_wait=None, d_obs_counts=None):
        """The duplicate-landmark filter, the FeatureWorldMatch lists and single_view_consensus.model_inliers for the frames of
        the last match_views().  d_world [rows][4] f64: rows [0, n_world) indexed by landmark key.  d_merge_ok [F][cap] uint8
        (optional): the caller's are_landmarks_sharing_view verdicts for the merge candidates (decision 2,
        cv-sfm/src/lib.rs:1521-1531, read from self.decision after match_views()) — non-zero admits ([best0, best1], feature)
        as a match, whose world point is row n_world + f * cap + feature of d_world (triangulate_merged_landmark_robust; d_world
        then has n_world + F * cap rows); stream_to_wait = the stream the mask and those rows were written on.  Without a mask no
        merge candidate becomes a match — equal to the reference exactly when none passes its graph test.
        d_obs_counts [n_world] uint32 (optional): observations of every landmark key — the match lists then leave in the
        reference's order (stable sort by descending observation count, cv-sfm/src/lib.rs:1561-1574) and the consensus takes
        them as they are (shuffle defaults to False); without it the lists are in feature order and shuffled with the seed
        (shuffle defaults to True).  Outputs: self.pairs / npairs, self.pose / best_id / inliers / n_inliers / stats."""
        if shuffle is None:
            shuffle = d_obs_counts is None
        cur, fb = self._cur, self._fb
        fb_p, F = _device.index_list(fb)
        rows = n_world if d_merge_ok is None else n_world + F * self.cap
        assert d_world.shape[0] >= rows
        call("hm_landmark_matches_ordered_batch_device", self.matcher.handle, self.best, self.decision, d_merge_ok, d_obs_counts,
             d_counts, fb_p, self.cap, F, d_world, n_world, self.pairs, self.npairs, _device.wait(stream_to_wait))
        self.cons.p3p_model_inliers_batch_device(d_kps, self.cap, fb, self.pairs, self.npairs, d_world, rows, self.cam, self.prm,
                                                 self.pose, self.best_id, self.inliers, self.n_inliers, self.stats, shuffle=shuffle,
                                                 stream_to_wait=self.hm_stream())
        cur["done"].record(self._rs_s)
        cur["used"] = True
        self._consensus_args = (d_kps, d_counts, d_world, n_world, d_merge_ok, d_obs_counts)

    def refine(self, d_poses, d_obs_start, d_obs, n_landmarks, params=None, stream=None):
        """What register_frame_subset does behind its consensus (cv-sfm/src/lib.rs:1625-1775) for the frames of the last
        consensus(): the original matches — that call's lists before the drop of the matches without a world point, in the same
        order — on the matcher's stream, then the single-view optimiser and consistency filter on rs_stream() behind the
        consensus, no host step.  The landmark table as triangulate() took it: d_poses [blocks][12] float64 the views' poses,
        d_obs_start [n_landmarks + 1] / d_obs [n_obs][2] int32 the observations {block, feature} of every landmark key.  stream:
        the torch stream the table was written on (default: nothing to wait for).  Outputs: self.originals / noriginals and
        self.refined (a single_view.RefineOutputs: pose, verdict, final, n_final, stats) — the pose for the pose graph and the
        final_matches map over self.originals."""
        cur, fb = self._cur, self._fb
        d_kps, d_counts, d_world, n_world, d_merge_ok, d_obs_counts = self._consensus_args
        fb_p, F = _device.index_list(fb)
        call("hm_landmark_original_matches_batch_device", self.matcher.handle, self.best, self.decision, d_merge_ok, d_obs_counts,
             d_counts, fb_p, self.cap, F, n_world, self.originals, self.noriginals, _device.wait(stream))
        self.refiner.refine_tensors(self.torch, d_kps, d_poses, self.cam, d_obs_start, d_obs, n_landmarks, d_world, n_world,
                                    fb, self.originals, self.noriginals, None if d_merge_ok is None else self.best,
                                    self.pose, self.best_id, self.inliers, self.n_inliers, params or self.sv_prm, out=self.refined,
                                    stream_to_wait=self.hm_stream())
        cur["done"].record(self._rs_s)
        return self.refined

    def sharing_view(self, table):
        """are_landmarks_sharing_view (cv-sfm/src/lib.rs:1435-1449) for the merge candidates of the last match_views() over
        `table` (a triangulation.LandmarkTable): self.merge_ok [F][cap] uint8, non-zero where decision 2 names two landmarks of
        the table that share no view.  Reads self.best / decision where match_views() left them: enqueued on rs_stream() behind
        the matcher's stream, no host step.  Returns the mask: hand it to triangulate_merged() and, with rs_stream() as
        stream_to_wait, to consensus()."""
        F = len(self._fb)
        self.landmarks.sharing_view_device(table.d_start, table.d_obs, table.n_obs, table.n_landmarks, self.best, self.decision,
                                           self.cap, F, self.merge_ok, self.hm_stream())
        return self.merge_ok

    def add_views(self, table, d_poses, d_split=None, d_split_count=None, skip=None, obs_room=None, lm_room=None):
        """VSlamData::add_view (cv-sfm/src/lib.rs:432-483) for the frames of the last refine() whose verdict is RS_SV_OK, over
        `table` — the LandmarkTable that refine() read — out of place.  d_poses [blocks][12] float64: the views' poses; the rows
        of the accepted frames are written from the refined poses.  d_split [room][2] / d_split_count [1] (optional): the split
        list of the observation filter that wrote `table`, whose rows become landmarks of one observation.  skip [F] (optional,
        a numpy array or device tensor): non-zero leaves a slot out — the reference's remove_view after a refused
        record_view_constraints is this call again, from `table`, with that slot skipped.  Enqueued on rs_stream() behind the
        refinement; no wait -> landmark_table.AddViewsTensors: table(torch) for the next triangulate() / refine(), landmarks_out
        for the next match_views(), obs_counts_out for the next consensus()."""
        d_kps, d_counts, d_world, n_world, d_merge_ok, d_obs_counts = self._consensus_args
        split_room = None if d_split is None else int(np.prod(d_split.shape)) // 2
        o = self.landmarks.add_views_tensors(self.torch, table, d_poses, self.cap, self._fb, d_counts, self.originals,
                                             self.noriginals, self.refined.final, self.refined.verdict, self.refined.pose,
                                             best=None if d_merge_ok is None else self.best, skip=skip, split=d_split,
                                             split_count=d_split_count, split_room=split_room, n_world=n_world, obs_room=obs_room,
                                             lm_room=lm_room)
        self._cur["done"].record(self._rs_s)             # this set's lists have been read when the call has run
        return o

    def sync(self):
        call("hm_sync", self.matcher.handle)
        self.cons.sync()

    def close(self):
        self.cons.close()
        self.matcher.close()
