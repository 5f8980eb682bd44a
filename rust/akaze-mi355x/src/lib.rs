//! `akaze`-compatible front-end over the MI355X library (C ABI declared in `include/akz.h`).
//!
//! NOT BUILT in this repository (no Rust toolchain in the build image); kept as the reference-side
//! binding of INTEGRATION.md.  Its C++ twin, include/akaze.hpp, has the same structure (per-thread context cache, capacity
//! growth, consensus layer) and IS built and run against the GPU by tests/cpp/estimate_pose.cpp.  The public surface is the one rust-cv callers use
//! (`akaze/src/lib.rs:69-185,295-366` of rust-cv/cv): `Akaze` with its 11 public fields,
//! `Akaze::{new, sparse, dense, extract, extract_from_gray_float_image, extract_path}`, `KeyPoint`, the `image`
//! module (`GrayFloatImage`, the separable filters, `gaussian_kernel`), a `space::Knn` implementor, the two-view
//! consensus and the place-recognition hasher.
use bitarray::BitArray;
use cv_core::{
    nalgebra::{Vector4, IsometryMatrix3, Matrix3, Point2, Rotation3, Translation3, UnitVector3, Vector3},
    sample_consensus::{Consensus, Estimator},
    CameraToCamera, FeatureMatch, FeatureWorldMatch, ImagePoint, Projective, TriangulatorObservations, WorldPoint, WorldToCamera,
};
use ::image::{DynamicImage, ImageResult};
use std::{cell::{Cell, RefCell}, os::raw::c_void, path::Path, ptr};

#[repr(C)]
#[derive(Clone, Copy)]
struct AkzConfig {
    maximum_features: u64,
    num_sublevels: u32,
    max_octave_evolution: u32,
    base_scale_offset: f64,
    initial_contrast: f64,
    contrast_percentile: f64,
    contrast_factor_num_bins: u64,
    derivative_factor: f64,
    detector_threshold: f64,
    descriptor_channels: u64,
    descriptor_pattern_size: u64,
}
#[repr(C)]
#[derive(Clone, Copy, Default)]
struct AkzKeypoint {
    x: f32,
    y: f32,
    response: f32,
    size: f32,
    angle: f32,
    octave: u32,
    class_id: u32,
}
#[repr(C)]
#[derive(Clone, Copy)]
pub struct AkzNeighbor {
    pub index: u32,
    pub distance: u32,
}

/// `akz_options` (include/akz.h): sixteen 32-bit words; everything zero = the library's defaults.
#[repr(C)]
#[derive(Clone, Copy, Default)]
struct AkzOptions {
    struct_size: u32,
    flags: u32,
    fed_block: u32,
    sup_capacity: u32,
    max_candidates: u32,
    desc_tile_shift: u32,
    stream_waves: u32,
    stream_min_waves: u32,
    arith: u32,
    cu_ss: u32,
    cu_kp: u32,
    resident_min_frames: u32,
    reserved: [u32; 4],
}

extern "C" {
    fn akz_create(cfg: *const AkzConfig, device: i32, max_w: i32, max_h: i32, max_batch: i32, max_kp: u32,
                  out: *mut *mut c_void) -> i32;
    fn akz_create_ex(cfg: *const AkzConfig, device: i32, max_w: i32, max_h: i32, max_batch: i32, max_kp: u32,
                     opts: *const AkzOptions, out: *mut *mut c_void) -> i32;
    fn akz_destroy(ctx: *mut c_void) -> i32;
    fn akz_extract_gray_u16(ctx: *mut c_void, img: *const u16, w: i32, h: i32, stride: i32, kps: *mut AkzKeypoint,
                            descs: *mut [u8; 64], cap: u32, n_out: *mut u32) -> i32;
    fn akz_extract_gray_u8(ctx: *mut c_void, img: *const u8, w: i32, h: i32, stride: i32, kps: *mut AkzKeypoint,
                           descs: *mut [u8; 64], cap: u32, n_out: *mut u32) -> i32;
    fn akz_extract_gray_f32(ctx: *mut c_void, img: *const f32, w: i32, h: i32, stride: i32, kps: *mut AkzKeypoint,
                            descs: *mut [u8; 64], cap: u32, n_out: *mut u32) -> i32;
    fn akz_extract_color(ctx: *mut c_void, pixels: *const c_void, fmt: i32, channels: i32, w: i32, h: i32, stride: i32,
                         kps: *mut AkzKeypoint, descs: *mut [u8; 64], cap: u32, n_out: *mut u32) -> i32;
    fn akz_gaussian_kernel(r: f32, kernel_size: u32, out: *mut f32) -> i32;
    fn akz_horizontal_filter(ctx: *mut c_void, img: *const f32, w: i32, h: i32, kernel: *const f32, ksize: u32,
                             out: *mut f32) -> i32;
    fn akz_vertical_filter(ctx: *mut c_void, img: *const f32, w: i32, h: i32, kernel: *const f32, ksize: u32,
                           out: *mut f32) -> i32;
    fn akz_half_size(ctx: *mut c_void, img: *const f32, w: i32, h: i32, out: *mut f32) -> i32;
    fn rs_create(device: i32, max_matches: u32, max_hypotheses: u32, out: *mut *mut c_void) -> i32;
    fn rs_destroy(ctx: *mut c_void) -> i32;
    fn rs_essential_batch(ctx: *mut c_void, bearings_a: *const f64, bearings_b: *const f64, n: u32,
                          sample_idx: *const u32, n_hyp: u32, thresh: f64, best_pose: *mut f64, best_id: *mut u32,
                          inlier_idx: *mut u32, cap: u32, n_inliers: *mut u32) -> i32;
    fn rs_essential_arrsac(ctx: *mut c_void, bearings_a: *const f64, bearings_b: *const f64, n: u32, sample_idx: *const u32,
                           params: *const RsArrsacParams, best_pose: *mut f64, best_id: *mut u32, inlier_idx: *mut u32,
                           cap: u32, n_inliers: *mut u32, stats: *mut c_void) -> i32;
    fn rs_p3p_arrsac(ctx: *mut c_void, bearings: *const f64, world: *const f64, n: u32, sample_idx: *const u32,
                     params: *const RsArrsacParams, best_pose: *mut f64, best_id: *mut u32, inlier_idx: *mut u32, cap: u32,
                     n_inliers: *mut u32, stats: *mut c_void) -> i32;
    fn rs_triangulate_params_default(params: *mut RsTriangulateParams) -> i32;
    fn rs_triangulate_observations(ctx: *mut c_void, poses: *const f64, bearings: *const f64, n: u32,
                                   params: *const RsTriangulateParams, point: *mut f64, reason: *mut u8) -> i32;
    fn rs_batch_reserve(ctx: *mut c_void, max_scenes: u32) -> i32;
    fn rs_sync(ctx: *mut c_void) -> i32;
    fn rs_stream(ctx: *mut c_void) -> *mut c_void;
    fn rs_three_view_params_default(params: *mut RsThreeViewParams) -> i32;
    fn rs_three_view_init_batch_device(ctx: *mut c_void, d_kps: *const c_void, cap_per_img: u32, n_blocks: u32, ic: *const u32,
                                       i_first: *const u32, i_second: *const u32, cam: *const RsCamera, d_pose_first: *const c_void,
                                       d_pose_second: *const c_void, d_triples: *const c_void, d_ntriples: *const c_void,
                                       d_first_only: *const c_void, d_nfirst: *const c_void, d_second_only: *const c_void,
                                       d_nsecond: *const c_void, n_scenes: u32, params: *const RsThreeViewParams,
                                       d_pose_out: *mut c_void, d_verdict: *mut c_void, d_combined: *mut c_void, d_first_ok: *mut c_void,
                                       d_second_ok: *mut c_void, d_stats: *mut c_void, stream_to_wait: *mut c_void) -> i32;
    fn rs_three_view_constraint_params_default(params: *mut RsThreeViewConstraintParams) -> i32;
    fn rs_three_view_constraint_batch_device(ctx: *mut c_void, d_kps: *const c_void, cap_per_img: u32, n_blocks: u32, d_poses: *const c_void,
                                             cam: *const RsCamera, d_views: *const c_void, d_lm_start: *const c_void, d_lm: *const c_void,
                                             n_lm: u32, n_constraints: u32, params: *const RsThreeViewConstraintParams,
                                             d_pose_out: *mut c_void, d_verdict: *mut c_void, d_stats: *mut c_void,
                                             stream_to_wait: *mut c_void) -> i32;
    fn rs_pose_graph_params_default(params: *mut RsPoseGraphParams) -> i32;
    fn rs_pose_graph_edges_device(ctx: *mut c_void, d_views: *const c_void, d_constraint_poses: *const c_void,
                                  d_constraint_verdict: *const c_void, n_constraints: u32, d_edges: *mut c_void,
                                  stream_to_wait: *mut c_void) -> i32;
    fn rs_pose_graph_relax_batch_device(ctx: *mut c_void, d_poses: *mut c_void, n_views: u32, d_graph_start: *const c_void, n_graphs: u32,
                                        d_row_start: *const c_void, d_row_edges: *const c_void, n_rows: u32, d_views: *const c_void,
                                        d_constraint_verdict: *const c_void, d_edges: *const c_void, n_constraints: u32,
                                        params: *const RsPoseGraphParams, d_graph_verdict: *mut c_void, d_view_state: *mut c_void,
                                        d_stats: *mut c_void, stream_to_wait: *mut c_void) -> i32;
    fn rs_pose_graph_debug_resident_views(ctx: *mut c_void, views: u32) -> i32;
    fn rs_observation_filter_params_default(params: *mut RsObservationFilterParams) -> i32;
    fn rs_filter_observations_device(ctx: *mut c_void, d_kps: *const c_void, cap_per_img: u32, n_blocks: u32, d_poses: *const c_void,
                                     cam: *const RsCamera, d_obs_start: *const c_void, d_obs: *const c_void, n_obs: u32, n_landmarks: u32,
                                     d_recon_start: *const c_void, d_view_start: *const c_void, n_recons: u32, d_skip: *const c_void,
                                     params: *const RsObservationFilterParams, d_keep: *mut c_void, d_lm_state: *mut c_void,
                                     d_tri_reason: *mut c_void, d_robust: *mut c_void, d_obs_start_out: *mut c_void, d_obs_out: *mut c_void,
                                     d_split_out: *mut c_void, d_counts: *mut c_void, d_recon_verdict: *mut c_void, d_stats: *mut c_void,
                                     stream_to_wait: *mut c_void) -> i32;
    fn rs_optimize_reconstruction_batch_device(ctx: *mut c_void, d_poses: *mut c_void, n_views: u32, d_graph_start: *const c_void, n_graphs: u32,
                                               d_row_start: *const c_void, d_row_edges: *const c_void, n_rows: u32, d_views: *const c_void,
                                               d_constraint_verdict: *const c_void, d_edges: *const c_void, n_constraints: u32,
                                               pg_params: *const RsPoseGraphParams, d_kps: *const c_void, cap_per_img: u32, cam: *const RsCamera,
                                               d_obs_start: *const c_void, d_obs: *const c_void, n_obs: u32, n_landmarks: u32,
                                               d_recon_start: *const c_void, params: *const RsObservationFilterParams, d_verdict: *mut c_void,
                                               d_graph_verdict: *mut c_void, d_view_state: *mut c_void, d_pg_stats: *mut c_void,
                                               d_keep: *mut c_void, d_lm_state: *mut c_void, d_tri_reason: *mut c_void, d_robust: *mut c_void,
                                               d_obs_start_out: *mut c_void, d_obs_out: *mut c_void, d_split_out: *mut c_void,
                                               d_counts: *mut c_void, d_recon_verdict: *mut c_void, d_of_stats: *mut c_void, d_world: *mut c_void,
                                               d_world_reason: *mut c_void, stream_to_wait: *mut c_void) -> i32;
    fn rs_covisibility_params_default(params: *mut RsCovisibilityParams) -> i32;
    fn rs_covisibility_candidates_device(ctx: *mut c_void, d_obs_start: *const c_void, d_obs: *const c_void, n_obs: u32, n_landmarks: u32,
                                         cap_per_img: u32, n_blocks: u32, d_reason: *const c_void, d_targets: *const c_void, n_targets: u32,
                                         params: *const RsCovisibilityParams, d_views: *mut c_void, d_lm_start: *mut c_void,
                                         d_lm: *mut c_void, d_slot_count: *mut c_void, d_target_verdict: *mut c_void, d_stats: *mut c_void,
                                         stream_to_wait: *mut c_void) -> i32;
    fn rs_covisibility_record_device(ctx: *mut c_void, d_constraint_verdict: *const c_void, d_targets: *const c_void, n_targets: u32,
                                     d_graph_start: *const c_void, n_graphs: u32, params: *const RsCovisibilityParams,
                                     d_recorded: *mut c_void, d_target_verdict: *mut c_void, d_stats: *mut c_void,
                                     stream_to_wait: *mut c_void) -> i32;
    fn rs_pose_graph_rows_device(ctx: *mut c_void, d_views: *const c_void, n_constraints: u32, n_views: u32, d_row_start: *mut c_void,
                                 d_row_edges: *mut c_void, d_flags: *mut c_void, stream_to_wait: *mut c_void) -> i32;
    fn rs_single_view_params_default(params: *mut RsSingleViewParams) -> i32;
    fn rs_refine_poses_batch_device(ctx: *mut c_void, d_kps: *const c_void, cap_per_img: u32, n_blocks: u32, d_poses: *const c_void,
                                    cam: *const RsCamera, d_obs_start: *const c_void, d_obs: *const c_void, n_obs: u32, n_landmarks: u32,
                                    d_world: *const c_void, n_world: u32, ik: *const u32, d_matches: *const c_void, d_nmatches: *const c_void,
                                    d_best: *const c_void, d_pose: *const c_void, d_best_id: *const c_void, d_inliers: *const c_void,
                                    d_n_inliers: *const c_void, n_scenes: u32, params: *const RsSingleViewParams, d_pose_out: *mut c_void,
                                    d_verdict: *mut c_void, d_final: *mut c_void, d_n_final: *mut c_void, d_stats: *mut c_void,
                                    stream_to_wait: *mut c_void) -> i32;
    fn rs_landmarks_sharing_view_device(ctx: *mut c_void, d_obs_start: *const c_void, d_obs: *const c_void, n_obs: u32, n_landmarks: u32,
                                        d_best: *const c_void, d_decision: *const c_void, cap_per_img: u32, n_frames: u32,
                                        d_merge_ok: *mut c_void, stream_to_wait: *mut c_void) -> i32;
    fn rs_add_views_device(ctx: *mut c_void, d_obs_start: *const c_void, d_obs: *const c_void, n_obs: u32, n_landmarks: u32, n_world: u32,
                           d_split: *const c_void, d_split_count: *const c_void, split_room: u32, cap_per_img: u32, n_blocks: u32,
                           ik: *const u32, n_frames: u32, d_counts: *const c_void, d_matches: *const c_void, d_nmatches: *const c_void,
                           d_final: *const c_void, d_verdict: *const c_void, d_pose_out: *const c_void, d_best: *const c_void,
                           d_skip: *const c_void, obs_room: u32, lm_room: u32, d_poses: *mut c_void, d_obs_start_out: *mut c_void,
                           d_obs_out: *mut c_void, d_counts_out: *mut c_void, d_landmarks_out: *mut c_void, d_obs_counts_out: *mut c_void,
                           d_frame_verdict: *mut c_void, d_stats: *mut c_void, d_call_verdict: *mut c_void,
                           stream_to_wait: *mut c_void) -> i32;
    fn rs_repack_table_device(ctx: *mut c_void, d_obs_start: *const c_void, d_obs: *const c_void, n_obs: u32, n_landmarks: u32,
                              cap_per_img: u32, n_blocks: u32, d_block_map: *const c_void, n_blocks_out: u32,
                              d_recon_start: *const c_void, n_recons: u32, obs_room: u32, lm_room: u32, d_obs_start_out: *mut c_void,
                              d_obs_out: *mut c_void, d_obs_counts_out: *mut c_void, d_landmarks_out: *mut c_void,
                              d_key_out: *mut c_void, d_recon_start_out: *mut c_void, d_counts_out: *mut c_void,
                              d_call_verdict: *mut c_void, stream_to_wait: *mut c_void) -> i32;
    fn rs_gather_blocks_device(ctx: *mut c_void, d_src: *const c_void, d_dst: *mut c_void, row_bytes: u32, n_blocks: u32,
                               d_block_map: *const c_void, n_blocks_out: u32, d_verdict: *mut c_void,
                               stream_to_wait: *mut c_void) -> i32;
    fn rs_repack_constraints_device(ctx: *mut c_void, d_views: *const c_void, d_constraint_poses: *const c_void,
                                    d_constraint_verdict: *const c_void, n_constraints: u32, d_block_map: *const c_void,
                                    n_blocks: u32, n_blocks_out: u32, d_start: *const c_void, n_ranges: u32,
                                    d_views_out: *mut c_void, d_constraint_poses_out: *mut c_void,
                                    d_constraint_verdict_out: *mut c_void, d_count: *mut c_void, d_start_out: *mut c_void,
                                    stream_to_wait: *mut c_void) -> i32;
    fn hm_place_remap_views_device(ctx: *mut c_void, d_recon: *mut c_void, d_view: *mut c_void, n_stored: u32, recon: u32,
                                   d_block_map: *const c_void, n_blocks: u32, d_flags: *mut c_void,
                                   stream_to_wait: *mut c_void) -> i32;
    fn rs_merge_map_device(ctx: *mut c_void, d_matches: *const c_void, d_nmatches: *const c_void, d_final: *const c_void, d_best: *const c_void,
                           n_world: u32, n_dst_landmarks: u32, cap_per_img: u32, slot: u32, d_counts: *const c_void,
                           d_src_landmarks: *const c_void, n_blocks: u32, bridge_block: u32, d_map: *mut c_void, d_map_count: *mut c_void,
                           stream_to_wait: *mut c_void) -> i32;
    fn rs_incorporate_reconstruction_device(ctx: *mut c_void, d_dst_start: *const c_void, d_dst_obs: *const c_void, n_dst_obs: u32,
                                            n_dst_landmarks: u32, d_src_start: *const c_void, d_src_obs: *const c_void, n_src_obs: u32,
                                            n_src_landmarks: u32, d_map: *const c_void, d_map_count: *const c_void, map_room: u32,
                                            cap_per_img: u32, n_blocks: u32, src_blocks: *const u32, n_src_views: u32, bridge_block: u32,
                                            d_src_pose: *const c_void, d_skip: *const c_void, obs_room: u32, lm_room: u32,
                                            d_poses: *mut c_void, d_obs_start_out: *mut c_void, d_obs_out: *mut c_void,
                                            d_counts_out: *mut c_void, d_landmarks_out: *mut c_void, d_obs_counts_out: *mut c_void,
                                            d_src_key_out: *mut c_void, d_call_verdict: *mut c_void, stream_to_wait: *mut c_void) -> i32;
    fn rs_normalize_reconstruction_device(ctx: *mut c_void, view_blocks: *const u32, n_views: u32, d_counts: *const c_void,
                                          d_landmarks: *const c_void, cap_per_img: u32, n_blocks: u32, d_world: *const c_void, n_world: u32,
                                          d_poses: *mut c_void, d_constraint_poses: *mut c_void, n_constraints: u32, d_stats: *mut c_void,
                                          d_verdict: *mut c_void, stream_to_wait: *mut c_void) -> i32;
    fn rs_export_reconstruction_device(ctx: *mut c_void, d_world: *const c_void, n_world: u32, d_obs_start: *const c_void, d_obs: *const c_void,
                                       n_obs: u32, n_landmarks: u32, d_colors: *const c_void, view_blocks: *const u32, n_views: u32,
                                       d_counts: *const c_void, d_landmarks: *const c_void, cap_per_img: u32, n_blocks: u32,
                                       d_poses: *const c_void, room: u32, d_xyz: *mut c_void, d_rgb: *mut c_void, d_key: *mut c_void,
                                       d_cameras: *mut c_void, d_counts_out: *mut c_void, d_verdict: *mut c_void,
                                       stream_to_wait: *mut c_void) -> i32;
    fn rs_write_ply(path: *const std::os::raw::c_char, xyz: *const f64, rgb: *const u8, n_vertices: u32, n_cameras: u32, camera_faces: i32) -> i32;
    fn rs_join_pairs_batch_device(ctx: *mut c_void, d_pairs: *const c_void, d_npairs: *const c_void, d_inliers: *const c_void,
                                  d_n_inliers: *const c_void, d_best_id: *const c_void, d_pose: *const c_void, n_slots: u32, cap_per_img: u32,
                                  slot_first: *const u32, slot_second: *const u32, n_scenes: u32, two_view_minimum_robust_matches: u32, flags: u32,
                                  seed: u64, d_triples: *mut c_void, d_ntriples: *mut c_void, d_first_only: *mut c_void, d_nfirst: *mut c_void,
                                  d_second_only: *mut c_void, d_nsecond: *mut c_void, d_pose_first: *mut c_void, d_pose_second: *mut c_void,
                                  d_verdict: *mut c_void, stream_to_wait: *mut c_void) -> i32;
    fn rs_add_reconstruction_batch_device(ctx: *mut c_void, d_triples: *const c_void, d_ntriples: *const c_void, d_first_only: *const c_void,
                                          d_nfirst: *const c_void, d_second_only: *const c_void, d_nsecond: *const c_void, d_combined: *const c_void,
                                          d_first_ok: *const c_void, d_second_ok: *const c_void, d_pose_out: *const c_void, d_verdict: *const c_void,
                                          ic: *const u32, i_first: *const u32, i_second: *const u32, n_scenes: u32, d_kps: *const c_void,
                                          d_counts: *const c_void, n_src_blocks: u32, cap_per_img: u32, d_skip: *const c_void,
                                          d_obs_start: *const c_void, d_obs: *const c_void, n_obs: u32, n_landmarks: u32,
                                          d_recon_start: *const c_void, d_view_start: *const c_void, n_recons: u32, d_kps_dst: *mut c_void,
                                          d_counts_dst: *mut c_void, d_poses: *mut c_void, n_blocks: u32, view_base: u32, obs_room: u32, lm_room: u32,
                                          d_obs_start_out: *mut c_void, d_obs_out: *mut c_void, d_obs_counts_out: *mut c_void,
                                          d_counts_out: *mut c_void, d_landmarks_out: *mut c_void, d_recon_start_out: *mut c_void,
                                          d_view_start_out: *mut c_void, d_views_out: *mut c_void, d_constraint_poses_out: *mut c_void,
                                          d_constraint_verdict_out: *mut c_void, d_frame_verdict: *mut c_void, d_stats: *mut c_void,
                                          d_call_verdict: *mut c_void, stream_to_wait: *mut c_void) -> i32;
    fn akz_sample_colors_batch_device(ctx: *mut c_void, d_rgb: *const c_void, n: i32, w: i32, h: i32, stride: i32, d_kps: *const c_void,
                                      d_counts: *const c_void, cap_per_img: u32, d_colors: *mut c_void, stream_to_wait: *mut c_void) -> i32;
    fn hm_landmark_original_matches_batch_device(ctx: *mut c_void, d_best: *const c_void, d_decision: *const c_void, d_merge_ok: *const c_void,
                                                 d_obs_counts: *const c_void, d_nq: *const c_void, iq: *const u32, cap_per_img: u32,
                                                 n_frames: u32, n_world: u32, d_pairs: *mut c_void, d_npairs: *mut c_void,
                                                 stream_to_wait: *mut c_void) -> i32;
    fn hm_create(device: i32, max_q: u32, max_t: u32, out: *mut *mut c_void) -> i32;
    fn hm_destroy(ctx: *mut c_void) -> i32;
    fn hm_knn2(ctx: *mut c_void, q: *const [u8; 64], nq: u32, t: *const [u8; 64], nt: u32, out: *mut AkzNeighbor) -> i32;
    fn hm_knn(ctx: *mut c_void, q: *const [u8; 64], nq: u32, t: *const [u8; 64], nt: u32, k: u32,
              out: *mut AkzNeighbor) -> i32;
    fn hm_set_targets(ctx: *mut c_void, t: *const [u8; 64], nt: u32) -> i32;
    fn hm_targets_generation(ctx: *mut c_void) -> u64;
    fn akz_abi_version() -> u32;
    fn hm_knn_targets(ctx: *mut c_void, q: *const [u8; 64], nq: u32, k: u32, out: *mut AkzNeighbor) -> i32;
    fn hm_hash_bag(ctx: *mut c_void, feats: *const [u8; 64], n: u32, codewords: *const [u8; 64], n_codewords: u32,
                   hash: *mut u8, words: *mut AkzNeighbor) -> i32;
    fn hm_hash_knn(ctx: *mut c_void, query: *const u8, hashes: *const u8, n: u32, hash_bytes: u32, k: u32,
                   out: *mut AkzNeighbor, n_out: *mut u32) -> i32;
    fn hm_place_params_default(params: *mut HmPlaceParams) -> i32;
    fn hm_place_room(params: *const HmPlaceParams) -> u32;
    fn hm_find_frames_batch_device(ctx: *mut c_void, d_hashes: *const c_void, d_feed: *const c_void, d_pos: *const c_void,
                                   d_recon: *const c_void, d_view: *const c_void, n_stored: u32, hash_bytes: u32, d_query: *const c_void,
                                   d_visible: *const c_void, nq: u32, params: *const HmPlaceParams, room: u32, d_found: *mut c_void,
                                   d_views_out: *mut c_void, d_group_recon: *mut c_void, d_group_start: *mut c_void, d_free: *mut c_void,
                                   d_search: *mut c_void, d_counts: *mut c_void, d_verdict: *mut c_void, stream_to_wait: *mut c_void) -> i32;
    fn hm_view_plan_device(ctx: *mut c_void, d_views_out: *const c_void, d_group_recon: *const c_void, d_group_start: *const c_void,
                           d_counts: *const c_void, d_verdict: *const c_void, room: u32, d_pick: *const c_void, flags: u32, n_frames: u32,
                           n_views: u32, n_blocks: u32, exp_blocks: u32, d_view_idx: *mut c_void, d_n_views: *mut c_void,
                           d_plan_verdict: *mut c_void, d_plan_counts: *mut c_void, stream_to_wait: *mut c_void) -> i32;
    fn hm_knn_planned_batch_device(ctx: *mut c_void, d_q: *const c_void, d_nq: *const c_void, d_t: *const c_void, d_nt: *const c_void,
                                   cap_per_img: u32, iq: *const u32, d_view_idx: *const c_void, d_n_views: *const c_void, n_frames: u32,
                                   n_views: u32, n_blocks: u32, exp_blocks: u32, k: u32, d_out: *mut c_void, stream_to_wait: *mut c_void) -> i32;
    fn hm_best_of_views_planned_batch_device(ctx: *mut c_void, d_knn: *const c_void, d_nq: *const c_void, iq: *const u32, cap_per_img: u32,
                                             d_view_idx: *const c_void, d_n_views: *const c_void, n_frames: u32, n_views: u32, n_blocks: u32,
                                             k: u32, d_landmarks: *const c_void, d_nviews: *const c_void, better_by: u32, d_best: *mut c_void,
                                             d_decision: *mut c_void, stream_to_wait: *mut c_void) -> i32;
}

/// `akaze::KeyPoint` (akaze/src/lib.rs:69-93).
#[derive(Debug, Clone, Copy)]
pub struct KeyPoint {
    pub point: (f32, f32),
    pub response: f32,
    pub size: f32,
    pub octave: usize,
    pub class_id: usize,
    pub angle: f32,
}
impl ImagePoint for KeyPoint {
    fn image_point(&self) -> Point2<f64> {
        Point2::new(self.point.0 as f64, self.point.1 as f64)
    }
}

/// `akaze::Akaze` (akaze/src/lib.rs:109-185): same fields, same defaults.
#[derive(Debug, Copy, Clone)]
pub struct Akaze {
    pub maximum_features: usize,
    pub num_sublevels: u32,
    pub max_octave_evolution: u32,
    pub base_scale_offset: f64,
    pub initial_contrast: f64,
    pub contrast_percentile: f64,
    pub contrast_factor_num_bins: usize,
    pub derivative_factor: f64,
    pub detector_threshold: f64,
    pub descriptor_channels: usize,
    pub descriptor_pattern_size: usize,
}
impl Default for Akaze {
    fn default() -> Akaze {
        Akaze {
            maximum_features: usize::MAX,
            num_sublevels: 4,
            max_octave_evolution: 4,
            base_scale_offset: 1.6,
            initial_contrast: 0.001,
            contrast_percentile: 0.7,
            contrast_factor_num_bins: 300,
            derivative_factor: 1.5,
            detector_threshold: 0.001,
            descriptor_channels: 3,
            descriptor_pattern_size: 10,
        }
    }
}

/// `rs_arrsac_params` (include/akz.h).
#[repr(C)]
#[derive(Clone, Copy)]
pub struct RsArrsacParams {
    struct_size: u32,
    n_hypotheses: u32,
    block_size: u32,
    init_blocks: u32,
    max_candidates: u32,
    flags: u32,
    threshold: f64,
    sprt_delta: f64,
    sprt_ratio: f64,
    seed: u64,
    estimations_per_block: u32,
    reserved: u32,
}

const AKZ_E_CAPACITY: i32 = -4;
const AKZ_E_INTERNAL: i32 = -7;
const FMT_U8: i32 = 0;
const FMT_F32: i32 = 1;
const FMT_U16: i32 = 2;
/// First capacity of the device's per-frame lists.  The reference's `Vec`s are unbounded (`maximum_features` is
/// `usize::MAX`, lib.rs:172): a call that overflows the capacity is repeated with twice as much, up to the library's
/// 262 144 keypoints per frame — a caller never sees the cap, only (beyond 262 144) a panic naming it.
const INITIAL_KP: u32 = 16384;
const LIBRARY_MAX_KP: u32 = 262144;

/// One device pyramid per (config, size, capacity), per thread.  `Akaze` itself stays the reference's `Copy` struct
/// with `&self` methods and no state (lib.rs:108): a loop of `extract` calls (cv-sfm/src/lib.rs:2200-2204) re-uses the
/// pyramid instead of allocating ~0.2 GB per frame.
struct CachedCtx {
    cfg: AkzConfig,
    w: u32,
    h: u32,
    cap: u32,
    arith: u32,
    ctx: *mut c_void,
}
impl Drop for CachedCtx {
    fn drop(&mut self) {
        unsafe { akz_destroy(self.ctx) };
    }
}
thread_local! {
    static CTX: RefCell<Option<CachedCtx>> = RefCell::new(None);
    static MATCHER: RefCell<Option<(u32, *mut c_void)>> = RefCell::new(None);
}
fn same_cfg(a: &AkzConfig, b: &AkzConfig) -> bool {
    a.maximum_features == b.maximum_features && a.num_sublevels == b.num_sublevels
        && a.max_octave_evolution == b.max_octave_evolution && a.base_scale_offset == b.base_scale_offset
        && a.initial_contrast == b.initial_contrast && a.contrast_percentile == b.contrast_percentile
        && a.contrast_factor_num_bins == b.contrast_factor_num_bins && a.derivative_factor == b.derivative_factor
        && a.detector_threshold == b.detector_threshold && a.descriptor_channels == b.descriptor_channels
        && a.descriptor_pattern_size == b.descriptor_pattern_size
}
/// Which of the reference's three un-vendored arithmetic orders the filters and `half_size` use (`akz_options.arith`,
/// `AKZ_ARITH_*` bits of include/akz.h; 0 = what the crate sources imply for a default x86-64 build).  The `Akaze` struct
/// stays the reference's eleven fields, so this is process-wide: call it once, before the first `extract`, with the value
/// `python3 tools/pin_arith.py <rust>_kps.csv <rust>_descs.txt image.png` names for the cargo build this crate replaces
/// (INTEGRATION.md 6).  Contexts created under another value are dropped at the next call.
pub fn set_arith(arith: u32) {
    assert!(arith < 8, "akz_options.arith takes AKZ_ARITH_* bits 0..7");
    ARITH.store(arith, std::sync::atomic::Ordering::Relaxed);
}
static ARITH: std::sync::atomic::AtomicU32 = std::sync::atomic::AtomicU32::new(0);

/// The thread's matcher context, grown to hold `n` descriptors a side.
/// include/akz.h AKZ_ABI_VERSION these bindings were written against; the loaded library must export the same number.
const AKZ_ABI_VERSION: u32 = 11;
fn require_abi() {
    let got = unsafe { akz_abi_version() };
    assert_eq!(got, AKZ_ABI_VERSION, "libakz exports ABI {got}, akaze-mi355x was written against {AKZ_ABI_VERSION}");
}

fn with_matcher<R>(n: u32, f: impl FnOnce(*mut c_void) -> R) -> R {
    MATCHER.with(|m| {
        let mut m = m.borrow_mut();
        if m.map_or(true, |(cap, _)| cap < n) {
            if let Some((_, old)) = m.take() {
                unsafe { hm_destroy(old) };
            }
            require_abi();
            let cap = n.max(4096).next_power_of_two();
            let mut ctx: *mut c_void = ptr::null_mut();
            let st = unsafe { hm_create(0, cap, cap, &mut ctx) };
            assert_eq!(st, 0, "hm_create failed with status {st} (there is no CPU fallback)");
            *m = Some((cap, ctx));
        }
        f(m.unwrap().1)
    })
}

impl Akaze {
    pub fn new(threshold: f64) -> Self {
        Self { detector_threshold: threshold, ..Default::default() }
    }
    pub fn sparse() -> Self {
        Self::new(0.01)
    }
    pub fn dense() -> Self {
        Self::new(0.0001)
    }

    fn config(&self) -> AkzConfig {
        AkzConfig {
            maximum_features: self.maximum_features as u64,
            num_sublevels: self.num_sublevels,
            max_octave_evolution: self.max_octave_evolution,
            base_scale_offset: self.base_scale_offset,
            initial_contrast: self.initial_contrast,
            contrast_percentile: self.contrast_percentile,
            contrast_factor_num_bins: self.contrast_factor_num_bins as u64,
            derivative_factor: self.derivative_factor,
            detector_threshold: self.detector_threshold,
            descriptor_channels: self.descriptor_channels as u64,
            descriptor_pattern_size: self.descriptor_pattern_size as u64,
        }
    }

    /// One extraction through the thread's cached context, with growth: `AKZ_E_INTERNAL` (a device list overflowed) and
    /// `AKZ_E_CAPACITY` (more keypoints than the output arrays hold) both mean "not enough room"; the reference has no
    /// such condition, so the call is repeated with twice the capacity.
    fn run<F: Fn(*mut c_void, *mut AkzKeypoint, *mut [u8; 64], u32, *mut u32) -> i32>(
        &self, w: u32, h: u32, f: F,
    ) -> (Vec<KeyPoint>, Vec<BitArray<64>>) {
        let cfg = self.config();
        let mut cap = INITIAL_KP.min((self.maximum_features as u64).max(64).min(LIBRARY_MAX_KP as u64) as u32);
        loop {
            let (st, kps, descs, n) = CTX.with(|slot| {
                let mut slot = slot.borrow_mut();
                let arith = ARITH.load(std::sync::atomic::Ordering::Relaxed);
                let fits = slot.as_ref().map_or(false, |c| same_cfg(&c.cfg, &cfg) && c.cap == cap && c.arith == arith && w <= c.w && h <= c.h);
                if !fits {
                    *slot = None; // drops (and destroys) the previous context first
                    let mut ctx: *mut c_void = ptr::null_mut();
                    let opts = AkzOptions { struct_size: std::mem::size_of::<AkzOptions>() as u32, arith, ..Default::default() };
                    let st = unsafe { akz_create_ex(&cfg, 0, w as i32, h as i32, 1, cap, if arith != 0 { &opts } else { ptr::null() }, &mut ctx) };
                    assert_eq!(st, 0, "akz_create_ex failed with status {st} (there is no CPU fallback)");
                    *slot = Some(CachedCtx { cfg, w, h, cap, arith, ctx });
                }
                let ctx = slot.as_ref().unwrap().ctx;
                let mut kps = vec![AkzKeypoint::default(); cap as usize];
                let mut descs = vec![[0u8; 64]; cap as usize];
                let mut n = 0u32;
                let st = f(ctx, kps.as_mut_ptr(), descs.as_mut_ptr(), cap, &mut n);
                (st, kps, descs, n)
            });
            if (st == AKZ_E_INTERNAL || st == AKZ_E_CAPACITY) && cap < LIBRARY_MAX_KP {
                cap = (cap * 2).min(LIBRARY_MAX_KP);
                continue;
            }
            assert_eq!(st, 0, "akz_extract failed with status {st} (capacity {cap} keypoints per frame)");
            let n = n as usize;
            let keypoints = kps[..n]
                .iter()
                .map(|k| KeyPoint {
                    point: (k.x, k.y),
                    response: k.response,
                    size: k.size,
                    octave: k.octave as usize,
                    class_id: k.class_id as usize,
                    angle: k.angle,
                })
                .collect();
            let descriptors = descs[..n].iter().map(|d| BitArray::new(*d)).collect();
            return (keypoints, descriptors);
        }
    }

    /// `Akaze::extract` (akaze/src/lib.rs:295).  Every arm of `GrayFloatImage::from_dynamic` (image.rs:45-109) runs on the
    /// device: the gray ones as they are, the colour ones through `akz_extract_color` (`DynamicImage::grayscale()` there).
    pub fn extract(&self, image: &DynamicImage) -> (Vec<KeyPoint>, Vec<BitArray<64>>) {
        let (w, h) = (image.width(), image.height());
        let colour = |pixels: *const c_void, fmt: i32, channels: i32| {
            self.run(w, h, move |ctx, k, d, cap, n| unsafe {
                akz_extract_color(ctx, pixels, fmt, channels, w as i32, h as i32, w as i32 * channels, k, d, cap, n)
            })
        };
        match image {
            DynamicImage::ImageLuma8(g) => self.run(w, h, |ctx, k, d, cap, n| unsafe {
                akz_extract_gray_u8(ctx, g.as_raw().as_ptr(), w as i32, h as i32, w as i32, k, d, cap, n)
            }),
            DynamicImage::ImageLuma16(g) => self.run(w, h, |ctx, k, d, cap, n| unsafe {
                // image.rs:57-66: f32::from(v) / 65535f32, done on the device
                akz_extract_gray_u16(ctx, g.as_raw().as_ptr(), w as i32, h as i32, w as i32, k, d, cap, n)
            }),
            DynamicImage::ImageRgb8(c) => colour(c.as_raw().as_ptr() as *const c_void, FMT_U8, 3),
            DynamicImage::ImageRgba8(c) => colour(c.as_raw().as_ptr() as *const c_void, FMT_U8, 4),
            DynamicImage::ImageRgb16(c) => colour(c.as_raw().as_ptr() as *const c_void, FMT_U16, 3),
            DynamicImage::ImageRgba16(c) => colour(c.as_raw().as_ptr() as *const c_void, FMT_U16, 4),
            DynamicImage::ImageRgb32F(c) => colour(c.as_raw().as_ptr() as *const c_void, FMT_F32, 3),
            DynamicImage::ImageRgba32F(c) => colour(c.as_raw().as_ptr() as *const c_void, FMT_F32, 4),
            // LumaA8 / LumaA16 (image.rs:67-86: the luma sample of every pixel): drop the alpha on the host
            other => match other.grayscale() {
                DynamicImage::ImageLumaA8(g) => {
                    let l: Vec<u8> = g.pixels().map(|p| p[0]).collect();
                    self.run(w, h, |ctx, k, d, cap, n| unsafe {
                        akz_extract_gray_u8(ctx, l.as_ptr(), w as i32, h as i32, w as i32, k, d, cap, n)
                    })
                }
                DynamicImage::ImageLumaA16(g) => {
                    let l: Vec<u16> = g.pixels().map(|p| p[0]).collect();
                    self.run(w, h, |ctx, k, d, cap, n| unsafe {
                        akz_extract_gray_u16(ctx, l.as_ptr(), w as i32, h as i32, w as i32, k, d, cap, n)
                    })
                }
                _ => panic!("DynamicImage::grayscale() returned unexpected type"), // image.rs:107
            },
        }
    }

    /// `Akaze::extract_from_gray_float_image` (akaze/src/lib.rs:309).
    pub fn extract_from_gray_float_image(&self, img: &crate::image::GrayFloatImage) -> (Vec<KeyPoint>, Vec<BitArray<64>>) {
        let (w, h) = (img.width() as u32, img.height() as u32);
        self.run(w, h, |ctx, k, d, cap, n| unsafe {
            akz_extract_gray_f32(ctx, img.0.as_raw().as_ptr(), w as i32, h as i32, w as i32, k, d, cap, n)
        })
    }

    /// `Akaze::extract_path` (akaze/src/lib.rs:361).
    pub fn extract_path(&self, path: impl AsRef<Path>) -> ImageResult<(Vec<KeyPoint>, Vec<BitArray<64>>)> {
        Ok(self.extract(&::image::open(path)?))
    }
}

/// A `space::Knn` implementor with `LinearKnn { metric: Hamming, iter }` semantics for `BitArray<64>`.
///
/// The reference's callers build the `LinearKnn` once per frame pair and call `knn` once per query descriptor
/// (akaze/tests/estimate_pose.rs:82-88, cv-sfm/src/lib.rs:3103).  Ported literally that is one kernel launch per query:
/// the target set is uploaded ONCE (`hm_set_targets`: it stays on the device for as long as this thread keeps asking
/// about the same slice) and each `knn` sends 64 bytes up and `num` neighbours back — correct, and far better than
/// re-uploading 320 KB per query, but still launch-bound (about 20 us per query against 0.2 us per query for a whole
/// frame at once).  Callers that own their loop should ask for all queries together: [`Mi355xLinearKnn::knn_batch`], or
/// [`match_descriptors`] / `symmetric_matching`, which also keep the pair lists on the device side of the matcher.
pub struct Mi355xLinearKnn<'a> {
    pub targets: &'a [BitArray<64>],
    /// (matcher, generation) of THIS value's upload (`hm_targets_generation` right after its `hm_set_targets`).  The
    /// borrow keeps `targets` immutable for as long as the value lives, and the token lives in the value: a set dropped
    /// and another allocated at the same address is a different value with no token, so it uploads.
    upload: Cell<Option<(*mut c_void, u64)>>,
}
impl<'a> Mi355xLinearKnn<'a> {
    /// `LinearKnn { metric: Hamming, iter: targets }`.
    pub fn new(targets: &'a [BitArray<64>]) -> Self {
        Self { targets, upload: Cell::new(None) }
    }
    /// Upload the targets unless the matcher still holds exactly this value's upload: any other upload, or any
    /// host-buffer call that took the staging buffer, changes the matcher's generation number.
    fn resident(&self, ctx: *mut c_void) {
        let current = unsafe { hm_targets_generation(ctx) };
        if self.upload.get().map_or(true, |(c, g)| c != ctx || g != current || current == 0) {
            let st = unsafe { hm_set_targets(ctx, self.targets.as_ptr() as *const [u8; 64], self.targets.len() as u32) };
            assert_eq!(st, 0, "hm_set_targets failed with status {st}");
            self.upload.set(Some((ctx, unsafe { hm_targets_generation(ctx) })));
        }
    }
    /// `knn(q, num)` for every query in ONE launch: `out[i]` are the `min(num, targets.len())` nearest targets of
    /// `queries[i]`, ascending (distance, index) — what `queries.iter().map(|q| self.knn(q, num))` returns.
    pub fn knn_batch(&self, queries: &[BitArray<64>], num: usize) -> Vec<Vec<space::Neighbor<u32, usize>>> {
        assert!((1..=3).contains(&num), "the MI355X matcher implements knn(query, k) for k <= 3");
        let (nq, nt) = (queries.len() as u32, self.targets.len() as u32);
        let mut out = vec![AkzNeighbor { index: 0, distance: 0 }; queries.len() * num];
        let st = with_matcher(nq.max(nt), |ctx| {
            self.resident(ctx);
            unsafe { hm_knn_targets(ctx, queries.as_ptr() as *const [u8; 64], nq, num as u32, out.as_mut_ptr()) }
        });
        assert_eq!(st, 0);
        let keep = num.min(self.targets.len());
        out.chunks(num).map(|c| c.iter().take(keep)
            .map(|o| space::Neighbor { index: o.index as usize, distance: o.distance }).collect()).collect()
    }
}
impl<'a> space::Knn for Mi355xLinearKnn<'a> {
    type Ix = usize;
    type Metric = bitarray::Hamming;
    type Point = BitArray<64>;
    type KnnIter = Vec<space::Neighbor<u32, usize>>;
    fn knn(&self, query: &BitArray<64>, num: usize) -> Self::KnnIter {
        // cv-sfm asks for 2 when matching frame pairs (lib.rs:3103) and 3 when registering a frame (lib.rs:1474)
        self.knn_batch(std::slice::from_ref(query), num).pop().unwrap()
    }
    fn nn(&self, query: &BitArray<64>) -> Option<space::Neighbor<u32, usize>> {
        self.knn(query, 2).into_iter().next()
    }
}

/// `hamming_lsh::HammingHasher<64, 512>` as cv-sfm uses it (cv-sfm/src/lib.rs:205,216,672): a bag of descriptors
/// -> 512-byte hash over a 4096-word codebook, on the MI355X.  (hamming-lsh is not vendored in the reference; the
/// nearest-codeword form restated in oracle/lsh_oracle.c is what runs here.)
pub struct Mi355xHammingHasher {
    codewords: Vec<BitArray<64>>,
}
impl Mi355xHammingHasher {
    pub fn new_with_codewords(codewords: Vec<BitArray<64>>) -> Self {
        assert_eq!(codewords.len(), 512 * 8);
        Self { codewords }
    }
    pub fn hash_bag<'a>(&self, features: impl IntoIterator<Item = &'a BitArray<64>>) -> BitArray<512> {
        let feats: Vec<BitArray<64>> = features.into_iter().cloned().collect();
        let cap = (feats.len() as u32).max(self.codewords.len() as u32);
        let mut hash = [0u8; 512];
        let st = with_matcher(cap, |ctx| unsafe {
            hm_hash_bag(ctx, feats.as_ptr() as *const [u8; 64], feats.len() as u32,
                        self.codewords.as_ptr() as *const [u8; 64], self.codewords.len() as u32, hash.as_mut_ptr(),
                        ptr::null_mut())
        });
        assert_eq!(st, 0);
        BitArray::new(hash)
    }
}

/// `lsh_to_frame.knn_values(&lsh, num)` (cv-sfm/src/lib.rs:622-624) as an exact search over the stored hashes:
/// (index into `hashes`, distance), ascending (distance, index).
pub fn nearest_hashes(query: &BitArray<512>, hashes: &[BitArray<512>], num: usize) -> Vec<(usize, u32)> {
    let mut out = vec![AkzNeighbor { index: 0, distance: 0 }; num.max(1)];
    let mut n: u32 = 0;
    let st = with_matcher(2, |ctx| unsafe {
        hm_hash_knn(ctx, query.bytes().as_ptr(), hashes.as_ptr() as *const u8, hashes.len() as u32, 512, num as u32,
                    out.as_mut_ptr(), &mut n)
    });
    assert_eq!(st, 0);
    out.iter().take(n as usize).map(|o| (o.index as usize, o.distance)).collect()
}

/// `akaze::image` (akaze/src/image.rs): the f32 image wrapper and the separable filters, on the MI355X.
pub mod image {
    use super::*;
    use ::image::{ImageBuffer, Luma};

    pub type GrayImageBuffer = ImageBuffer<Luma<f32>, Vec<f32>>;

    /// `GrayFloatImage` (image.rs:36).
    #[derive(Debug, Clone)]
    pub struct GrayFloatImage(pub GrayImageBuffer);

    fn with_ctx<R>(w: u32, h: u32, f: impl FnOnce(*mut c_void) -> R) -> R {
        let cfg = Akaze::default().config();
        let mut ctx: *mut c_void = ptr::null_mut();
        assert_eq!(unsafe { akz_create(&cfg, 0, w as i32, h as i32, 1, 16, &mut ctx) }, 0);
        let r = f(ctx);
        unsafe { akz_destroy(ctx) };
        r
    }

    impl GrayFloatImage {
        /// image.rs:45-109 (8-bit gray takes v / 255 per pixel; everything else goes through `to_luma32f`)
        pub fn from_dynamic(input_image: &DynamicImage) -> Self {
            match input_image.grayscale() {
                DynamicImage::ImageLuma8(g) => Self(ImageBuffer::from_fn(g.width(), g.height(), |x, y| {
                    Luma([f32::from(g.get_pixel(x, y)[0]) / 255f32])
                })),
                other => Self(other.to_luma32f()),
            }
        }
        pub fn width(&self) -> usize { self.0.width() as usize }
        pub fn height(&self) -> usize { self.0.height() as usize }
        pub fn new(width: usize, height: usize) -> Self { Self(ImageBuffer::new(width as u32, height as u32)) }
        pub fn get(&self, x: usize, y: usize) -> f32 { self.0.get_pixel(x as u32, y as u32)[0] }
        pub fn put(&mut self, x: usize, y: usize, v: f32) { self.0.put_pixel(x as u32, y as u32, Luma([v])) }
        /// image.rs:154-199
        pub fn half_size(&self) -> Self {
            let (w, h) = (self.0.width(), self.0.height());
            let mut out = vec![0f32; ((w / 2) * (h / 2)) as usize];
            let st = with_ctx(w, h, |ctx| unsafe {
                akz_half_size(ctx, self.0.as_raw().as_ptr(), w as i32, h as i32, out.as_mut_ptr())
            });
            assert_eq!(st, 0);
            Self(ImageBuffer::from_raw(w / 2, h / 2, out).unwrap())
        }
    }

    fn filter(image: &GrayImageBuffer, kernel: &[f32], vertical: bool) -> GrayImageBuffer {
        let (w, h) = (image.width(), image.height());
        let mut out = vec![0f32; (w * h) as usize];
        let st = with_ctx(w, h, |ctx| unsafe {
            if vertical {
                akz_vertical_filter(ctx, image.as_raw().as_ptr(), w as i32, h as i32, kernel.as_ptr(), kernel.len() as u32,
                                    out.as_mut_ptr())
            } else {
                akz_horizontal_filter(ctx, image.as_raw().as_ptr(), w as i32, h as i32, kernel.as_ptr(),
                                      kernel.len() as u32, out.as_mut_ptr())
            }
        });
        assert_eq!(st, 0);
        ImageBuffer::from_raw(w, h, out).unwrap()
    }
    /// image.rs:202
    pub fn horizontal_filter(image: &GrayImageBuffer, kernel: &[f32]) -> GrayImageBuffer { filter(image, kernel, false) }
    /// image.rs:253
    pub fn vertical_filter(image: &GrayImageBuffer, kernel: &[f32]) -> GrayImageBuffer { filter(image, kernel, true) }
    /// image.rs:333
    pub fn separable_filter(image: &GrayImageBuffer, h_kernel: &[f32], v_kernel: &[f32]) -> GrayImageBuffer {
        vertical_filter(&horizontal_filter(image, h_kernel), v_kernel)
    }
    /// image.rs:360
    pub fn gaussian_kernel(r: f32, kernel_size: usize) -> Vec<f32> {
        let mut k = vec![0f32; kernel_size];
        assert_eq!(unsafe { akz_gaussian_kernel(r, kernel_size as u32, k.as_mut_ptr()) }, 0);
        k
    }
    /// image.rs:383
    pub fn gaussian_blur(image: &GrayFloatImage, r: f32) -> GrayFloatImage {
        assert!(r > 0.0, "sigma must be > 0.0");                       // image.rs:384
        let radius = (2.0 * r).ceil() as usize;                        // image.rs:385
        let k = gaussian_kernel(r, 2 * radius + 1);
        GrayFloatImage(separable_filter(&image.0, &k, &k))
    }
}

/// `arrsac::Arrsac` over the MI355X library: the `sample_consensus::Consensus` the reference's callers hand their
/// estimators to (akaze/tests/estimate_pose.rs:63-75, vslam-sandbox/src/main.rs:105-117, cv-sfm/src/lib.rs:1394-1412 and
/// 1619-1622), for the two estimators of the hot path — `EightPoint` over `FeatureMatch` and `LambdaTwist` over
/// `FeatureWorldMatch`.  The estimator argument selects the device procedure (`rs_essential_arrsac` / `rs_p3p_arrsac`);
/// its own `estimate` is not called: hypotheses, scoring and consensus all run on the GPU.  The `arrsac` crate is not
/// vendored in rust-cv/cv; what runs is this library's ARRSAC-shaped procedure (include/akz.h, specified by
/// oracle/arrsac_oracle.c) under the crate's builder names, seeded with a `u64` where the crate takes an `Rng`.
pub struct Arrsac {
    params: RsArrsacParams,
    ctx: Option<(u32, u32, *mut c_void)>, // (matches, hypotheses) the context holds
}
impl Arrsac {
    pub fn new(inlier_threshold: f64, seed: u64) -> Self {
        Self {
            params: RsArrsacParams {
                struct_size: std::mem::size_of::<RsArrsacParams>() as u32,
                // arrsac 0.10's documented defaults (the crate is not vendored in rust-cv/cv: unverified here):
                // initialization_hypotheses 256, block_size 100, initialization_blocks 4, max_candidate_hypotheses 50,
                // estimations_per_block 64, likelihood_ratio_threshold 1e3
                n_hypotheses: 256,
                block_size: 100,
                init_blocks: 4,
                max_candidates: 50,
                flags: 1 | 2 | 4, // RS_PRUNE_BOUND | RS_PRUNE_SPRT | RS_PRUNE_HALVE
                threshold: inlier_threshold,
                sprt_delta: 0.05,
                sprt_ratio: 1e3,
                seed,
                estimations_per_block: 64,
                reserved: 0,
            },
            ctx: None,
        }
    }
    pub fn initialization_hypotheses(mut self, n: usize) -> Self { self.params.n_hypotheses = n as u32; self }
    pub fn max_candidate_hypotheses(mut self, n: usize) -> Self { self.params.max_candidates = n as u32; self }
    pub fn estimations_per_block(mut self, n: usize) -> Self { self.params.estimations_per_block = n as u32; self }
    pub fn block_size(mut self, n: usize) -> Self { self.params.block_size = n as u32; self }
    pub fn initialization_blocks(mut self, n: usize) -> Self { self.params.init_blocks = n as u32; self }
    pub fn likelihood_ratio_threshold(mut self, r: f64) -> Self { self.params.sprt_ratio = r; self }

    /// `per`: hypothesis slots a sample takes (ten for the five-point estimator, one otherwise)
    fn context(&mut self, n: u32, per: u32) -> *mut c_void {
        let blocks = (n + self.params.block_size - 1) / self.params.block_size;
        let need_h = (self.params.n_hypotheses + self.params.estimations_per_block * blocks) * per;
        if self.ctx.map_or(true, |(m, h, _)| m < n || h < need_h) {
            if let Some((_, _, old)) = self.ctx.take() {
                unsafe { rs_destroy(old) };
            }
            let mut ctx: *mut c_void = ptr::null_mut();
            let st = unsafe { rs_create(0, n.max(64), need_h, &mut ctx) };
            assert_eq!(st, 0, "rs_create failed with status {st} (there is no CPU fallback)");
            self.ctx = Some((n.max(64), need_h, ctx));
        }
        self.ctx.unwrap().2
    }
    /// (row-major 3x4 `[R | t]`, inlier indices) or `None`
    fn run(&mut self, p3p: bool, a: &[f64], b: &[f64], n: u32) -> Option<([f64; 12], Vec<usize>)> {
        self.run_with(p3p, false, a, b, n)
    }
    /// `five_point`: RS_ESTIMATOR_FIVE_POINT (include/akz.h) — the hypothesis counts are five-match samples, ten slots each
    fn run_with(&mut self, p3p: bool, five_point: bool, a: &[f64], b: &[f64], n: u32) -> Option<([f64; 12], Vec<usize>)> {
        let ctx = self.context(n, if five_point { 10 } else { 1 });
        let mut params = self.params;
        if five_point {
            params.flags |= 8; // RS_ESTIMATOR_FIVE_POINT
        }
        let mut pose = [0f64; 12];
        let (mut best, mut n_inl) = (0u32, 0u32);
        let mut inl = vec![0u32; n as usize];
        let st = unsafe {
            if p3p {
                rs_p3p_arrsac(ctx, a.as_ptr(), b.as_ptr(), n, ptr::null(), &params, pose.as_mut_ptr(), &mut best,
                              inl.as_mut_ptr(), n, &mut n_inl, ptr::null_mut())
            } else {
                rs_essential_arrsac(ctx, a.as_ptr(), b.as_ptr(), n, ptr::null(), &params, pose.as_mut_ptr(), &mut best,
                                    inl.as_mut_ptr(), n, &mut n_inl, ptr::null_mut())
            }
        };
        assert_eq!(st, 0, "consensus failed with status {st}");
        if best == u32::MAX {
            return None; // Consensus::model_inliers -> None: no sample produced a model
        }
        Some((pose, inl[..n_inl as usize].iter().map(|&i| i as usize).collect()))
    }
}
impl Drop for Arrsac {
    fn drop(&mut self) {
        if let Some((_, _, ctx)) = self.ctx.take() {
            unsafe { rs_destroy(ctx) };
        }
    }
}
fn isometry(rt: &[f64; 12]) -> IsometryMatrix3<f64> {
    let r = Matrix3::new(rt[0], rt[1], rt[2], rt[4], rt[5], rt[6], rt[8], rt[9], rt[10]);
    IsometryMatrix3::from_parts(Translation3::from(Vector3::new(rt[3], rt[7], rt[11])), Rotation3::from_matrix_unchecked(r))
}
/// `Consensus<EightPoint, FeatureMatch>` — eight-point/src/lib.rs:70-83 estimates, cv-core/src/pose.rs:249-295 scores.
impl Consensus<eight_point::EightPoint, FeatureMatch> for Arrsac {
    type Inliers = Vec<usize>;
    fn model<I>(&mut self, estimator: &eight_point::EightPoint, data: I) -> Option<CameraToCamera>
    where I: Iterator<Item = FeatureMatch> + Clone {
        self.model_inliers(estimator, data).map(|(m, _)| m)
    }
    fn model_inliers<I>(&mut self, _estimator: &eight_point::EightPoint, data: I) -> Option<(CameraToCamera, Vec<usize>)>
    where I: Iterator<Item = FeatureMatch> + Clone {
        let (mut a, mut b) = (Vec::new(), Vec::new());
        for FeatureMatch(fa, fb) in data {
            a.extend_from_slice(fa.as_ref().as_slice());
            b.extend_from_slice(fb.as_ref().as_slice());
        }
        let n = (a.len() / 3) as u32;
        if (n as usize) < <eight_point::EightPoint as Estimator<FeatureMatch>>::MIN_SAMPLES {
            return None;
        }
        self.run(false, &a, &b, n).map(|(rt, inl)| (CameraToCamera(isometry(&rt)), inl))
    }
}
/// `Consensus<NisterStewenius, FeatureMatch>` — the five-point minimal solver for calibrated cameras
/// (nister-stewenius/src/lib.rs:303-330).  What runs is include/akz_five_point_math.h: the reference's algorithm with rows
/// 6..9 of the action matrix's eigenvector (rows 5..8 as written at lib.rs:230 do not solve the problem); the builder's
/// hypothesis counts are five-match samples, each with up to ten essential matrices.
impl Consensus<nister_stewenius::NisterStewenius, FeatureMatch> for Arrsac {
    type Inliers = Vec<usize>;
    fn model<I>(&mut self, estimator: &nister_stewenius::NisterStewenius, data: I) -> Option<CameraToCamera>
    where I: Iterator<Item = FeatureMatch> + Clone {
        self.model_inliers(estimator, data).map(|(m, _)| m)
    }
    fn model_inliers<I>(&mut self, _estimator: &nister_stewenius::NisterStewenius, data: I) -> Option<(CameraToCamera, Vec<usize>)>
    where I: Iterator<Item = FeatureMatch> + Clone {
        let (mut a, mut b) = (Vec::new(), Vec::new());
        for FeatureMatch(fa, fb) in data {
            a.extend_from_slice(fa.as_ref().as_slice());
            b.extend_from_slice(fb.as_ref().as_slice());
        }
        let n = (a.len() / 3) as u32;
        if (n as usize) < <nister_stewenius::NisterStewenius as Estimator<FeatureMatch>>::MIN_SAMPLES {
            return None;
        }
        self.run_with(false, true, &a, &b, n).map(|(rt, inl)| (CameraToCamera(isometry(&rt)), inl))
    }
}
/// `Consensus<LambdaTwist, FeatureWorldMatch>` — lambda-twist/src/lib.rs:330-347 estimates, cv-core/src/pose.rs:194-201 scores.
impl Consensus<lambda_twist::LambdaTwist, FeatureWorldMatch> for Arrsac {
    type Inliers = Vec<usize>;
    fn model<I>(&mut self, estimator: &lambda_twist::LambdaTwist, data: I) -> Option<WorldToCamera>
    where I: Iterator<Item = FeatureWorldMatch> + Clone {
        self.model_inliers(estimator, data).map(|(m, _)| m)
    }
    fn model_inliers<I>(&mut self, _estimator: &lambda_twist::LambdaTwist, data: I) -> Option<(WorldToCamera, Vec<usize>)>
    where I: Iterator<Item = FeatureWorldMatch> + Clone {
        let (mut a, mut w) = (Vec::new(), Vec::new());
        for FeatureWorldMatch(bearing, world) in data {
            a.extend_from_slice(bearing.as_ref().as_slice());
            w.extend_from_slice(world.homogeneous().as_slice()); // Projective form: xyz normalised, w = 1 / distance
        }
        let n = (a.len() / 3) as u32;
        if (n as usize) < <lambda_twist::LambdaTwist as Estimator<FeatureWorldMatch>>::MIN_SAMPLES {
            return None;
        }
        self.run(true, &a, &w, n).map(|(rt, inl)| (WorldToCamera(isometry(&rt)), inl))
    }
}
/// `UnitVector3` bearings of a match list, for callers that hold keypoints: `CameraIntrinsics::calibrate` is the reference's
/// own (cv-pinhole/src/lib.rs:108-117) and stays on the host — it is a handful of flops per keypoint.
pub fn bearing(v: [f64; 3]) -> UnitVector3<f64> {
    UnitVector3::new_unchecked(Vector3::new(v[0], v[1], v[2]))
}

/// `rs_triangulate_params` (include/akz.h).
#[repr(C)]
#[derive(Clone, Copy)]
pub struct RsTriangulateParams {
    struct_size: u32,
    max_sweeps: u32,
    eps: f64,
    robust_minimum_observations: u32,
    n_views: u32,
    incidence_minimum_cosine_distance: f64,
}

/// `cv_geom::triangulation::LinearEigenTriangulator` (cv-geom/src/triangulation.rs:39-130) computed on the MI355X
/// (`rs_triangulate_observations`).  `TriangulatorObservations` gives `triangulate_observations_to_camera` and, through
/// cv-core's blanket impl, `TriangulatorRelative::triangulate_relative` (cv-core/src/triangulation.rs:21-36, 52-67).
/// The device-resident forms (`rs_triangulate_landmarks_device`, `.._merged_device`, `.._pairs_batch_device`) take device
/// pointers and belong to the caller that owns those buffers.
pub struct LinearEigenTriangulator {
    params: RsTriangulateParams,
    ctx: Cell<*mut c_void>,
}
impl LinearEigenTriangulator {
    pub fn new() -> Self {
        let mut params = RsTriangulateParams { struct_size: 0, max_sweeps: 0, eps: 0.0, robust_minimum_observations: 0, n_views: 0,
                                                incidence_minimum_cosine_distance: 0.0 };
        unsafe { rs_triangulate_params_default(&mut params) };
        Self { params, ctx: Cell::new(ptr::null_mut()) }
    }
    #[must_use]
    pub fn epsilon(mut self, epsilon: f64) -> Self {
        self.params.eps = epsilon;
        self
    }
    #[must_use]
    pub fn max_iterations(mut self, max_iterations: usize) -> Self {
        // (nalgebra reads 0 as "no limit")
        self.params.max_sweeps = if max_iterations == 0 || max_iterations > 0x7FFF_FFFF { 0x7FFF_FFFF } else { max_iterations as u32 };
        self
    }
}
impl Default for LinearEigenTriangulator {
    fn default() -> Self {
        Self::new()
    }
}
impl Drop for LinearEigenTriangulator {
    fn drop(&mut self) {
        if !self.ctx.get().is_null() {
            unsafe { rs_destroy(self.ctx.get()) };
        }
    }
}
impl TriangulatorObservations for LinearEigenTriangulator {
    fn triangulate_observations(&self, pairs: impl Iterator<Item = (WorldToCamera, UnitVector3<f64>)> + Clone) -> Option<WorldPoint> {
        let mut poses = Vec::new();
        let mut bearings = Vec::new();
        for (pose, bearing) in pairs {
            let r = pose.0.rotation.matrix();
            let t = pose.0.translation.vector;
            for i in 0..3 {
                poses.extend_from_slice(&[r[(i, 0)], r[(i, 1)], r[(i, 2)], t[i]]);
            }
            bearings.extend_from_slice(&[bearing.x, bearing.y, bearing.z]);
        }
        if self.ctx.get().is_null() {
            require_abi();
            let mut ctx = ptr::null_mut();
            assert_eq!(unsafe { rs_create(0, 8, 1, &mut ctx) }, 0, "rs_create");
            self.ctx.set(ctx);
        }
        let mut point = [0.0f64; 4];
        let mut reason = 0u8;
        let st = unsafe {
            rs_triangulate_observations(self.ctx.get(), poses.as_ptr(), bearings.as_ptr(), (bearings.len() / 3) as u32, &self.params,
                                        point.as_mut_ptr(), &mut reason)
        };
        assert_eq!(st, 0, "rs_triangulate_observations");
        // (the device has already normalised xyz: from_homogeneous_unchecked would do; from_homogeneous is idempotent on it)
        (reason == 0).then(|| WorldPoint::from_homogeneous(Vector4::new(point[0], point[1], point[2], point[3])))
    }
}

/// `rs_camera` (include/akz.h).
#[repr(C)]
#[derive(Clone, Copy)]
pub struct RsCamera {
    pub fx: f64,
    pub fy: f64,
    pub cx: f64,
    pub cy: f64,
    pub skew: f64,
    pub k1: f64,
    pub use_k1: i32,
    pub reserved: i32,
}

/// `rs_three_view_params` (include/akz.h): cv-sfm's settings of the three-view bootstrap (cv-sfm/src/settings.rs:320-427).
#[repr(C)]
#[derive(Clone, Copy)]
pub struct RsThreeViewParams {
    struct_size: u32,
    pub robust_view_num_robust_bearing_pair: u32,
    pub maximum_cosine_distance: f64,
    pub maximum_sine_distance: f64,
    pub robust_observation_incidence_minimum_cosine_distance: f64,
    pub robust_view_bearing_pair_minimum_cosine_distance: f64,
    pub optimization_rate: f64,
    pub three_view_minimum_relative_scales: u32,
    pub three_view_filter_loop_iterations: u32,
    pub three_view_optimization_landmarks: u32,
    pub three_view_patience: u32,
    pub three_view_minimum_robust_matches: u32,
    pub hard_minimum_matches: u32,
    pub triangulate: RsTriangulateParams,
}

/// The verdict of one triple (`RS_TV_*`).  The reference `continue`s to the next combination on every one of them but
/// `FewBearingPairs`, where `init_reconstruction` returns `None` (cv-sfm/src/lib.rs:1100-1106).
#[repr(u32)]
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum ThreeViewVerdict {
    Ok = 0,
    FewScales = 1,
    FewBearingPairs = 2,
    FewMatches = 3,
    LostHalf = 4,
    FewRobust = 5,
    BadIndex = 6,
}

/// Words of a scene's `d_stats` row (`RS_TV_S_*`).
pub const RS_TV_STATS: usize = 24;

/// `VSlam::init_reconstruction` from its common matches on (cv-sfm/src/lib.rs:1002-1300) for many triples side by side
/// (`rs_three_view_init_batch_device`).  Every `d_*` argument is device memory the caller owns, laid out as include/akz.h
/// documents; the call enqueues on `stream()` and returns.  The HashMap join and the shuffle of lib.rs:992-999 stay with
/// the caller, who owns the RNG.
pub struct ThreeViewInit {
    pub params: RsThreeViewParams,
    ctx: *mut c_void,
}
impl ThreeViewInit {
    /// Room for `max_scenes` triples per call.
    pub fn new(max_scenes: u32) -> Self {
        require_abi();
        let mut params: RsThreeViewParams = unsafe { std::mem::zeroed() };
        assert_eq!(unsafe { rs_three_view_params_default(&mut params) }, 0, "rs_three_view_params_default");
        let mut ctx = ptr::null_mut();
        assert_eq!(unsafe { rs_create(0, 8, 1, &mut ctx) }, 0, "rs_create");
        assert_eq!(unsafe { rs_batch_reserve(ctx, max_scenes) }, 0, "rs_batch_reserve");
        Self { params, ctx }
    }
    /// # Safety
    /// Every pointer names device memory of the documented size, alive until `sync()` returns.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn init_batch_device(&self, d_kps: *const c_void, cap_per_img: u32, n_blocks: u32, ic: &[u32], i_first: &[u32], i_second: &[u32],
                                    cam: &RsCamera, d_pose_first: *const c_void, d_pose_second: *const c_void, d_triples: *const c_void,
                                    d_ntriples: *const c_void, d_first_only: *const c_void, d_nfirst: *const c_void,
                                    d_second_only: *const c_void, d_nsecond: *const c_void, d_pose_out: *mut c_void, d_verdict: *mut c_void,
                                    d_combined: *mut c_void, d_first_ok: *mut c_void, d_second_ok: *mut c_void, d_stats: *mut c_void,
                                    stream_to_wait: *mut c_void) -> Result<(), i32> {
        assert!(i_first.len() == ic.len() && i_second.len() == ic.len(), "one centre, first and second block per scene");
        let st = rs_three_view_init_batch_device(self.ctx, d_kps, cap_per_img, n_blocks, ic.as_ptr(), i_first.as_ptr(), i_second.as_ptr(), cam,
                                                 d_pose_first, d_pose_second, d_triples, d_ntriples, d_first_only, d_nfirst, d_second_only,
                                                 d_nsecond, ic.len() as u32, &self.params, d_pose_out, d_verdict, d_combined, d_first_ok,
                                                 d_second_ok, d_stats, stream_to_wait);
        if st == 0 { Ok(()) } else { Err(st) }
    }
    pub fn sync(&self) {
        assert_eq!(unsafe { rs_sync(self.ctx) }, 0, "rs_sync");
    }
    pub fn stream(&self) -> *mut c_void {
        unsafe { rs_stream(self.ctx) }
    }
}
impl Drop for ThreeViewInit {
    fn drop(&mut self) {
        unsafe { rs_destroy(self.ctx) };
    }
}

/// `rs_three_view_constraint_params` (include/akz.h): cv-sfm's settings of a three-view constraint
/// (cv-sfm/src/settings.rs:332-338, 465-483).
#[repr(C)]
#[derive(Clone, Copy)]
pub struct RsThreeViewConstraintParams {
    struct_size: u32,
    pub optimization_minimum_landmarks: u32,
    pub optimization_maximum_landmarks: u32,
    pub constraint_patience: u32,
    pub robust_view_num_robust_bearing_pair: u32,
    pub robust_view_bearing_pair_minimum_cosine_distance: f64,
}

/// The verdict of one constraint (`RS_TVC_*`): `optimize_three_view` returns `None` on the two in the middle
/// (cv-sfm/src/lib.rs:1949, 2026).
#[repr(u32)]
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum ThreeViewConstraintVerdict {
    Ok = 0,
    FewLandmarks = 1,
    FewBearingPairs = 2,
    BadIndex = 3,
}

/// Words of a constraint's `d_stats` row (`RS_TVC_S_*`).
pub const RS_TVC_STATS: usize = 8;

/// `VSlam::optimize_three_view` behind its shuffle and sort (cv-sfm/src/lib.rs:1939-2062) for many view triples side by
/// side (`rs_three_view_constraint_batch_device`), one wavefront per constraint.  Every `d_*` argument is device memory
/// the caller owns, laid out as include/akz.h documents; the call enqueues on `stream()` and returns.  The shuffle and the
/// unstable sort by observation count (lib.rs:1968-1977) stay with the caller, who owns the RNG.
pub struct ThreeViewConstraints {
    pub params: RsThreeViewConstraintParams,
    ctx: *mut c_void,
}
impl ThreeViewConstraints {
    pub fn new() -> Self {
        require_abi();
        let mut params: RsThreeViewConstraintParams = unsafe { std::mem::zeroed() };
        assert_eq!(unsafe { rs_three_view_constraint_params_default(&mut params) }, 0, "rs_three_view_constraint_params_default");
        let mut ctx = ptr::null_mut();
        assert_eq!(unsafe { rs_create(0, 8, 1, &mut ctx) }, 0, "rs_create");
        Self { params, ctx }
    }
    /// # Safety
    /// Every pointer names device memory of the documented size, alive until `sync()` returns.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn batch_device(&self, d_kps: *const c_void, cap_per_img: u32, n_blocks: u32, d_poses: *const c_void, cam: &RsCamera,
                               d_views: *const c_void, d_lm_start: *const c_void, d_lm: *const c_void, n_lm: u32, n_constraints: u32,
                               d_pose_out: *mut c_void, d_verdict: *mut c_void, d_stats: *mut c_void,
                               stream_to_wait: *mut c_void) -> Result<(), i32> {
        let st = rs_three_view_constraint_batch_device(self.ctx, d_kps, cap_per_img, n_blocks, d_poses, cam, d_views, d_lm_start, d_lm, n_lm,
                                                       n_constraints, &self.params, d_pose_out, d_verdict, d_stats, stream_to_wait);
        if st == 0 { Ok(()) } else { Err(st) }
    }
    pub fn sync(&self) {
        assert_eq!(unsafe { rs_sync(self.ctx) }, 0, "rs_sync");
    }
    pub fn stream(&self) -> *mut c_void {
        unsafe { rs_stream(self.ctx) }
    }
}
impl Default for ThreeViewConstraints {
    fn default() -> Self {
        Self::new()
    }
}
impl Drop for ThreeViewConstraints {
    fn drop(&mut self) {
        unsafe { rs_destroy(self.ctx) };
    }
}

/// `rs_pose_graph_params` (include/akz.h): cv-sfm's settings of the pose-graph relaxation
/// (cv-sfm/src/settings.rs:461-463, 477-479).
#[repr(C)]
#[derive(Clone, Copy)]
pub struct RsPoseGraphParams {
    struct_size: u32,
    pub optimization_iterations: u32,
    pub graph_optimization_rate: f64,
}

/// The verdict of one graph (`RS_PG_*`): `apply_constraints` removes the reconstruction on `FewViews`
/// (cv-sfm/src/lib.rs:2413) and panics in the round after `Nonfinite` unless that round was the last.
#[repr(u32)]
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum PoseGraphVerdict {
    Ok = 0,
    FewViews = 1,
    Nonfinite = 2,
    BadIndex = 3,
}

/// The state of one view (`RS_PG_VIEW_*`).
#[repr(u32)]
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum PoseGraphViewState {
    Updated = 0,
    NoConstraint = 1,
    Nonfinite = 2,
}

/// Words of a graph's `d_stats` row (`RS_PG_S_*`).
pub const RS_PG_STATS: usize = 8;
/// The most views the persistent workgroup can hold (`RS_PG_RESIDENT_VIEWS`) and the most it takes unless told otherwise
/// (`RS_PG_DEFAULT_RESIDENT_VIEWS`).
pub const RS_PG_RESIDENT_VIEWS: u32 = 256;
pub const RS_PG_DEFAULT_RESIDENT_VIEWS: u32 = 8;
/// Edge slot `s` of a constraint has target view `views[RS_PG_SLOT_TARGET[s]]` and other view `views[RS_PG_SLOT_OTHER[s]]`
/// (`ThreeViewConstraint::edge_constraints`, cv-sfm/src/lib.rs:167-180).
pub const RS_PG_SLOT_TARGET: [usize; 6] = [0, 0, 1, 1, 2, 2];
pub const RS_PG_SLOT_OTHER: [usize; 6] = [2, 1, 0, 2, 1, 0];

/// `VSlam::apply_constraints` (cv-sfm/src/lib.rs:2358-2375) for many reconstructions side by side
/// (`rs_pose_graph_edges_device`, `rs_pose_graph_relax_batch_device`), one wavefront per view and round.  Every `d_*`
/// argument is device memory the caller owns, laid out as include/akz.h documents; the calls enqueue on `stream()` and
/// return.  `flatten` builds the rows in the documented admissible order.
pub struct PoseGraph {
    pub params: RsPoseGraphParams,
    ctx: *mut c_void,
}
impl PoseGraph {
    pub fn new() -> Self {
        require_abi();
        let mut params: RsPoseGraphParams = unsafe { std::mem::zeroed() };
        assert_eq!(unsafe { rs_pose_graph_params_default(&mut params) }, 0, "rs_pose_graph_params_default");
        let mut ctx = ptr::null_mut();
        assert_eq!(unsafe { rs_create(0, 8, 1, &mut ctx) }, 0, "rs_create");
        Self { params, ctx }
    }
    /// `(row_start [n_views + 1], row_edges [6 n])` from the constraints' view triples: view `v`'s row holds the edge ids
    /// `6 * constraint + slot` whose target is `v`, constraint index ascending, slot order within a constraint.  `None`: a
    /// triple names a view `>= n_views`.
    pub fn flatten(views: &[[u32; 3]], n_views: u32) -> Option<(Vec<u32>, Vec<u32>)> {
        let mut rows: Vec<Vec<u32>> = vec![Vec::new(); n_views as usize];
        for (c, tri) in views.iter().enumerate() {
            for (slot, &t) in RS_PG_SLOT_TARGET.iter().enumerate() {
                rows.get_mut(tri[t] as usize)?.push((6 * c + slot) as u32);
            }
        }
        let mut row_start = vec![0u32];
        for row in &rows {
            row_start.push(row_start[row_start.len() - 1] + row.len() as u32);
        }
        Some((row_start, rows.concat()))
    }
    /// # Safety
    /// Every pointer names device memory of the documented size, alive until `sync()` returns.
    pub unsafe fn edges_device(&self, d_views: *const c_void, d_constraint_poses: *const c_void, d_constraint_verdict: *const c_void,
                               n_constraints: u32, d_edges: *mut c_void, stream_to_wait: *mut c_void) -> Result<(), i32> {
        let st = rs_pose_graph_edges_device(self.ctx, d_views, d_constraint_poses, d_constraint_verdict, n_constraints, d_edges, stream_to_wait);
        if st == 0 { Ok(()) } else { Err(st) }
    }
    /// # Safety
    /// Every pointer names device memory of the documented size, alive until `sync()` returns.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn relax_batch_device(&self, d_poses: *mut c_void, n_views: u32, d_graph_start: *const c_void, n_graphs: u32,
                                     d_row_start: *const c_void, d_row_edges: *const c_void, n_rows: u32, d_views: *const c_void,
                                     d_constraint_verdict: *const c_void, d_edges: *const c_void, n_constraints: u32,
                                     d_graph_verdict: *mut c_void, d_view_state: *mut c_void, d_stats: *mut c_void,
                                     stream_to_wait: *mut c_void) -> Result<(), i32> {
        let st = rs_pose_graph_relax_batch_device(self.ctx, d_poses, n_views, d_graph_start, n_graphs, d_row_start, d_row_edges, n_rows, d_views,
                                                  d_constraint_verdict, d_edges, n_constraints, &self.params, d_graph_verdict, d_view_state,
                                                  d_stats, stream_to_wait);
        if st == 0 { Ok(()) } else { Err(st) }
    }
    /// Parity tap (`rs_pose_graph_debug_resident_views`): graphs of more than `views` views (at most
    /// `RS_PG_RESIDENT_VIEWS`) take the swept form in the calls that follow; 0 sends every graph through it.
    pub fn resident_views(&self, views: u32) -> Result<(), i32> {
        let st = unsafe { rs_pose_graph_debug_resident_views(self.ctx, views) };
        if st == 0 { Ok(()) } else { Err(st) }
    }
    pub fn sync(&self) {
        assert_eq!(unsafe { rs_sync(self.ctx) }, 0, "rs_sync");
    }
    pub fn stream(&self) -> *mut c_void {
        unsafe { rs_stream(self.ctx) }
    }
}
impl Default for PoseGraph {
    fn default() -> Self {
        Self::new()
    }
}
impl Drop for PoseGraph {
    fn drop(&mut self) {
        unsafe { rs_destroy(self.ctx) };
    }
}

/// `rs_observation_filter_params` (include/akz.h): cv-sfm's settings of `filter_non_robust_observations` and
/// `optimize_reconstruction` (cv-sfm/src/settings.rs:324-350, 429-431).
#[repr(C)]
#[derive(Clone, Copy)]
pub struct RsObservationFilterParams {
    struct_size: u32,
    pub minimum_robust_landmarks: u32,
    pub maximum_cosine_distance: f64,
    pub maximum_sine_distance: f64,
    pub reconstruction_optimization_iterations: u32,
    reserved: u32,
    pub triangulate: RsTriangulateParams,
}

/// What became of a landmark (`RS_OF_*`, one byte of `d_lm_state`).
#[repr(u8)]
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum LandmarkState {
    Kept = 0,
    Single = 1,
    PairSplit = 2,
    NoPoint = 3,
    Kicked = 4,
    BadIndex = 5,
    Skipped = 6,
}

/// The filter's verdict on a reconstruction (`RS_OF_OK` ...): the reference removes it on `FewLandmarks`
/// (cv-sfm/src/lib.rs:2747-2753).
#[repr(u32)]
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum ObservationFilterVerdict {
    Ok = 0,
    FewLandmarks = 1,
    BadRange = 2,
    Skipped = 3,
}

/// Words of a reconstruction's `d_stats` row (`RS_OF_STATS`); `d_tri_reason` of a landmark without a solve
/// (`RS_OF_NO_SOLVE`); the bits of `d_robust`.
pub const RS_OF_STATS: usize = 8;
pub const RS_OF_NO_SOLVE: u8 = 255;
pub const RS_OF_ROBUST_BEFORE: u8 = 1;
pub const RS_OF_ROBUST_AFTER: u8 = 2;
/// A word of `optimize_reconstruction`'s `d_verdict`: 0, or `RS_OR_STOPPED | round << 16 | stage << 8 | the stage's verdict`.
pub const RS_OR_STOPPED: u32 = 1 << 30;
pub const RS_OR_STAGE_RELAX: u32 = 1;
pub const RS_OR_STAGE_FILTER: u32 = 2;

/// `VSlam::filter_non_robust_observations` (cv-sfm/src/lib.rs:2657-2757) for many reconstructions side by side
/// (`rs_filter_observations_device`) and `VSlam::optimize_reconstruction` (lib.rs:2343-2355) as a whole
/// (`rs_optimize_reconstruction_batch_device`).  Every `d_*` argument is device memory the caller owns, laid out as
/// include/akz.h documents; the calls enqueue on `stream()` and return.
pub struct ObservationFilter {
    pub params: RsObservationFilterParams,
    ctx: *mut c_void,
}
impl ObservationFilter {
    pub fn new() -> Self {
        require_abi();
        let mut params: RsObservationFilterParams = unsafe { std::mem::zeroed() };
        assert_eq!(unsafe { rs_observation_filter_params_default(&mut params) }, 0, "rs_observation_filter_params_default");
        let mut ctx = ptr::null_mut();
        assert_eq!(unsafe { rs_create(0, 8, 1, &mut ctx) }, 0, "rs_create");
        Self { params, ctx }
    }
    /// # Safety
    /// Every pointer names device memory of the documented size, alive until `sync()` returns.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn filter_device(&self, d_kps: *const c_void, cap_per_img: u32, n_blocks: u32, d_poses: *const c_void, cam: &RsCamera,
                                d_obs_start: *const c_void, d_obs: *const c_void, n_obs: u32, n_landmarks: u32, d_recon_start: *const c_void,
                                d_view_start: *const c_void, n_recons: u32, d_skip: *const c_void, d_keep: *mut c_void, d_lm_state: *mut c_void,
                                d_tri_reason: *mut c_void, d_robust: *mut c_void, d_obs_start_out: *mut c_void, d_obs_out: *mut c_void,
                                d_split_out: *mut c_void, d_counts: *mut c_void, d_recon_verdict: *mut c_void, d_stats: *mut c_void,
                                stream_to_wait: *mut c_void) -> Result<(), i32> {
        let st = rs_filter_observations_device(self.ctx, d_kps, cap_per_img, n_blocks, d_poses, cam, d_obs_start, d_obs, n_obs, n_landmarks,
                                               d_recon_start, d_view_start, n_recons, d_skip, &self.params, d_keep, d_lm_state, d_tri_reason,
                                               d_robust, d_obs_start_out, d_obs_out, d_split_out, d_counts, d_recon_verdict, d_stats,
                                               stream_to_wait);
        if st == 0 { Ok(()) } else { Err(st) }
    }
    /// `optimize_reconstruction`: `self.params.reconstruction_optimization_iterations` rounds of the relaxation (under
    /// `pg_params`) and the filter, then the world table of the final lists into `d_world` (may be null).
    /// # Safety
    /// Every pointer names device memory of the documented size, alive until `sync()` returns.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn optimize_reconstruction_device(&self, pg_params: &RsPoseGraphParams, d_poses: *mut c_void, n_views: u32,
                                                 d_graph_start: *const c_void, n_graphs: u32, d_row_start: *const c_void,
                                                 d_row_edges: *const c_void, n_rows: u32, d_views: *const c_void,
                                                 d_constraint_verdict: *const c_void, d_edges: *const c_void, n_constraints: u32,
                                                 d_kps: *const c_void, cap_per_img: u32, cam: &RsCamera, d_obs_start: *const c_void,
                                                 d_obs: *const c_void, n_obs: u32, n_landmarks: u32, d_recon_start: *const c_void,
                                                 d_verdict: *mut c_void, d_graph_verdict: *mut c_void, d_view_state: *mut c_void,
                                                 d_pg_stats: *mut c_void, d_keep: *mut c_void, d_lm_state: *mut c_void, d_tri_reason: *mut c_void,
                                                 d_robust: *mut c_void, d_obs_start_out: *mut c_void, d_obs_out: *mut c_void,
                                                 d_split_out: *mut c_void, d_counts: *mut c_void, d_recon_verdict: *mut c_void,
                                                 d_of_stats: *mut c_void, d_world: *mut c_void, d_world_reason: *mut c_void,
                                                 stream_to_wait: *mut c_void) -> Result<(), i32> {
        let st = rs_optimize_reconstruction_batch_device(self.ctx, d_poses, n_views, d_graph_start, n_graphs, d_row_start, d_row_edges, n_rows,
                                                         d_views, d_constraint_verdict, d_edges, n_constraints, pg_params, d_kps, cap_per_img, cam,
                                                         d_obs_start, d_obs, n_obs, n_landmarks, d_recon_start, &self.params, d_verdict,
                                                         d_graph_verdict, d_view_state, d_pg_stats, d_keep, d_lm_state, d_tri_reason, d_robust,
                                                         d_obs_start_out, d_obs_out, d_split_out, d_counts, d_recon_verdict, d_of_stats, d_world,
                                                         d_world_reason, stream_to_wait);
        if st == 0 { Ok(()) } else { Err(st) }
    }
    pub fn sync(&self) {
        assert_eq!(unsafe { rs_sync(self.ctx) }, 0, "rs_sync");
    }
    pub fn stream(&self) -> *mut c_void {
        unsafe { rs_stream(self.ctx) }
    }
}
impl Default for ObservationFilter {
    fn default() -> Self {
        Self::new()
    }
}
impl Drop for ObservationFilter {
    fn drop(&mut self) {
        unsafe { rs_destroy(self.ctx) };
    }
}

/// `rs_covisibility_params` (include/akz.h): cv-sfm's settings of `generate_view_constraints` and `record_view_constraints`
/// (cv-sfm/src/settings.rs:453-475), the slots per target and the seed that stands in for the shuffle.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct RsCovisibilityParams {
    struct_size: u32,
    pub optimization_robust_covisibility_minimum_landmarks: u32,
    pub optimization_maximum_three_view_constraints: u32,
    pub optimization_minimum_new_constraints: u32,
    pub optimization_minimum_landmarks: u32,
    pub optimization_maximum_landmarks: u32,
    pub candidate_limit: u32,
    pub shuffle_seed: u32,
}

/// A target's verdict (`RS_CV_OK` ...).
#[repr(u32)]
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum CovisibilityVerdict {
    Ok = 0,
    FewConstraints = 1,
    BadIndex = 2,
    NoGraph = 3,
}

/// `d_recorded` of an accepted constraint the record did not take; the capacities; the words of a target's `d_stats` row.
pub const RS_CV_NOT_RECORDED: u32 = 16;
pub const RS_CV_MAX_CANDIDATE_VIEWS: u32 = 128;
pub const RS_CV_MAX_SLOTS: u32 = 256;
pub const RS_CV_MAX_FEATURES: u32 = 8192;
pub const RS_CV_STATS: usize = 8;
pub const RS_CV_F_CANDIDATES_CAPPED: u32 = 1;
pub const RS_CV_F_LIMIT_REACHED: u32 = 2;

/// `VSlam::generate_view_constraints` up to its call of `optimize_three_view` (cv-sfm/src/lib.rs:2438-2516), the verdict of
/// `record_view_constraints` (lib.rs:2092-2109) and `flatten_constraints` (lib.rs:2519-2532) on a context the caller owns
/// (`ctx`: the one the constraint stage and the pose graph run on).  Every `d_*` argument is device memory the caller owns,
/// laid out as include/akz.h documents; the calls enqueue and return.
pub struct ViewConstraints {
    pub params: RsCovisibilityParams,
    ctx: *mut c_void,
}
impl ViewConstraints {
    /// # Safety
    /// `ctx` is a live `rs_ctx` that outlives this object.
    pub unsafe fn new(ctx: *mut c_void) -> Self {
        require_abi();
        let mut params: RsCovisibilityParams = std::mem::zeroed();
        assert_eq!(rs_covisibility_params_default(&mut params), 0, "rs_covisibility_params_default");
        Self { params, ctx }
    }
    /// slots per target
    pub fn limit(&self) -> u32 {
        if self.params.candidate_limit != 0 { self.params.candidate_limit } else { self.params.optimization_maximum_three_view_constraints }
    }
    /// # Safety
    /// Every pointer names device memory of the documented size, alive until the context's stream has run.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn candidates_device(&self, d_obs_start: *const c_void, d_obs: *const c_void, n_obs: u32, n_landmarks: u32, cap_per_img: u32,
                                    n_blocks: u32, d_reason: *const c_void, d_targets: *const c_void, n_targets: u32, d_views: *mut c_void,
                                    d_lm_start: *mut c_void, d_lm: *mut c_void, d_slot_count: *mut c_void, d_target_verdict: *mut c_void,
                                    d_stats: *mut c_void, stream_to_wait: *mut c_void) -> Result<(), i32> {
        let st = rs_covisibility_candidates_device(self.ctx, d_obs_start, d_obs, n_obs, n_landmarks, cap_per_img, n_blocks, d_reason, d_targets,
                                                   n_targets, &self.params, d_views, d_lm_start, d_lm, d_slot_count, d_target_verdict, d_stats,
                                                   stream_to_wait);
        if st == 0 { Ok(()) } else { Err(st) }
    }
    /// # Safety
    /// Every pointer names device memory of the documented size, alive until the context's stream has run.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn record_device(&self, d_constraint_verdict: *const c_void, d_targets: *const c_void, n_targets: u32,
                                d_graph_start: *const c_void, n_graphs: u32, d_recorded: *mut c_void, d_target_verdict: *mut c_void,
                                d_stats: *mut c_void, stream_to_wait: *mut c_void) -> Result<(), i32> {
        let st = rs_covisibility_record_device(self.ctx, d_constraint_verdict, d_targets, n_targets, d_graph_start, n_graphs, &self.params,
                                               d_recorded, d_target_verdict, d_stats, stream_to_wait);
        if st == 0 { Ok(()) } else { Err(st) }
    }
    /// `flatten_constraints` on the device: `d_row_start` [n_views + 1], `d_row_edges` [6 n], `d_flags` [1].
    /// # Safety
    /// Every pointer names device memory of the documented size, alive until the context's stream has run.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn rows_device(&self, d_views: *const c_void, n_constraints: u32, n_views: u32, d_row_start: *mut c_void,
                              d_row_edges: *mut c_void, d_flags: *mut c_void, stream_to_wait: *mut c_void) -> Result<(), i32> {
        let st = rs_pose_graph_rows_device(self.ctx, d_views, n_constraints, n_views, d_row_start, d_row_edges, d_flags, stream_to_wait);
        if st == 0 { Ok(()) } else { Err(st) }
    }
}

/// `rs_single_view_params` (include/akz.h): cv-sfm's settings of the single-view refinement (cv-sfm/src/settings.rs:324-383).
#[repr(C)]
#[derive(Clone, Copy)]
pub struct RsSingleViewParams {
    struct_size: u32,
    pub single_view_optimization_num_matches: u32,
    pub single_view_filter_loop_iterations: u32,
    pub single_view_patience: u32,
    pub single_view_optimization_rate: f64,
    pub single_view_minimum_landmarks: u32,
    pub single_view_minimum_robust_landmarks: u32,
    pub maximum_cosine_distance: f64,
    pub maximum_sine_distance: f64,
    pub triangulate: RsTriangulateParams,
}

/// The verdict on a new frame (`RS_SV_*`): the reference returns `None` on every one but `Ok`.
#[repr(u32)]
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum SingleViewVerdict {
    Ok = 0,
    NoModel = 1,
    FewLandmarks = 2,
    LostHalf = 3,
    FewRobust = 4,
    BadIndex = 5,
}

/// The limits of the refinement and the words of a scene's `d_stats` row.
pub const RS_SV_MAX_MATCHES: u32 = 2048;
pub const RS_SV_MAX_RUNS: u32 = 9;
pub const RS_SV_MAX_ITERATIONS: u32 = 1 << 20;
pub const RS_SV_STATS: usize = 24;
pub const RS_SV_S_INLIERS: usize = 0;
pub const RS_SV_S_RUN_MATCHES: usize = 1;
pub const RS_SV_S_RUN_STOP: usize = 10;
pub const RS_SV_S_ROBUST: usize = 19;
pub const RS_SV_S_NO_OTHER: usize = 20;
pub const RS_SV_S_STAGE: usize = 21;

/// What `register_frame_subset` does behind its consensus (cv-sfm/src/lib.rs:1625-1775) for the new frames of a micro-batch
/// (`rs_refine_poses_batch_device`), on the context of the consensus that registered them (not owned).  Every `d_*`
/// argument is device memory the caller owns, laid out as include/akz.h documents; the call enqueues and returns.
pub struct SingleViewRefiner {
    pub params: RsSingleViewParams,
    ctx: *mut c_void,
}
impl SingleViewRefiner {
    /// # Safety
    /// `ctx` is a live `rs_ctx` that outlives this object.
    pub unsafe fn new(ctx: *mut c_void) -> Self {
        require_abi();
        let mut params: RsSingleViewParams = std::mem::zeroed();
        assert_eq!(rs_single_view_params_default(&mut params), 0, "rs_single_view_params_default");
        Self { params, ctx }
    }
    /// # Safety
    /// Every pointer names device memory of the documented size, alive until the context's stream has run the call.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn refine_batch_device(&self, d_kps: *const c_void, cap_per_img: u32, n_blocks: u32, d_poses: *const c_void, cam: &RsCamera,
                                      d_obs_start: *const c_void, d_obs: *const c_void, n_obs: u32, n_landmarks: u32, d_world: *const c_void,
                                      n_world: u32, ik: &[u32], d_matches: *const c_void, d_nmatches: *const c_void, d_best: *const c_void,
                                      d_pose: *const c_void, d_best_id: *const c_void, d_inliers: *const c_void, d_n_inliers: *const c_void,
                                      d_pose_out: *mut c_void, d_verdict: *mut c_void, d_final: *mut c_void, d_n_final: *mut c_void,
                                      d_stats: *mut c_void, stream_to_wait: *mut c_void) -> Result<(), i32> {
        let st = rs_refine_poses_batch_device(self.ctx, d_kps, cap_per_img, n_blocks, d_poses, cam, d_obs_start, d_obs, n_obs, n_landmarks, d_world,
                                              n_world, ik.as_ptr(), d_matches, d_nmatches, d_best, d_pose, d_best_id, d_inliers, d_n_inliers,
                                              ik.len() as u32, &self.params, d_pose_out, d_verdict, d_final, d_n_final, d_stats, stream_to_wait);
        if st == 0 { Ok(()) } else { Err(st) }
    }
}

/// The verdict on a slot of `LandmarkBook::add_views` (`d_frame_verdict`) and on the call (`d_call_verdict`).
#[repr(u32)]
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum AddViewVerdict {
    Ok = 0,
    NotAccepted = 1,
    BadIndex = 2,
    BadTable = 3,
}

/// The words of a slot's `d_stats` row and of `d_counts_out`, and the rows of the input table one workgroup scans.
pub const RS_AV_STATS: usize = 4;
pub const RS_AV_S_OBSERVATIONS: usize = 0;
pub const RS_AV_S_MERGED: usize = 1;
pub const RS_AV_S_DEMOTED: usize = 2;
pub const RS_AV_S_NEW_LANDMARKS: usize = 3;
pub const RS_AV_COUNTS: usize = 4;
pub const RS_LT_TILE: u32 = 1024;

/// cv-sfm's landmark bookkeeping around the registration of a micro-batch: `are_landmarks_sharing_view` for the merge
/// candidates (cv-sfm/src/lib.rs:1435-1449, `rs_landmarks_sharing_view_device`) and `add_view` with `merge_landmarks` for the
/// accepted frames (lib.rs:432-483, 699-721, `rs_add_views_device`), on the context of the consensus that registered them (not
/// owned).  Every `d_*` argument is device memory the caller owns, laid out as include/akz.h documents; the calls enqueue and
/// return.
pub struct LandmarkBook {
    ctx: *mut c_void,
}
impl LandmarkBook {
    /// # Safety
    /// `ctx` is a live `rs_ctx` that outlives this object.
    pub unsafe fn new(ctx: *mut c_void) -> Self {
        require_abi();
        Self { ctx }
    }
    /// # Safety
    /// Every pointer names device memory of the documented size, alive until the context's stream has run the call.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn sharing_view(&self, d_obs_start: *const c_void, d_obs: *const c_void, n_obs: u32, n_landmarks: u32, d_best: *const c_void,
                               d_decision: *const c_void, cap_per_img: u32, n_frames: u32, d_merge_ok: *mut c_void,
                               stream_to_wait: *mut c_void) -> Result<(), i32> {
        let st = rs_landmarks_sharing_view_device(self.ctx, d_obs_start, d_obs, n_obs, n_landmarks, d_best, d_decision, cap_per_img, n_frames,
                                                  d_merge_ok, stream_to_wait);
        if st == 0 { Ok(()) } else { Err(st) }
    }
    /// # Safety
    /// Every pointer names device memory of the documented size, alive until the context's stream has run the call.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn add_views(&self, d_obs_start: *const c_void, d_obs: *const c_void, n_obs: u32, n_landmarks: u32, n_world: u32,
                            d_split: *const c_void, d_split_count: *const c_void, split_room: u32, cap_per_img: u32, n_blocks: u32, ik: &[u32],
                            d_counts: *const c_void, d_matches: *const c_void, d_nmatches: *const c_void, d_final: *const c_void,
                            d_verdict: *const c_void, d_pose_out: *const c_void, d_best: *const c_void, d_skip: *const c_void, obs_room: u32,
                            lm_room: u32, d_poses: *mut c_void, d_obs_start_out: *mut c_void, d_obs_out: *mut c_void,
                            d_counts_out: *mut c_void, d_landmarks_out: *mut c_void, d_obs_counts_out: *mut c_void,
                            d_frame_verdict: *mut c_void, d_stats: *mut c_void, d_call_verdict: *mut c_void,
                            stream_to_wait: *mut c_void) -> Result<(), i32> {
        let st = rs_add_views_device(self.ctx, d_obs_start, d_obs, n_obs, n_landmarks, n_world, d_split, d_split_count, split_room, cap_per_img,
                                     n_blocks, ik.as_ptr(), ik.len() as u32, d_counts, d_matches, d_nmatches, d_final, d_verdict, d_pose_out,
                                     d_best, d_skip, obs_room, lm_room, d_poses, d_obs_start_out, d_obs_out, d_counts_out, d_landmarks_out,
                                     d_obs_counts_out, d_frame_verdict, d_stats, d_call_verdict, stream_to_wait);
        if st == 0 { Ok(()) } else { Err(st) }
    }
}

/// The verdict on `ReconstructionMerge::incorporate` (`d_call_verdict`).
#[repr(u32)]
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum IncorporateVerdict {
    Ok = 0,
    BadTable = 1,
    BadIndex = 2,
    SharedBlock = 3,
}

/// The verdict on `ReconstructionMerge::normalize` (`d_verdict`).
#[repr(u32)]
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum NormalizeVerdict {
    Ok = 0,
    NotNormal = 1,
    BadIndex = 2,
}

/// The words of `d_counts_out` of `ReconstructionMerge::incorporate`.
pub const RS_IR_C_ROWS: usize = 0;
pub const RS_IR_C_OBSERVATIONS: usize = 1;
pub const RS_IR_C_APPLIED: usize = 2;
pub const RS_IR_C_DEMOTED: usize = 3;
pub const RS_IR_C_NEW_ROWS: usize = 4;
pub const RS_IR_C_DROPPED: usize = 5;
pub const RS_IR_COUNTS: usize = 6;

/// cv-sfm's loop closure between two reconstructions and its normalisation: the landmark map of the bridging frame
/// (cv-sfm/src/lib.rs:2159-2170, `rs_merge_map_device`), `incorporate_reconstruction` (lib.rs:1817-1887,
/// `rs_incorporate_reconstruction_device`) and `normalize_reconstruction` (lib.rs:2241-2283,
/// `rs_normalize_reconstruction_device`), on the context of the consensus that registered the bridging frame (not owned).
/// Every `d_*` argument is device memory the caller owns, laid out as include/akz.h documents; the calls enqueue and return.
/// Like the other declarations of this file these are source only: they are not compiled here (no toolchain).
pub struct ReconstructionMerge {
    ctx: *mut c_void,
}
impl ReconstructionMerge {
    /// # Safety
    /// `ctx` is a live `rs_ctx` that outlives this object.
    pub unsafe fn new(ctx: *mut c_void) -> Self {
        require_abi();
        Self { ctx }
    }
    /// # Safety
    /// Every pointer names device memory of the documented size, alive until the context's stream has run the call.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn merge_map(&self, d_matches: *const c_void, d_nmatches: *const c_void, d_final: *const c_void, d_best: *const c_void,
                            n_world: u32, n_dst_landmarks: u32, cap_per_img: u32, slot: u32, d_counts: *const c_void,
                            d_src_landmarks: *const c_void, n_blocks: u32, bridge_block: u32, d_map: *mut c_void, d_map_count: *mut c_void,
                            stream_to_wait: *mut c_void) -> Result<(), i32> {
        let st = rs_merge_map_device(self.ctx, d_matches, d_nmatches, d_final, d_best, n_world, n_dst_landmarks, cap_per_img, slot, d_counts,
                                     d_src_landmarks, n_blocks, bridge_block, d_map, d_map_count, stream_to_wait);
        if st == 0 { Ok(()) } else { Err(st) }
    }
    /// # Safety
    /// Every pointer names device memory of the documented size, alive until the context's stream has run the call.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn incorporate(&self, d_dst_start: *const c_void, d_dst_obs: *const c_void, n_dst_obs: u32, n_dst_landmarks: u32,
                              d_src_start: *const c_void, d_src_obs: *const c_void, n_src_obs: u32, n_src_landmarks: u32,
                              d_map: *const c_void, d_map_count: *const c_void, map_room: u32, cap_per_img: u32, n_blocks: u32,
                              src_blocks: &[u32], bridge_block: u32, d_src_pose: *const c_void, d_skip: *const c_void, obs_room: u32,
                              lm_room: u32, d_poses: *mut c_void, d_obs_start_out: *mut c_void, d_obs_out: *mut c_void,
                              d_counts_out: *mut c_void, d_landmarks_out: *mut c_void, d_obs_counts_out: *mut c_void,
                              d_src_key_out: *mut c_void, d_call_verdict: *mut c_void, stream_to_wait: *mut c_void) -> Result<(), i32> {
        let st = rs_incorporate_reconstruction_device(self.ctx, d_dst_start, d_dst_obs, n_dst_obs, n_dst_landmarks, d_src_start, d_src_obs,
                                                      n_src_obs, n_src_landmarks, d_map, d_map_count, map_room, cap_per_img, n_blocks,
                                                      src_blocks.as_ptr(), src_blocks.len() as u32, bridge_block, d_src_pose, d_skip,
                                                      obs_room, lm_room, d_poses, d_obs_start_out, d_obs_out, d_counts_out,
                                                      d_landmarks_out, d_obs_counts_out, d_src_key_out, d_call_verdict, stream_to_wait);
        if st == 0 { Ok(()) } else { Err(st) }
    }
    /// # Safety
    /// Every pointer names device memory of the documented size, alive until the context's stream has run the call.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn normalize(&self, view_blocks: &[u32], d_counts: *const c_void, d_landmarks: *const c_void, cap_per_img: u32, n_blocks: u32,
                            d_world: *const c_void, n_world: u32, d_poses: *mut c_void, d_constraint_poses: *mut c_void,
                            n_constraints: u32, d_stats: *mut c_void, d_verdict: *mut c_void, stream_to_wait: *mut c_void) -> Result<(), i32> {
        let st = rs_normalize_reconstruction_device(self.ctx, view_blocks.as_ptr(), view_blocks.len() as u32, d_counts, d_landmarks,
                                                    cap_per_img, n_blocks, d_world, n_world, d_poses, d_constraint_poses, n_constraints,
                                                    d_stats, d_verdict, stream_to_wait);
        if st == 0 { Ok(()) } else { Err(st) }
    }
}

/// The verdict on `ReconstructionExport::export_device` (`d_verdict`).
#[repr(u32)]
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum ExportVerdict {
    Ok = 0,
    Overflow = 1,
    BadTable = 2,
}

/// The words of `d_counts_out` of `ReconstructionExport::export_device`, the words of a camera row and a camera's vertices.
pub const RS_EX_C_POINTS: usize = 0;
pub const RS_EX_C_NO_POINT: usize = 1;
pub const RS_EX_C_INFINITE: usize = 2;
pub const RS_EX_C_BAD_ROWS: usize = 3;
pub const RS_EX_COUNTS: usize = 4;
pub const RS_EX_CAMERA_WORDS: usize = 10;
pub const RS_EX_CAMERA_VERTICES: usize = 5;

/// `VSlam::export_reconstruction` (cv-sfm/src/lib.rs:2285-2340) with export.rs: the coloured point cloud and the cameras'
/// frusta as the vertex arrays of the .ply file (`rs_export_reconstruction_device`), on the context of the consensus whose
/// stream made the world table (not owned), and the file's text (`rs_write_ply`, host code).  Every `d_*` argument is device
/// memory the caller owns, laid out as include/akz.h documents; `export_device` enqueues and returns.
/// Like the other declarations of this file these are source only: they are not compiled here (no toolchain).
pub struct ReconstructionExport {
    ctx: *mut c_void,
}
impl ReconstructionExport {
    /// # Safety
    /// `ctx` is a live `rs_ctx` that outlives this object.
    pub unsafe fn new(ctx: *mut c_void) -> Self {
        require_abi();
        Self { ctx }
    }
    /// # Safety
    /// Every pointer names device memory of the documented size, alive until the context's stream has run the call.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn export_device(&self, d_world: *const c_void, n_world: u32, d_obs_start: *const c_void, d_obs: *const c_void, n_obs: u32,
                                n_landmarks: u32, d_colors: *const c_void, view_blocks: &[u32], d_counts: *const c_void,
                                d_landmarks: *const c_void, cap_per_img: u32, n_blocks: u32, d_poses: *const c_void, room: u32,
                                d_xyz: *mut c_void, d_rgb: *mut c_void, d_key: *mut c_void, d_cameras: *mut c_void,
                                d_counts_out: *mut c_void, d_verdict: *mut c_void, stream_to_wait: *mut c_void) -> Result<(), i32> {
        let st = rs_export_reconstruction_device(self.ctx, d_world, n_world, d_obs_start, d_obs, n_obs, n_landmarks, d_colors,
                                                 view_blocks.as_ptr(), view_blocks.len() as u32, d_counts, d_landmarks, cap_per_img, n_blocks,
                                                 d_poses, room, d_xyz, d_rgb, d_key, d_cameras, d_counts_out, d_verdict, stream_to_wait);
        if st == 0 { Ok(()) } else { Err(st) }
    }
    /// Host arrays `xyz` [n][3] and `rgb` [n][3] whose first `5 * n_cameras` rows are the cameras' vertices -> the file.
    pub fn write_ply(path: &std::ffi::CStr, xyz: &[f64], rgb: &[u8], n_cameras: u32, camera_faces: bool) -> Result<(), i32> {
        if xyz.len() != rgb.len() || xyz.len() % 3 != 0 { return Err(-1); }
        let st = unsafe { rs_write_ply(path.as_ptr(), xyz.as_ptr(), rgb.as_ptr(), (xyz.len() / 3) as u32, n_cameras, camera_faces as i32) };
        if st == 0 { Ok(()) } else { Err(st) }
    }
}

/// The verdict on a scene of `ReconstructionStart::join_pairs_device` (`RS_JP_*` of include/akz.h).
#[repr(u32)]
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum JoinVerdict {
    Ok = 0,
    NoModel = 1,
    FewInliers = 2,
    BadIndex = 3,
}
/// The verdict on a scene, and on a call, of `ReconstructionStart::add_reconstruction_device` (`RS_AR_*`).
#[repr(u32)]
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum AddReconstructionVerdict {
    Ok = 0,
    NotAccepted = 1,
    BadIndex = 2,
    Taken = 3,
    BadTable = 4,
}
pub const RS_JP_DEFAULT_MINIMUM_ROBUST_MATCHES: u32 = 256;
pub const RS_JP_MAX_FEATURES: u32 = 9216;
pub const RS_AR_S_TRIPLES: usize = 0;
pub const RS_AR_S_FIRST: usize = 1;
pub const RS_AR_S_SECOND: usize = 2;
pub const RS_AR_S_LANDMARKS: usize = 3;
pub const RS_AR_STATS: usize = 4;
pub const RS_AR_COUNTS: usize = 4;

/// The two integer steps of cv-sfm's `try_init` around the three-view bootstrap (`rs_join_pairs_batch_device`: the join and
/// shuffle of `init_reconstruction`, cv-sfm/src/lib.rs:992-999; `rs_add_reconstruction_batch_device`: `add_reconstruction`,
/// lib.rs:377-427), on the context of the consensus whose stream made the inlier lists (not owned).  Every `d_*` argument is
/// device memory the caller owns, laid out as include/akz.h documents; both calls enqueue and return.
/// Like the other declarations of this file these are source only: they are not compiled here (no toolchain).
pub struct ReconstructionStart {
    ctx: *mut c_void,
}
impl ReconstructionStart {
    /// # Safety
    /// `ctx` is a live `rs_ctx` that outlives this object.
    pub unsafe fn new(ctx: *mut c_void) -> Self {
        require_abi();
        Self { ctx }
    }
    /// # Safety
    /// Every pointer names device memory of the documented size, alive until the context's stream has run the call.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn join_pairs_device(&self, d_pairs: *const c_void, d_npairs: *const c_void, d_inliers: *const c_void, d_n_inliers: *const c_void,
                                           d_best_id: *const c_void, d_pose: *const c_void, n_slots: u32, cap_per_img: u32, slot_first: &[u32],
                                           slot_second: &[u32], two_view_minimum_robust_matches: u32, flags: u32, seed: u64, d_triples: *mut c_void,
                                           d_ntriples: *mut c_void, d_first_only: *mut c_void, d_nfirst: *mut c_void, d_second_only: *mut c_void,
                                           d_nsecond: *mut c_void, d_pose_first: *mut c_void, d_pose_second: *mut c_void, d_verdict: *mut c_void,
                                           stream_to_wait: *mut c_void) -> Result<(), i32> {
        if slot_second.len() != slot_first.len() { return Err(-1); }
        let st = rs_join_pairs_batch_device(self.ctx, d_pairs, d_npairs, d_inliers, d_n_inliers, d_best_id, d_pose, n_slots, cap_per_img,
                                            slot_first.as_ptr(), slot_second.as_ptr(), slot_first.len() as u32, two_view_minimum_robust_matches,
                                            flags, seed, d_triples, d_ntriples, d_first_only, d_nfirst, d_second_only, d_nsecond, d_pose_first,
                                            d_pose_second, d_verdict, stream_to_wait);
        if st == 0 { Ok(()) } else { Err(st) }
    }
    /// # Safety
    /// Every pointer names device memory of the documented size, alive until the context's stream has run the call.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn add_reconstruction_device(&self, d_triples: *const c_void, d_ntriples: *const c_void, d_first_only: *const c_void,
                                                   d_nfirst: *const c_void, d_second_only: *const c_void, d_nsecond: *const c_void,
                                                   d_combined: *const c_void, d_first_ok: *const c_void, d_second_ok: *const c_void,
                                                   d_pose_out: *const c_void, d_verdict: *const c_void, ic: &[u32], i_first: &[u32], i_second: &[u32],
                                                   d_kps: *const c_void, d_counts: *const c_void, n_src_blocks: u32, cap_per_img: u32,
                                                   d_skip: *const c_void, d_obs_start: *const c_void, d_obs: *const c_void, n_obs: u32,
                                                   n_landmarks: u32, d_recon_start: *const c_void, d_view_start: *const c_void, n_recons: u32,
                                                   d_kps_dst: *mut c_void, d_counts_dst: *mut c_void, d_poses: *mut c_void, n_blocks: u32,
                                                   view_base: u32, obs_room: u32, lm_room: u32, d_obs_start_out: *mut c_void, d_obs_out: *mut c_void,
                                                   d_obs_counts_out: *mut c_void, d_counts_out: *mut c_void, d_landmarks_out: *mut c_void,
                                                   d_recon_start_out: *mut c_void, d_view_start_out: *mut c_void, d_views_out: *mut c_void,
                                                   d_constraint_poses_out: *mut c_void, d_constraint_verdict_out: *mut c_void,
                                                   d_frame_verdict: *mut c_void, d_stats: *mut c_void, d_call_verdict: *mut c_void,
                                                   stream_to_wait: *mut c_void) -> Result<(), i32> {
        if i_first.len() != ic.len() || i_second.len() != ic.len() { return Err(-1); }
        let st = rs_add_reconstruction_batch_device(self.ctx, d_triples, d_ntriples, d_first_only, d_nfirst, d_second_only, d_nsecond, d_combined,
                                                    d_first_ok, d_second_ok, d_pose_out, d_verdict, ic.as_ptr(), i_first.as_ptr(), i_second.as_ptr(),
                                                    ic.len() as u32, d_kps, d_counts, n_src_blocks, cap_per_img, d_skip, d_obs_start, d_obs, n_obs,
                                                    n_landmarks, d_recon_start, d_view_start, n_recons, d_kps_dst, d_counts_dst, d_poses, n_blocks,
                                                    view_base, obs_room, lm_room, d_obs_start_out, d_obs_out, d_obs_counts_out, d_counts_out,
                                                    d_landmarks_out, d_recon_start_out, d_view_start_out, d_views_out, d_constraint_poses_out,
                                                    d_constraint_verdict_out, d_frame_verdict, d_stats, d_call_verdict, stream_to_wait);
        if st == 0 { Ok(()) } else { Err(st) }
    }
}

/// `hm_place_params` of include/akz.h (the defaults: cv-sfm/src/settings.rs:437-451).
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct HmPlaceParams {
    pub num_similar: u32,
    pub num_recent: u32,
    pub recent_threshold: u32,
    pub search_num: u32,
}
#[repr(u32)]
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum PlaceVerdict {
    Ok = 0,
    BadIndex = 1,
    BadTable = 2,
}
pub const HM_PL_OK: u32 = 0;
pub const HM_PL_BAD_INDEX: u32 = 1;
pub const HM_PL_BAD_TABLE: u32 = 2;
pub const HM_PL_C_RECENT: usize = 0;
pub const HM_PL_C_SIMILAR: usize = 1;
pub const HM_PL_C_SEARCHED: usize = 2;
pub const HM_PL_C_GROUPS: usize = 3;
pub const HM_PL_C_FREE: usize = 4;
pub const HM_PL_COUNTS: usize = 5;
pub const HM_PL_MAX_HASH_BYTES: u32 = 4096;
pub const HM_PL_MAX_SEARCH: u32 = 2048;
pub const HM_PL_MAX_RECENT: u32 = 256;
pub const HM_PL_NONE: u32 = 0xFFFF_FFFF;
#[repr(u32)]
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum PlanVerdict {
    Ok = 0,
    Cut = 1,
    NoGroup = 2,
    FindRefused = 3,
    BadView = 4,
    NoRoom = 5,
}
pub const HM_VP_OK: u32 = 0;
pub const HM_VP_CUT: u32 = 1;
pub const HM_VP_NO_GROUP: u32 = 2;
pub const HM_VP_FIND_REFUSED: u32 = 3;
pub const HM_VP_BAD_VIEW: u32 = 4;
pub const HM_VP_NO_ROOM: u32 = 5;
pub const HM_VP_C_BLOCKS: usize = 0;
pub const HM_VP_C_LIVE: usize = 1;
pub const HM_VP_C_VERDICT: usize = 2;
pub const HM_VP_C_FRAMES: usize = 3;
pub const HM_VP_COUNTS: usize = 4;
pub const HM_VP_PICK_RECON: u32 = 1;
pub const HM_VP_MAX_VIEWS: u32 = 64;

/// The outputs of `hm_view_plan_device`, device memory the caller owns: `view_idx [n_frames][n_views]`, `n_views_of [n_frames]`,
/// `verdict [n_frames]`, `counts [HM_VP_COUNTS]` u32; and the rooms the planned calls size their grids from.
#[derive(Clone, Copy, Debug)]
pub struct ViewPlan {
    pub view_idx: *mut c_void,
    pub n_views_of: *mut c_void,
    pub verdict: *mut c_void,
    pub counts: *mut c_void,
    pub n_frames: u32,
    pub n_views: u32,
    pub n_blocks: u32,
    pub exp_blocks: u32,
}

/// The rows `[first, first + count)` of a [`FrameIndex`]: their addresses in the table's five arrays.
#[derive(Clone, Copy, Debug)]
pub struct FrameRows {
    pub first: u32,
    pub count: u32,
    pub hashes: *mut c_void,
    pub feed: *mut c_void,
    pub pos: *mut c_void,
    pub recon: *mut c_void,
    pub view: *mut c_void,
}

/// Which frames a frame is compared with (`hm_find_frames_batch_device`: `find_visually_similar_and_recent_frames`,
/// cv-sfm/src/lib.rs:597-668, and the order `try_localize` gives its reconstructions, :853-855), for a batch of queries on the
/// matcher's stream.  The frame table is device memory the caller owns, laid out as include/akz.h documents; this struct keeps
/// its five addresses, its capacity and its row count.  The rows' feed / pos / recon / view words are copied by the caller to the
/// addresses `append_rows` / `set_views` hand out; the hashes are written by `hm_hash_bag_device`, whose `d_hash` is the tail.
/// Like the other declarations of this file these are source only: they are not compiled here (no toolchain).
pub struct FrameIndex {
    ctx: *mut c_void,
    hashes: *mut c_void,
    feed: *mut c_void,
    pos: *mut c_void,
    recon: *mut c_void,
    view: *mut c_void,
    capacity: u32,
    hash_bytes: u32,
    n: u32,
}
impl FrameIndex {
    /// # Safety
    /// `ctx` is a live `hm_ctx` that outlives this object; the five pointers name device arrays of `capacity` rows.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn new(ctx: *mut c_void, d_hashes: *mut c_void, d_feed: *mut c_void, d_pos: *mut c_void, d_recon: *mut c_void,
                      d_view: *mut c_void, capacity: u32, hash_bytes: u32) -> Result<Self, i32> {
        require_abi();
        if hash_bytes == 0 || hash_bytes % 4 != 0 || hash_bytes > HM_PL_MAX_HASH_BYTES { return Err(-1); }
        Ok(Self { ctx, hashes: d_hashes, feed: d_feed, pos: d_pos, recon: d_recon, view: d_view, capacity, hash_bytes, n: 0 })
    }
    pub fn params() -> HmPlaceParams {
        let mut p = HmPlaceParams { num_similar: 0, num_recent: 0, recent_threshold: 0, search_num: 0 };
        unsafe { hm_place_params_default(&mut p) };
        p
    }
    pub fn room(p: &HmPlaceParams) -> u32 {
        unsafe { hm_place_room(p) }
    }
    pub fn len(&self) -> u32 {
        self.n
    }
    pub fn is_empty(&self) -> bool {
        self.n == 0
    }
    fn rows(&self, first: u32, count: u32) -> FrameRows {
        let at = |base: *mut c_void, width: usize| (base as *mut u8).wrapping_add(width * first as usize) as *mut c_void;
        FrameRows { first, count, hashes: at(self.hashes, self.hash_bytes as usize), feed: at(self.feed, 4), pos: at(self.pos, 4),
                    recon: at(self.recon, 4), view: at(self.view, 4) }
    }
    /// `k` frames appended in insertion order -> where their rows lie.  They have no view until `set_views`: the caller writes
    /// `HM_PL_NONE` to their recon words with the feed and pos.
    pub fn append_rows(&mut self, k: u32) -> Result<FrameRows, i32> {
        if k > self.capacity - self.n { return Err(-6); }
        let r = self.rows(self.n, k);
        self.n += k;
        Ok(r)
    }
    /// `Frame::view` of the stored rows `[first, first + k)`: where the caller copies their reconstruction and view keys.
    pub fn set_views(&self, first: u32, k: u32) -> Result<FrameRows, i32> {
        if first > self.n || k > self.n - first { return Err(-1); }
        Ok(self.rows(first, k))
    }
    /// # Safety
    /// Every pointer names device memory of the documented size, alive until the matcher's stream has run the call.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn find(&self, d_query: *const c_void, d_visible: *const c_void, nq: u32, params: &HmPlaceParams, room: u32,
                       d_found: *mut c_void, d_views_out: *mut c_void, d_group_recon: *mut c_void, d_group_start: *mut c_void,
                       d_free: *mut c_void, d_search: *mut c_void, d_counts: *mut c_void, d_verdict: *mut c_void,
                       stream_to_wait: *mut c_void) -> Result<(), i32> {
        let st = hm_find_frames_batch_device(self.ctx, self.hashes, self.feed, self.pos, self.recon, self.view, self.n, self.hash_bytes,
                                             d_query, d_visible, nq, params, room, d_found, d_views_out, d_group_recon, d_group_start, d_free,
                                             d_search, d_counts, d_verdict, stream_to_wait);
        if st == 0 { Ok(()) } else { Err(st) }
    }
    /// From a find's outputs to the views every frame is matched against (`hm_view_plan_device`): ONE found reconstruction per
    /// frame — `try_localize`'s turn (cv-sfm/src/lib.rs:858-891; `d_pick` null: the first) or, `by_recon`, the named one
    /// (`.remove(&reconstruction)`, :926-939) — at most `plan.n_views` of its views.
    /// # Safety
    /// Every pointer names device memory of the documented size, alive until the matcher's stream has run the call.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn plan_views(&self, d_views_out: *const c_void, d_group_recon: *const c_void, d_group_start: *const c_void,
                             d_counts: *const c_void, d_verdict: *const c_void, room: u32, d_pick: *const c_void, by_recon: bool,
                             plan: &ViewPlan, stream_to_wait: *mut c_void) -> Result<(), i32> {
        let st = hm_view_plan_device(self.ctx, d_views_out, d_group_recon, d_group_start, d_counts, d_verdict, room, d_pick,
                                     if by_recon { HM_VP_PICK_RECON } else { 0 }, plan.n_frames, plan.n_views, plan.n_blocks, plan.exp_blocks,
                                     plan.view_idx, plan.n_views_of, plan.verdict, plan.counts, stream_to_wait);
        if st == 0 { Ok(()) } else { Err(st) }
    }
    /// `hm_knn_planned_batch_device`: the frames' blocks `iq` (host) against the views of their lists; `d_out
    /// [n_frames][n_views][cap][k]`, the slabs behind a frame's list not written.
    /// # Safety
    /// As `plan_views`; `iq` names `plan.n_frames` words.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn knn_planned(&self, d_descs: *const c_void, d_counts: *const c_void, cap_per_img: u32, iq: *const u32, plan: &ViewPlan,
                              k: u32, d_out: *mut c_void, stream_to_wait: *mut c_void) -> Result<(), i32> {
        let st = hm_knn_planned_batch_device(self.ctx, d_descs, d_counts, d_descs, d_counts, cap_per_img, iq, plan.view_idx, plan.n_views_of,
                                             plan.n_frames, plan.n_views, plan.n_blocks, plan.exp_blocks, k, d_out, stream_to_wait);
        if st == 0 { Ok(()) } else { Err(st) }
    }
    /// `hm_best_of_views_planned_batch_device` over those lists.
    /// # Safety
    /// As `knn_planned`.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn best_of_views_planned(&self, d_knn: *const c_void, d_counts: *const c_void, cap_per_img: u32, iq: *const u32,
                                        plan: &ViewPlan, k: u32, d_landmarks: *const c_void, better_by: u32, d_best: *mut c_void,
                                        d_decision: *mut c_void, stream_to_wait: *mut c_void) -> Result<(), i32> {
        let st = hm_best_of_views_planned_batch_device(self.ctx, d_knn, d_counts, iq, cap_per_img, plan.view_idx, plan.n_views_of,
                                                       plan.n_frames, plan.n_views, plan.n_blocks, k, d_landmarks, d_counts, better_by,
                                                       d_best, d_decision, stream_to_wait);
        if st == 0 { Ok(()) } else { Err(st) }
    }
}
