/* The CPU checker of the reconstruction-merge kernels: the host's execution of each whole procedure is in
 * include/akz_reconstruction_merge_math.h itself (the kernels' loops of cv_amd/csrc/rs_reconstruction_merge.hip one after
 * another, around the decisions and the arithmetic the kernels compile for the device); this file exports it.
 * tests/reconstruction_merge_checker.py has tests/host_build.py build it with the host compiler into a shared object and loads
 * it with ctypes.  Every output buffer is produced whole: what the device call does not write is not written here either, so
 * that both sides can start from one fill. */
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/akz_reconstruction_merge_math.h"

/* rs_merge_map_device on host arrays.  -1: out of memory. */
int mr_merge_map(const uint32_t* matches, const uint32_t* nmatches, const unsigned char* final_mask, const uint32_t* best, uint32_t n_world,
                 uint32_t n_dst_landmarks, uint32_t cap, uint32_t slot, const uint32_t* counts, const uint32_t* src_landmarks, uint32_t n_blocks,
                 uint32_t bridge_block, uint32_t* map, uint32_t* map_count)
{
    uint32_t* feat = (uint32_t*)malloc(((size_t)cap + 1) * sizeof(uint32_t));
    (void)n_blocks;
    if (!feat) return -1;
    akz_mr_merge_map(matches, nmatches, final_mask, best, n_world, n_dst_landmarks, cap, slot, counts, src_landmarks, bridge_block, feat, map,
                     map_count);
    free(feat);
    return 0;
}

/* rs_incorporate_reconstruction_device on host arrays (the refusals of the entry point are not restated: the caller keeps its
 * rooms).  -1: out of memory. */
int mr_incorporate(const uint32_t* dst_start, const uint32_t* dst_obs, uint32_t n_dst_obs, uint32_t n_dst, const uint32_t* src_start,
                   const uint32_t* src_obs, uint32_t n_src_obs, uint32_t n_src, const uint32_t* map, const uint32_t* map_count, uint32_t map_room,
                   uint32_t cap, uint32_t n_blocks, const uint32_t* src_blocks, uint32_t n_src_views, uint32_t bridge_block, const double* src_pose,
                   const uint32_t* skip, uint32_t obs_room, uint32_t lm_room, double* poses, uint32_t* obs_start_out, uint32_t* obs_out,
                   uint32_t* counts_out, uint32_t* landmarks_out, uint32_t* obs_counts_out, uint32_t* src_key_out, uint32_t* call_verdict)
{
    return akz_ir_incorporate(dst_start, dst_obs, n_dst_obs, n_dst, src_start, src_obs, n_src_obs, n_src, map, map_count, map_room, cap, n_blocks,
                              src_blocks, n_src_views, bridge_block, src_pose, skip, obs_room, lm_room, poses, obs_start_out, obs_out, counts_out,
                              landmarks_out, obs_counts_out, src_key_out, call_verdict);
}

/* rs_normalize_reconstruction_device on host arrays */
void mr_normalize(const uint32_t* view_blocks, uint32_t n_views, const uint32_t* counts, const uint32_t* landmarks, uint32_t cap, uint32_t n_blocks,
                  const double* world, uint32_t n_world, double* poses, double* constraint_poses, uint32_t n_constraints, double* stats,
                  uint32_t* verdict)
{
    akz_nr_normalize(view_blocks, n_views, counts, landmarks, cap, n_blocks, world, n_world, poses, constraint_poses, n_constraints, stats, verdict);
}

/* ---- the pieces, for the rule tests ---- */
int mr_is_normal(double x) { return akz_nr_is_normal(x); }
void mr_transform(const double* src_pose, const double* dest_pose, double* t) { akz_ir_transform(src_pose, dest_pose, t); }
