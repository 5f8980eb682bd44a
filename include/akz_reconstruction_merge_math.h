/* akz_reconstruction_merge_math.h — cv-sfm's loop closure between two reconstructions and its normalisation: the landmark map
 * of a bridging frame, incorporate_reconstruction over two CSR landmark tables, normalize_reconstruction.  Integer decisions and
 * the pose arithmetic, written once for gcc (the CPU checker, tests/cpp/reconstruction_merge_host.c) and hipcc (the gfx950
 * kernels of cv_amd/csrc/rs_reconstruction_merge.hip): parity is "host build == HIP" in every byte of every output.
 *
 * Reference code restated here (paths relative to rust-cv/cv):
 *   VSlam::try_merge_reconstructions (the map)      cv-sfm/src/lib.rs:2116-2193 (2159-2170)
 *   VSlam::incorporate_reconstruction               cv-sfm/src/lib.rs:1817-1887
 *   VSlam::normalize_reconstruction                 cv-sfm/src/lib.rs:2241-2283
 *   WorldToWorld::from_camera_poses                 cv-core/src/pose.rs:322-324
 *
 * Departures:
 *   - order: the reference walks HashMaps and slotmaps.  Here a destination row is its old list, then the kept observations of
 *     the source landmark mapped to it in source order; new keys ascend with the source key;
 *   - a map that is not one-to-one: the reference's HashMap insert would silently overwrite an observation.  Here an entry is
 *     applied iff no other entry names its source landmark and none names its destination landmark (akz_lt_merge_applied);
 *     a demoted source landmark gets its own row;
 *   - destination keys are stable and destination tombstones stay; source tombstones and rows emptied by the drop take no key;
 *   - remove_view after a refused record (lib.rs:1880-1884): the caller runs again from the old tables with d_skip;
 *   - the mean (the `average` crate's Mean, not in the tree: unpinned): a sum in akz_sum_order.h's order, T = 256, divided by
 *     the count;
 *   - the isometry product and inverse (nalgebra, not in the tree: unpinned): akz_tvc_pose_mul and akz_tv_pose_inverse, as
 *     the pose-graph header states them.  The transform is inverse(src_pose) * dest_pose formed directly, where the
 *     reference inverts inverse(dest_pose) * src_pose;
 *   - a finding, shipped as the reference's text: WorldToWorld is an isometry without scale, so two reconstructions of
 *     different scale are joined with the source's translations unscaled.
 */
#ifndef AKZ_RECONSTRUCTION_MERGE_MATH_H
#define AKZ_RECONSTRUCTION_MERGE_MATH_H

#include "akz_landmark_table_math.h"
#include "akz_three_view_constraint_math.h"

/* the verdict on an incorporation (RS_IR_* of include/akz.h) */
enum {
    AKZ_IR_OK = 0,
    AKZ_IR_BAD_TABLE = 1,       /* either table's starts do not ascend inside its n_obs */
    AKZ_IR_BAD_INDEX = 2,       /* a kept source observation names a feature >= cap */
    AKZ_IR_SHARED_BLOCK = 3     /* a kept source observation names a block the destination table names */
};
/* words of d_counts_out */
enum {
    AKZ_IR_C_ROWS = 0, AKZ_IR_C_OBSERVATIONS = 1, AKZ_IR_C_APPLIED = 2, AKZ_IR_C_DEMOTED = 3, AKZ_IR_C_NEW_ROWS = 4, AKZ_IR_C_DROPPED = 5,
    AKZ_IR_COUNTS = 6
};
/* what a block is to a call: bits of its word */
enum { AKZ_IR_BLOCK_KEPT = 1, AKZ_IR_BLOCK_DEST = 2 };
/* the verdict on a normalisation (RS_NR_*) */
enum { AKZ_NR_OK = 0, AKZ_NR_NOT_NORMAL = 1, AKZ_NR_BAD_INDEX = 2 };

/* ---- the map (lib.rs:2159-2170) ---- */
/* Final match {feature, row} of slot f: 1 and the entry {source landmark, destination landmark} when the match names something
 * under akz_lt_match's rules and the feature has a source landmark.  The destination of a merged match is best[0]. */
AKZ_LT_FN int akz_mr_map_entry(uint32_t feature, uint32_t row, uint32_t count, uint32_t f, uint32_t cap, uint32_t n_world, uint32_t n_landmarks,
                               const uint32_t* best, const uint32_t* src_landmarks_of_block, uint32_t* src, uint32_t* dst)
{
    uint32_t b;
    if (akz_lt_match(feature, row, count, f, cap, n_world, n_landmarks, best, dst, &b) == AKZ_LT_MATCH_BAD) return 0;
    *src = src_landmarks_of_block[feature];                  /* feature < count <= cap */
    return *src != AKZ_LT_NONE;
}

/* ---- incorporate (lib.rs:1817-1887) ---- */
/* the verdict of a call from what its validation found */
AKZ_LT_FN uint32_t akz_ir_verdict(int bad_table, int bad_index, int shared)
{
    return bad_table ? AKZ_IR_BAD_TABLE : bad_index ? AKZ_IR_BAD_INDEX : shared ? AKZ_IR_SHARED_BLOCK : AKZ_IR_OK;
}
/* a source observation is kept iff its block is a source view of the call that is not skipped */
AKZ_LT_FN int akz_ir_kept(const uint32_t* block_bits, uint32_t n_blocks, uint32_t block)
{
    return block < n_blocks && (block_bits[block] & (uint32_t)AKZ_IR_BLOCK_KEPT) != 0u;
}
/* what a kept observation {block, feature} does to the call: 0, AKZ_IR_BAD_INDEX or AKZ_IR_SHARED_BLOCK (block < n_blocks) */
AKZ_LT_FN uint32_t akz_ir_kept_fault(const uint32_t* block_bits, uint32_t block, uint32_t feature, uint32_t cap)
{
    if (feature >= cap) return AKZ_IR_BAD_INDEX;
    return (block_bits[block] & (uint32_t)AKZ_IR_BLOCK_DEST) ? (uint32_t)AKZ_IR_SHARED_BLOCK : 0u;
}
/* a map entry names rows of both tables */
AKZ_LT_FN int akz_ir_entry_inside(uint32_t src, uint32_t dst, uint32_t n_src_landmarks, uint32_t n_dst_landmarks)
{
    return src < n_src_landmarks && dst < n_dst_landmarks;
}
/* the batch rule of akz_landmark_table_math.h on the map: refs = how many entries of the map name the landmark */
AKZ_LT_FN int akz_ir_entry_applied(uint32_t src, uint32_t dst, uint32_t n_src_landmarks, uint32_t n_dst_landmarks, const uint32_t* src_refs,
                                   const uint32_t* dst_refs)
{
    return akz_ir_entry_inside(src, dst, n_src_landmarks, n_dst_landmarks) && akz_lt_merge_applied(src_refs[src], dst_refs[dst]);
}
/* an unmapped source landmark with a kept observation becomes a row behind the destination's */
AKZ_LT_FN int akz_ir_new_row(uint32_t mapped_to, uint32_t kept_len) { return mapped_to == AKZ_LT_NONE && kept_len != 0u; }

/* dest_to_src_transform (lib.rs:1824 with pose.rs:322-324): inverse(src_pose) * dest_pose */
AKZ_RM_FN void akz_ir_transform(const double* src_pose, const double* dest_pose, double* t)
{
    double inv[12];
    akz_tv_pose_inverse(src_pose, inv);
    akz_tvc_pose_mul(inv, dest_pose, t);
}

/* ---- normalise (lib.rs:2241-2283) ---- */
/* 1 and the distance of world point p [4] from the camera of `pose` when the point has a Euclidean position: w < 0 is
 * akz_tri_none, w == 0 a point at infinity.  |(pose * p).xyz / w| */
AKZ_RM_FN int akz_nr_distance(const double* pose, const double* p, double* distance)
{
    const double w = p[3];
    if (w < 0.0 || w == 0.0) return 0;
    double c[3];
    AKZ_RM_UNROLL
    for (int i = 0; i < 3; ++i) c[i] = (((pose[i * 4] * p[0] + pose[i * 4 + 1] * p[1]) + pose[i * 4 + 2] * p[2]) + pose[i * 4 + 3] * w) / w;
    *distance = AKZ_RM_SQRT((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
    return 1;
}
/* the mean of n distances; of none, 0 (not a normal number: the reference's 0 / 0 is not one either, and a NaN's sign is not
 * the same on every machine) */
AKZ_RM_FN double akz_nr_mean(double sum, uint32_t n) { return n ? sum / (double)n : 0.0; }
/* f64::is_normal: neither zero, subnormal, infinite nor NaN */
AKZ_RM_FN int akz_nr_is_normal(double x)
{
    const double a = x < 0.0 ? -x : x;
    return a >= 2.2250738585072014e-308 && a <= 1.7976931348623157e308;
}
/* a view's pose: pose * inverse(first), its translation times the factor */
AKZ_RM_FN void akz_nr_view(const double* pose, const double* inv_first, double factor, double* out)
{
    akz_tvc_pose_mul(pose, inv_first, out);
    out[3] = out[3] * factor; out[7] = out[7] * factor; out[11] = out[11] * factor;
}

#if !defined(__HIP_DEVICE_COMPILE__)
/* ---- the host's execution of each whole procedure (the CPU checker's; the kernels' loops one after another) ---- */
#include <stdlib.h>
#include <string.h>
#define AKZ_MR_HOST_FN static inline

/* rs_merge_map_device: map [cap][2], entries [0, *map_count) written, in ascending feature order; a feature in two final
 * matches takes the first. */
AKZ_MR_HOST_FN void akz_mr_merge_map(const uint32_t* matches, const uint32_t* nmatches, const unsigned char* final_mask, const uint32_t* best,
                                     uint32_t n_world, uint32_t n_dst_landmarks, uint32_t cap, uint32_t f, const uint32_t* counts,
                                     const uint32_t* src_landmarks, uint32_t bridge_block, uint32_t* scratch_feat, uint32_t* map,
                                     uint32_t* map_count)
{
    const uint32_t count = counts[bridge_block], nm = nmatches[f];
    uint32_t n = 0;
    *map_count = 0u;
    if (count > cap || nm > cap) return;
    for (uint32_t j = 0; j < cap; ++j) scratch_feat[j] = AKZ_LT_NONE;
    for (uint32_t i = 0; i < nm; ++i) {
        const size_t at = (size_t)f * cap + i;
        uint32_t s, d;
        if (!final_mask[at]) continue;
        if (!akz_mr_map_entry(matches[2 * at], matches[2 * at + 1], count, f, cap, n_world, n_dst_landmarks, best,
                              src_landmarks + (size_t)bridge_block * cap, &s, &d))
            continue;
        if (i < scratch_feat[matches[2 * at]]) scratch_feat[matches[2 * at]] = i;
    }
    for (uint32_t j = 0; j < count; ++j) {
        const uint32_t i = scratch_feat[j];
        uint32_t s = AKZ_LT_NONE, d = AKZ_LT_NONE;
        if (i == AKZ_LT_NONE) continue;
        const size_t at = (size_t)f * cap + i;
        akz_mr_map_entry(matches[2 * at], matches[2 * at + 1], count, f, cap, n_world, n_dst_landmarks, best,
                         src_landmarks + (size_t)bridge_block * cap, &s, &d);
        map[2 * (size_t)n] = s;
        map[2 * (size_t)n + 1] = d;
        ++n;
    }
    *map_count = n;
}

typedef struct akz_ir_out {
    uint32_t* obs_out;
    uint32_t* landmarks_out;
    uint32_t cap, n_blocks;
} akz_ir_out;
AKZ_MR_HOST_FN void akz_ir_put(const akz_ir_out* o, uint32_t at, uint32_t blk, uint32_t feat, uint32_t key)
{
    o->obs_out[2 * (size_t)at] = blk;
    o->obs_out[2 * (size_t)at + 1] = feat;
    if (blk < o->n_blocks && feat < o->cap) {
        uint32_t* w = o->landmarks_out + (size_t)blk * o->cap + feat;
        if (key < *w) *w = key;
    }
}

/* rs_incorporate_reconstruction_device on host arrays (the refusals of the entry point are not restated).  -1: out of memory. */
AKZ_MR_HOST_FN int akz_ir_incorporate(const uint32_t* dst_start, const uint32_t* dst_obs, uint32_t n_dst_obs, uint32_t n_dst, const uint32_t* src_start,
                                      const uint32_t* src_obs, uint32_t n_src_obs, uint32_t n_src, const uint32_t* map, const uint32_t* map_count,
                                      uint32_t map_room, uint32_t cap, uint32_t n_blocks, const uint32_t* src_blocks, uint32_t n_src_views,
                                      uint32_t bridge_block, const double* src_pose, const uint32_t* skip, uint32_t obs_room, uint32_t lm_room,
                                      double* poses, uint32_t* obs_start_out, uint32_t* obs_out, uint32_t* counts_out, uint32_t* landmarks_out,
                                      uint32_t* obs_counts_out, uint32_t* src_key_out, uint32_t* call_verdict)
{
    uint32_t* bits = (uint32_t*)calloc((size_t)n_blocks + 1, sizeof(uint32_t));
    uint32_t* src_refs = (uint32_t*)calloc((size_t)n_src + 1, sizeof(uint32_t));
    uint32_t* dst_refs = (uint32_t*)calloc((size_t)n_dst + 1, sizeof(uint32_t));
    uint32_t* kept_len = (uint32_t*)calloc((size_t)n_src + 1, sizeof(uint32_t));
    uint32_t* map_to = (uint32_t*)malloc(((size_t)n_src + 1) * sizeof(uint32_t));
    uint32_t* map_from = (uint32_t*)malloc(((size_t)n_dst + 1) * sizeof(uint32_t));
    (void)obs_room;
    if (!bits || !src_refs || !dst_refs || !kept_len || !map_to || !map_from) {
        free(bits); free(src_refs); free(dst_refs); free(kept_len); free(map_to); free(map_from);
        return -1;
    }
    memset(map_to, 0xFF, ((size_t)n_src + 1) * sizeof(uint32_t));
    memset(map_from, 0xFF, ((size_t)n_dst + 1) * sizeof(uint32_t));
    memset(landmarks_out, 0xFF, (size_t)n_blocks * cap * sizeof(uint32_t));
    const akz_ir_out out = {obs_out, landmarks_out, cap, n_blocks};
    const uint32_t n_map = *map_count < map_room ? *map_count : map_room;

    /* k_ir_check: the starts of both tables, the blocks of the call, the references of the map */
    int bad_dst = 0, bad_src = 0, bad_index = 0, shared = 0;
    for (uint32_t l = 0; l <= n_dst; ++l) bad_dst |= akz_lt_start_bad(dst_start, l, n_dst, n_dst_obs);
    for (uint32_t l = 0; l <= n_src; ++l) bad_src |= akz_lt_start_bad(src_start, l, n_src, n_src_obs);
    for (uint32_t v = 0; v < n_src_views; ++v)
        if (!(skip && skip[v] != 0u)) bits[src_blocks[v]] |= (uint32_t)AKZ_IR_BLOCK_KEPT;
    for (uint32_t i = 0; i < n_dst_obs && i < dst_start[n_dst]; ++i)
        if (dst_obs[2 * (size_t)i] < n_blocks) bits[dst_obs[2 * (size_t)i]] |= (uint32_t)AKZ_IR_BLOCK_DEST;
    for (uint32_t e = 0; e < n_map; ++e) {
        if (map[2 * (size_t)e] < n_src) ++src_refs[map[2 * (size_t)e]];
        if (map[2 * (size_t)e + 1] < n_dst) ++dst_refs[map[2 * (size_t)e + 1]];
    }
    const int bad_table = bad_dst || bad_src;

    /* k_ir_source_rows: the kept observations of every source row, and what they do to the call */
    uint32_t kept_total = 0;
    if (!bad_table)
        for (uint32_t r = 0; r < n_src; ++r)
            for (uint32_t i = src_start[r]; i < src_start[r + 1]; ++i) {
                const uint32_t blk = src_obs[2 * (size_t)i], feat = src_obs[2 * (size_t)i + 1];
                if (!akz_ir_kept(bits, n_blocks, blk)) continue;
                const uint32_t fault = akz_ir_kept_fault(bits, blk, feat, cap);
                bad_index |= fault == (uint32_t)AKZ_IR_BAD_INDEX;
                shared |= fault == (uint32_t)AKZ_IR_SHARED_BLOCK;
                ++kept_len[r];
                ++kept_total;
            }
    const uint32_t verdict = akz_ir_verdict(bad_table, bad_index, shared);
    const int ok = verdict == (uint32_t)AKZ_IR_OK;

    /* k_ir_apply */
    uint32_t n_applied = 0, n_demoted = 0;
    if (ok)
        for (uint32_t e = 0; e < n_map; ++e) {
            const uint32_t s = map[2 * (size_t)e], d = map[2 * (size_t)e + 1];
            if (akz_ir_entry_applied(s, d, n_src, n_dst, src_refs, dst_refs)) {
                map_to[s] = d;
                map_from[d] = s;
                ++n_applied;
            } else {
                ++n_demoted;
            }
        }

    /* k_ir_tile_sums .. k_ir_dest_rows: the rows of the destination */
    uint32_t total = 0;
    for (uint32_t l = 0; l < n_dst; ++l) {
        const uint32_t m = map_from[l];
        const uint32_t len = bad_dst ? 0u : (dst_start[l + 1] - dst_start[l]) + (m != AKZ_LT_NONE ? kept_len[m] : 0u);
        uint32_t at = total;
        obs_counts_out[l] = len;
        obs_start_out[l] = total;
        total += len;
        if (bad_dst) continue;
        for (uint32_t i = dst_start[l]; i < dst_start[l + 1]; ++i) akz_ir_put(&out, at++, dst_obs[2 * (size_t)i], dst_obs[2 * (size_t)i + 1], l);
        if (m != AKZ_LT_NONE)
            for (uint32_t i = src_start[m]; i < src_start[m + 1]; ++i)
                if (akz_ir_kept(bits, n_blocks, src_obs[2 * (size_t)i])) akz_ir_put(&out, at++, src_obs[2 * (size_t)i], src_obs[2 * (size_t)i + 1], l);
    }

    /* k_ir_source_out: the new rows, the key of every source landmark */
    uint32_t rows = n_dst;
    for (uint32_t r = 0; r < n_src; ++r) {
        if (!ok) {
            src_key_out[r] = AKZ_LT_NONE;
            continue;
        }
        if (!akz_ir_new_row(map_to[r], kept_len[r])) {
            src_key_out[r] = map_to[r];
            continue;
        }
        src_key_out[r] = rows;
        obs_start_out[rows] = total;
        obs_counts_out[rows] = kept_len[r];
        for (uint32_t i = src_start[r]; i < src_start[r + 1]; ++i)
            if (akz_ir_kept(bits, n_blocks, src_obs[2 * (size_t)i])) akz_ir_put(&out, total++, src_obs[2 * (size_t)i], src_obs[2 * (size_t)i + 1], rows);
        ++rows;
    }

    /* k_ir_tail: the empty rows up to the room; k_ir_scan_sums: the counts */
    for (uint32_t r = rows; r <= lm_room; ++r) {
        obs_start_out[r] = total;
        if (r < lm_room) obs_counts_out[r] = 0u;
    }
    counts_out[AKZ_IR_C_ROWS] = rows;
    counts_out[AKZ_IR_C_OBSERVATIONS] = total;
    counts_out[AKZ_IR_C_APPLIED] = n_applied;
    counts_out[AKZ_IR_C_DEMOTED] = n_demoted;
    counts_out[AKZ_IR_C_NEW_ROWS] = rows - n_dst;
    counts_out[AKZ_IR_C_DROPPED] = ok ? src_start[n_src] - kept_total : 0u;
    *call_verdict = verdict;

    /* k_ir_poses */
    if (ok) {
        double t[12], o[12];
        akz_ir_transform(src_pose, poses + (size_t)12 * bridge_block, t);
        for (uint32_t v = 0; v < n_src_views; ++v) {
            if (skip && skip[v] != 0u) continue;
            double* p = poses + (size_t)12 * src_blocks[v];
            akz_tvc_pose_mul(p, t, o);
            for (int k = 0; k < 12; ++k) p[k] = o[k];
        }
    }
    free(bits); free(src_refs); free(dst_refs); free(kept_len); free(map_to); free(map_from);
    return 0;
}

/* rs_normalize_reconstruction_device on host arrays: one workgroup of AKZ_SUM_THREADS */
AKZ_MR_HOST_FN void akz_nr_normalize(const uint32_t* view_blocks, uint32_t n_views, const uint32_t* counts, const uint32_t* landmarks, uint32_t cap,
                                     uint32_t n_blocks, const double* world, uint32_t n_world, double* poses, double* constraint_poses,
                                     uint32_t n_constraints, double* stats, uint32_t* verdict)
{
    int bad = 0;
    for (uint32_t v = 0; v < n_views; ++v) bad |= view_blocks[v] >= n_blocks;
    if (!bad) bad = counts[view_blocks[0]] > cap;
    if (bad) {
        stats[0] = 0.0;
        stats[1] = 0.0;
        *verdict = AKZ_NR_BAD_INDEX;
        return;
    }
    const uint32_t first = view_blocks[0], count = counts[first];
    double part[AKZ_SUM_THREADS], net;
    uint32_t n = 0;
    for (uint32_t t = 0; t < (uint32_t)AKZ_SUM_THREADS; ++t) {
        part[t] = 0.0;
        for (uint32_t j = t; j < count; j += (uint32_t)AKZ_SUM_THREADS) {
            const uint32_t lm = landmarks[(size_t)first * cap + j];
            double d;
            if (lm >= n_world || !akz_nr_distance(poses + (size_t)12 * first, world + 4 * (size_t)lm, &d)) continue;
            part[t] = part[t] + d;
            ++n;
        }
    }
    akz_sum_block(part, 1, &net);
    const double mean = akz_nr_mean(net, n);
    stats[0] = mean;
    stats[1] = (double)n;
    if (!akz_nr_is_normal(mean)) {
        *verdict = AKZ_NR_NOT_NORMAL;
        return;
    }
    *verdict = AKZ_NR_OK;
    const double factor = 1.0 / mean;
    double inv[12], o[12];
    akz_tv_pose_inverse(poses + (size_t)12 * first, inv);
    for (uint32_t v = 0; v < n_views; ++v) {
        double* p = poses + (size_t)12 * view_blocks[v];
        akz_nr_view(p, inv, factor, o);
        for (int k = 0; k < 12; ++k) p[k] = o[k];
    }
    for (size_t c = 0; c < 2 * (size_t)n_constraints; ++c) {
        double* p = constraint_poses + 12 * c;
        p[3] = p[3] * factor; p[7] = p[7] * factor; p[11] = p[11] * factor;
    }
}
#endif /* !__HIP_DEVICE_COMPILE__ */

#endif /* AKZ_RECONSTRUCTION_MERGE_MATH_H */
