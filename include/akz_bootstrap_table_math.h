/* akz_bootstrap_table_math.h — the two integer steps around cv-sfm's three-view bootstrap that create a reconstruction: the join
 * (and shuffle) of two consensuses' inlier lists in front of it and add_reconstruction behind it — the first generation of the
 * landmark table.  Integer decisions only, written once for gcc (the CPU checker, tests/cpp/bootstrap_table_host.c) and hipcc
 * (the gfx950 kernels of cv_amd/csrc/rs_bootstrap_table.hip): parity is "host build == HIP" in every byte of every output.
 *
 * Reference code restated here (paths relative to rust-cv/cv):
 *   VSlam::init_reconstruction, the join and the shuffle   cv-sfm/src/lib.rs:992-999, 1190-1191, 1216, 1234
 *   the two-view inlier minimum                            cv-sfm/src/lib.rs:1421
 *   VSlamData::add_reconstruction                          cv-sfm/src/lib.rs:377-427
 *   VSlamData::add_view / add_landmark                     cv-sfm/src/lib.rs:432-500
 *
 * Departures:
 *   - the shuffle of the common matches uses the caller's RNG in the reference; here it is RS_BATCH_SHUFFLE's rule: position j
 *     holds the triple with the j-th smallest key akz_bt_shuffle_key(scene seed, j), ties in index order;
 *   - a reconstruction's views are a contiguous block range {centre, first, second}: the reference's insertion order, in which
 *     canonical_view_order is the identity;
 *   - the reference tries one combination of frames after another and takes the first that passes; a call here walks its scenes
 *     in order and refuses a scene that names a source frame of an earlier accepted scene (AKZ_AR_TAKEN);
 *   - a scene in which a feature of one view occurs in two accepted matches is refused alone (AKZ_AR_BAD_INDEX): the reference's
 *     HashMaps would silently overwrite, and symmetric matching never produces it;
 *   - the order of a landmark's list: {centre}, then {first}, then {second}; the rows: one per centre feature in feature order,
 *     then the first frame's features in no accepted match, ascending, then the second frame's.
 */
#ifndef AKZ_BOOTSTRAP_TABLE_MATH_H
#define AKZ_BOOTSTRAP_TABLE_MATH_H

#include <stdint.h>

#include "akz_landmark_table_math.h"

/* the verdict on a scene of the join (RS_JP_* of include/akz.h) */
enum {
    AKZ_JP_OK = 0,
    AKZ_JP_NO_MODEL = 1,      /* a consensus of the scene ended without a model */
    AKZ_JP_FEW_INLIERS = 2,   /* an inlier list shorter than two_view_minimum_robust_matches (lib.rs:1421) */
    AKZ_JP_BAD_INDEX = 3      /* a count above the capacity, an inlier index outside its pair list, a feature outside its block */
};
/* the verdict on a scene of add_reconstruction, and on a call (RS_AR_*) */
enum {
    AKZ_AR_OK = 0,
    AKZ_AR_NOT_ACCEPTED = 1,  /* the bootstrap's verdict was not RS_TV_OK, the caller skipped the scene, or the call was refused */
    AKZ_AR_BAD_INDEX = 2,     /* a count above the capacity, a match that names nothing, a feature in two accepted matches */
    AKZ_AR_TAKEN = 3,         /* an earlier accepted scene of the call names one of the scene's frames */
    AKZ_AR_BAD_TABLE = 4      /* the call's verdict only: the existing table's starts do not ascend or do not end where they must */
};
/* stats words (u32) of a scene */
enum { AKZ_AR_S_TRIPLES = 0, AKZ_AR_S_FIRST = 1, AKZ_AR_S_SECOND = 2, AKZ_AR_S_LANDMARKS = 3, AKZ_AR_STATS = 4 };
/* words of d_counts_out */
enum { AKZ_AR_C_ROWS = 0, AKZ_AR_C_OBSERVATIONS = 1, AKZ_AR_C_RECONSTRUCTIONS = 2, AKZ_AR_C_ACCEPTED = 3, AKZ_AR_COUNTS = 4 };
enum { AKZ_BT_TV_OK = 0, AKZ_BT_TVC_OK = 0, AKZ_BT_NOT_RECORDED = 16 };   /* RS_TV_OK, RS_TVC_OK, RS_CV_NOT_RECORDED */

/* ---- the shuffle: RS_BATCH_SHUFFLE's rule (include/akz.h) ---- */
AKZ_LT_FN uint64_t akz_bt_splitmix64(uint64_t x)
{
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
AKZ_LT_FN uint64_t akz_bt_scene_seed(uint64_t seed, uint32_t s) { return seed + 0x9E3779B97F4A7C15ull * (uint64_t)s; }
AKZ_LT_FN uint32_t akz_bt_shuffle_key(uint64_t scene_seed, uint32_t j)
{
    return (uint32_t)(akz_bt_splitmix64((scene_seed ^ 0x5851F42D4C957F2Dull) + 0xD1342543DE82EF95ull * (uint64_t)j) >> 32);
}

/* ---- the join ---- */
/* What the counts and the consensuses' ids say about a scene before any pair is read: OK means n_first, n_second <= cap. */
AKZ_LT_FN uint32_t akz_jp_counts_verdict(uint32_t best_first, uint32_t best_second, uint32_t n_first, uint32_t n_second, uint32_t npairs_first,
                                         uint32_t npairs_second, uint32_t cap, uint32_t minimum)
{
    if (best_first == AKZ_LT_NONE || best_second == AKZ_LT_NONE) return AKZ_JP_NO_MODEL;
    if (n_first > cap || n_second > cap || npairs_first > cap || npairs_second > cap) return AKZ_JP_BAD_INDEX;
    if (n_first < minimum || n_second < minimum) return AKZ_JP_FEW_INLIERS;
    return AKZ_JP_OK;
}
/* Inlier i of a slot (pairs [cap][2], inliers [cap], npairs <= cap): 1 and {centre, other} when it names a pair of the list whose
 * features lie below cap; 0: the scene is AKZ_JP_BAD_INDEX.  Nothing is read out of bounds. */
AKZ_LT_FN int akz_jp_pair(const uint32_t* pairs, const uint32_t* inliers, uint32_t i, uint32_t npairs, uint32_t cap, uint32_t* centre,
                          uint32_t* other)
{
    const uint32_t k = inliers[i];
    if (k >= npairs) return 0;
    *centre = pairs[2 * (size_t)k];
    *other = pairs[2 * (size_t)k + 1];
    return *centre < cap && *other < cap;
}
/* A map centre feature -> position + 1 of its LAST entry in a list (0: none): the larger position wins. */
AKZ_LT_FN uint32_t akz_jp_map_word(uint32_t i) { return i + 1u; }

/* ---- add_reconstruction ---- */
/* The counts of a scene: its three frames are distinct and none of the six counts is above cap. */
AKZ_LT_FN int akz_ar_counts_ok(uint32_t ic, uint32_t i_first, uint32_t i_second, uint32_t count_c, uint32_t count_f, uint32_t count_s,
                               uint32_t ntriples, uint32_t nfirst, uint32_t nsecond, uint32_t cap)
{
    if (ic == i_first || ic == i_second || i_first == i_second) return 0;
    return count_c <= cap && count_f <= cap && count_s <= cap && ntriples <= cap && nfirst <= cap && nsecond <= cap;
}
/* The length of the row of a centre feature: its own observation and one per frame with an accepted match on it. */
AKZ_LT_FN uint32_t akz_ar_row_length(uint32_t first_feature, uint32_t second_feature)
{
    return 1u + (first_feature != AKZ_LT_NONE ? 1u : 0u) + (second_feature != AKZ_LT_NONE ? 1u : 0u);
}
/* The rows and the observations of an accepted scene: matched_f / matched_s = accepted matches that name a feature of the first /
 * second frame (distinct features: the scene is valid). */
AKZ_LT_FN uint32_t akz_ar_scene_rows(uint32_t count_c, uint32_t count_f, uint32_t count_s, uint32_t matched_f, uint32_t matched_s)
{
    return count_c + (count_f - matched_f) + (count_s - matched_s);
}
AKZ_LT_FN uint32_t akz_ar_centre_observations(uint32_t count_c, uint32_t matched_f, uint32_t matched_s) { return count_c + matched_f + matched_s; }
/* view k (0 centre, 1 first, 2 second) of scene s */
AKZ_LT_FN uint32_t akz_ar_view(uint32_t view_base, uint32_t s, uint32_t k) { return view_base + 3u * s + k; }
/* start l <= n of an ascending range table over [0, limit] is bad */
AKZ_LT_FN int akz_ar_range_bad(const uint32_t* start, uint32_t l, uint32_t n, uint32_t limit)
{
    return l < n ? start[l] > start[l + 1] : start[l] != limit;
}
/* a row length of the existing table, whatever its starts are */
AKZ_LT_FN uint32_t akz_ar_old_length(const uint32_t* start, uint32_t l) { return start[l + 1] >= start[l] ? start[l + 1] - start[l] : 0u; }

#if !defined(__HIP_DEVICE_COMPILE__)
/* ---- the host's execution of the two procedures (the CPU checker's; the kernels' loops one after another) ---- */
#include <stdlib.h>
#include <string.h>
#define AKZ_BT_HOST_FN static inline

/* the stable ascending order of n 32-bit keys: order[j] = the index of the j-th smallest, ties in index order */
AKZ_BT_HOST_FN void akz_bt_stable_order(const uint32_t* key, uint32_t n, uint32_t* order)
{
    for (uint32_t j = 0; j < n; ++j) order[j] = j;
    uint32_t* tmp = (uint32_t*)malloc(sizeof(uint32_t) * (n ? n : 1u));
    for (int pass = 0; pass < 4; ++pass) {
        uint32_t at[257];
        memset(at, 0, sizeof at);
        for (uint32_t j = 0; j < n; ++j) ++at[((key[order[j]] >> (8 * pass)) & 255u) + 1u];
        for (int d = 0; d < 256; ++d) at[d + 1] += at[d];
        for (uint32_t j = 0; j < n; ++j) tmp[at[(key[order[j]] >> (8 * pass)) & 255u]++] = order[j];
        memcpy(order, tmp, sizeof(uint32_t) * n);
    }
    free(tmp);
}

/* rs_join_pairs_batch_device on host arrays (the refusals of the entry point are not restated); what the device call does not
 * write is not written here either. */
AKZ_BT_HOST_FN void akz_jp_join(const uint32_t* pairs, const uint32_t* npairs, const uint32_t* inliers, const uint32_t* n_inliers,
                                const uint32_t* best_id, const double* pose, uint32_t cap, const uint32_t* slot_first,
                                const uint32_t* slot_second, uint32_t n_scenes, uint32_t minimum, int shuffle, uint64_t seed, uint32_t* triples,
                                uint32_t* ntriples, uint32_t* first_only, uint32_t* nfirst, uint32_t* second_only, uint32_t* nsecond,
                                double* pose_first, double* pose_second, uint32_t* verdict)
{
    uint32_t* map = (uint32_t*)malloc(sizeof(uint32_t) * 7 * (size_t)cap);
    uint32_t *map_f = map, *map_s = map + cap, *key = map + 2 * (size_t)cap, *order = key + cap, *plain = order + cap;   /* plain: [cap][3] */
    for (uint32_t s = 0; s < n_scenes; ++s) {
        const uint32_t a = slot_first[s], b = slot_second[s];
        const uint32_t *pa = pairs + 2 * (size_t)a * cap, *pb = pairs + 2 * (size_t)b * cap;
        const uint32_t *ia = inliers + (size_t)a * cap, *ib = inliers + (size_t)b * cap;
        for (int k = 0; k < 12; ++k) {
            pose_first[12 * (size_t)s + k] = pose[12 * (size_t)a + k];
            pose_second[12 * (size_t)s + k] = pose[12 * (size_t)b + k];
        }
        const uint32_t n1 = n_inliers[a], n2 = n_inliers[b];
        uint32_t v = akz_jp_counts_verdict(best_id[a], best_id[b], n1, n2, npairs[a], npairs[b], cap, minimum), c = 0u, o = 0u;
        if (v == AKZ_JP_OK) {
            for (uint32_t i = 0; i < n1; ++i) v = akz_jp_pair(pa, ia, i, npairs[a], cap, &c, &o) ? v : AKZ_JP_BAD_INDEX;
            for (uint32_t i = 0; i < n2; ++i) v = akz_jp_pair(pb, ib, i, npairs[b], cap, &c, &o) ? v : AKZ_JP_BAD_INDEX;
        }
        verdict[s] = v;
        ntriples[s] = nfirst[s] = nsecond[s] = 0u;
        if (v != AKZ_JP_OK) continue;
        memset(map, 0, sizeof(uint32_t) * 2 * (size_t)cap);
        for (uint32_t i = 0; i < n1; ++i) {
            akz_jp_pair(pa, ia, i, npairs[a], cap, &c, &o);
            if (akz_jp_map_word(i) > map_f[c]) map_f[c] = akz_jp_map_word(i);
        }
        for (uint32_t i = 0; i < n2; ++i) {
            akz_jp_pair(pb, ib, i, npairs[b], cap, &c, &o);
            if (akz_jp_map_word(i) > map_s[c]) map_s[c] = akz_jp_map_word(i);
        }
        uint32_t nt = 0, nf = 0, ns = 0;
        uint32_t *t = triples + 3 * (size_t)s * cap, *f = first_only + 2 * (size_t)s * cap, *g = second_only + 2 * (size_t)s * cap;
        for (uint32_t i = 0; i < n1; ++i) {
            akz_jp_pair(pa, ia, i, npairs[a], cap, &c, &o);
            if (map_s[c]) {
                uint32_t c2 = 0u, o2 = 0u;
                akz_jp_pair(pb, ib, map_s[c] - 1u, npairs[b], cap, &c2, &o2);
                plain[3 * nt] = c; plain[3 * nt + 1] = o; plain[3 * nt + 2] = o2;
                ++nt;
            } else {
                f[2 * nf] = c; f[2 * nf + 1] = o;
                ++nf;
            }
        }
        for (uint32_t i = 0; i < n2; ++i) {
            akz_jp_pair(pb, ib, i, npairs[b], cap, &c, &o);
            if (map_f[c]) continue;
            g[2 * ns] = c; g[2 * ns + 1] = o;
            ++ns;
        }
        if (shuffle) {
            const uint64_t ss = akz_bt_scene_seed(seed, s);
            for (uint32_t j = 0; j < nt; ++j) key[j] = akz_bt_shuffle_key(ss, j);
            akz_bt_stable_order(key, nt, order);
        }
        for (uint32_t j = 0; j < nt; ++j)
            for (int k = 0; k < 3; ++k) t[3 * j + k] = plain[3 * (shuffle ? order[j] : j) + k];
        ntriples[s] = nt; nfirst[s] = nf; nsecond[s] = ns;
    }
    free(map);
}

AKZ_BT_HOST_FN void akz_ar_put(uint32_t* obs_out, uint32_t* landmarks_out, uint32_t n_blocks, uint32_t cap, uint32_t at, uint32_t blk, uint32_t feat,
                               uint32_t key)
{
    obs_out[2 * (size_t)at] = blk;
    obs_out[2 * (size_t)at + 1] = feat;
    if (blk < n_blocks && feat < cap && key < landmarks_out[(size_t)blk * cap + feat]) landmarks_out[(size_t)blk * cap + feat] = key;
}

/* rs_add_reconstruction_batch_device on host arrays (the refusals of the entry point are not restated).  kps / kps_dst are
 * blocks of cap keypoints of kp_bytes bytes each; what the device call does not write is not written here either. */
AKZ_BT_HOST_FN void akz_ar_add(const uint32_t* triples, const uint32_t* ntriples, const uint32_t* first_only, const uint32_t* nfirst,
                               const uint32_t* second_only, const uint32_t* nsecond, const unsigned char* combined, const unsigned char* first_ok,
                               const unsigned char* second_ok, const double* pose_out, const uint32_t* tv_verdict, const uint32_t* ic,
                               const uint32_t* i_first, const uint32_t* i_second, uint32_t n_scenes, const unsigned char* kps, const uint32_t* counts,
                               uint32_t n_src_blocks, uint32_t cap, uint32_t kp_bytes, const uint32_t* skip, const uint32_t* obs_start,
                               const uint32_t* obs, uint32_t n_obs, uint32_t n_landmarks, const uint32_t* recon_start, const uint32_t* view_start,
                               uint32_t n_recons, unsigned char* kps_dst, uint32_t* counts_dst, double* poses, uint32_t n_blocks, uint32_t view_base,
                               uint32_t obs_room, uint32_t lm_room, uint32_t* obs_start_out, uint32_t* obs_out, uint32_t* obs_counts_out,
                               uint32_t* counts_out, uint32_t* landmarks_out, uint32_t* recon_start_out, uint32_t* view_start_out, uint32_t* views_out,
                               double* constraint_poses_out, uint32_t* constraint_verdict_out, uint32_t* frame_verdict, uint32_t* stats,
                               uint32_t* call_verdict)
{
    (void)obs_room;
    const uint32_t no_table = 0u;
    if (!obs_start) obs_start = &no_table;                               /* no table: one start, 0 */
    /* k_bt_check_table */
    int bad = 0;
    for (uint32_t l = 0; l <= n_landmarks; ++l) bad |= akz_lt_start_bad(obs_start, l, n_landmarks, n_obs);
    if (n_recons)
        for (uint32_t r = 0; r <= n_recons; ++r)
            bad |= akz_ar_range_bad(recon_start, r, n_recons, n_landmarks) | akz_ar_range_bad(view_start, r, n_recons, view_base);
    /* the old table */
    memset(landmarks_out, 0xFF, sizeof(uint32_t) * (size_t)n_blocks * cap);
    const uint32_t fill = bad ? n_obs : obs_start[n_landmarks];
    for (uint32_t l = 0; l < n_landmarks; ++l) {
        obs_start_out[l] = obs_start[l];
        obs_counts_out[l] = akz_ar_old_length(obs_start, l);
    }
    for (uint32_t i = 0; i < fill; ++i) {
        obs_out[2 * (size_t)i] = obs[2 * (size_t)i];
        obs_out[2 * (size_t)i + 1] = obs[2 * (size_t)i + 1];
    }
    if (!bad)
        for (uint32_t l = 0; l < n_landmarks; ++l)
            for (uint32_t i = obs_start[l]; i < obs_start[l + 1]; ++i)
                akz_ar_put(obs_out, landmarks_out, n_blocks, cap, i, obs[2 * (size_t)i], obs[2 * (size_t)i + 1], l);
    for (uint32_t r = 0; r < n_recons; ++r) {
        recon_start_out[r] = recon_start[r];
        view_start_out[r] = view_start[r];
    }
    /* k_bt_validate, then k_bt_accept's walk */
    unsigned char* taken = (unsigned char*)calloc(n_src_blocks ? n_src_blocks : 1u, 1);
    uint32_t* map = (uint32_t*)malloc(sizeof(uint32_t) * 5 * (size_t)cap);
    uint32_t *cen = map, *cen_f = map + cap, *cen_s = map + 2 * (size_t)cap, *fst = map + 3 * (size_t)cap, *snd = map + 4 * (size_t)cap;
    uint32_t row = n_landmarks, at = obs_start[n_landmarks], accepted_n = 0;
    const uint32_t old_end_recon = n_recons ? recon_start[n_recons] : n_landmarks, old_end_view = n_recons ? view_start[n_recons] : view_base;
    for (uint32_t s = 0; s < n_scenes; ++s) {
        const uint32_t bc = ic[s], bf = i_first[s], bs = i_second[s];      /* below n_src_blocks: the entry point */
        uint32_t v = AKZ_AR_OK, mt = 0, mf = 0, ms = 0;
        const uint32_t cc = counts[bc], cf = counts[bf], cs = counts[bs];
        if (bad || tv_verdict[s] != (uint32_t)AKZ_BT_TV_OK || (skip && skip[s] != 0u)) v = AKZ_AR_NOT_ACCEPTED;
        else if (!akz_ar_counts_ok(bc, bf, bs, cc, cf, cs, ntriples[s], nfirst[s], nsecond[s], cap)) v = AKZ_AR_BAD_INDEX;
        if (v == AKZ_AR_OK) {
            memset(map, 0xFF, sizeof(uint32_t) * 5 * (size_t)cap);
            const uint32_t *t = triples + 3 * (size_t)s * cap, *f = first_only + 2 * (size_t)s * cap, *g = second_only + 2 * (size_t)s * cap;
            for (uint32_t i = 0; i < ntriples[s]; ++i) {
                if (!combined[(size_t)s * cap + i]) continue;
                const uint32_t c = t[3 * i], x = t[3 * i + 1], y = t[3 * i + 2];
                if (c >= cc || x >= cf || y >= cs || cen[c] != AKZ_LT_NONE || fst[x] != AKZ_LT_NONE || snd[y] != AKZ_LT_NONE) { v = AKZ_AR_BAD_INDEX; break; }
                cen[c] = 0u; cen_f[c] = x; cen_s[c] = y; fst[x] = c; snd[y] = c;
                ++mt;
            }
            for (uint32_t i = 0; v == AKZ_AR_OK && i < nfirst[s]; ++i) {
                if (!first_ok[(size_t)s * cap + i]) continue;
                const uint32_t c = f[2 * i], x = f[2 * i + 1];
                if (c >= cc || x >= cf || cen[c] != AKZ_LT_NONE || fst[x] != AKZ_LT_NONE) { v = AKZ_AR_BAD_INDEX; break; }
                cen[c] = 0u; cen_f[c] = x; fst[x] = c;
                ++mf;
            }
            for (uint32_t i = 0; v == AKZ_AR_OK && i < nsecond[s]; ++i) {
                if (!second_ok[(size_t)s * cap + i]) continue;
                const uint32_t c = g[2 * i], y = g[2 * i + 1];
                if (c >= cc || y >= cs || cen[c] != AKZ_LT_NONE || snd[y] != AKZ_LT_NONE) { v = AKZ_AR_BAD_INDEX; break; }
                cen[c] = 0u; cen_s[c] = y; snd[y] = c;
                ++ms;
            }
        }
        if (v == AKZ_AR_OK && (taken[bc] || taken[bf] || taken[bs])) v = AKZ_AR_TAKEN;
        frame_verdict[s] = v;
        uint32_t* st = stats + (size_t)AKZ_AR_STATS * s;
        st[AKZ_AR_S_TRIPLES] = st[AKZ_AR_S_FIRST] = st[AKZ_AR_S_SECOND] = st[AKZ_AR_S_LANDMARKS] = 0u;
        recon_start_out[n_recons + s] = bad ? old_end_recon : row;
        view_start_out[n_recons + s] = bad ? old_end_view : akz_ar_view(view_base, s, 0);
        for (uint32_t k = 0; k < 3; ++k) views_out[3 * (size_t)s + k] = akz_ar_view(view_base, s, k);
        constraint_verdict_out[s] = v == AKZ_AR_OK ? (uint32_t)AKZ_BT_TVC_OK : (uint32_t)AKZ_BT_NOT_RECORDED;
        if (v != AKZ_AR_OK) continue;
        taken[bc] = taken[bf] = taken[bs] = 1;
        ++accepted_n;
        const uint32_t src[3] = {bc, bf, bs}, cnt[3] = {cc, cf, cs};
        for (uint32_t k = 0; k < 3; ++k) {
            const uint32_t view = akz_ar_view(view_base, s, k);
            memmove(kps_dst + (size_t)view * cap * kp_bytes, kps + (size_t)src[k] * cap * kp_bytes, (size_t)cap * kp_bytes);
            counts_dst[view] = cnt[k];
            for (int e = 0; e < 12; ++e)
                poses[12 * (size_t)view + e] = k == 0 ? ((e == 0 || e == 5 || e == 10) ? 1.0 : 0.0) : pose_out[24 * (size_t)s + 12 * (k - 1u) + e];
        }
        for (int e = 0; e < 24; ++e) constraint_poses_out[24 * (size_t)s + e] = pose_out[24 * (size_t)s + e];
        st[AKZ_AR_S_TRIPLES] = mt; st[AKZ_AR_S_FIRST] = mf; st[AKZ_AR_S_SECOND] = ms;
        st[AKZ_AR_S_LANDMARKS] = akz_ar_scene_rows(cc, cf, cs, mt + mf, mt + ms);
        /* k_bt_rows, k_bt_new_rows */
        for (uint32_t j = 0; j < cc; ++j, ++row) {
            obs_start_out[row] = at;
            obs_counts_out[row] = akz_ar_row_length(cen_f[j], cen_s[j]);
            akz_ar_put(obs_out, landmarks_out, n_blocks, cap, at++, akz_ar_view(view_base, s, 0), j, row);
            if (cen_f[j] != AKZ_LT_NONE) akz_ar_put(obs_out, landmarks_out, n_blocks, cap, at++, akz_ar_view(view_base, s, 1), cen_f[j], row);
            if (cen_s[j] != AKZ_LT_NONE) akz_ar_put(obs_out, landmarks_out, n_blocks, cap, at++, akz_ar_view(view_base, s, 2), cen_s[j], row);
        }
        for (uint32_t k = 1; k < 3; ++k)
            for (uint32_t j = 0; j < cnt[k]; ++j) {
                if ((k == 1 ? fst : snd)[j] != AKZ_LT_NONE) continue;
                obs_start_out[row] = at;
                obs_counts_out[row] = 1u;
                akz_ar_put(obs_out, landmarks_out, n_blocks, cap, at++, akz_ar_view(view_base, s, k), j, row);
                ++row;
            }
    }
    /* k_bt_tail: every start behind the total equals the total */
    const uint32_t rows = bad ? n_landmarks : row, total = bad ? obs_start[n_landmarks] : at;
    for (uint32_t r = rows; r <= lm_room; ++r) {
        obs_start_out[r] = total;
        if (r < lm_room) obs_counts_out[r] = 0u;
    }
    recon_start_out[n_recons + n_scenes] = bad ? old_end_recon : rows;
    view_start_out[n_recons + n_scenes] = bad ? old_end_view : akz_ar_view(view_base, n_scenes, 0);
    counts_out[AKZ_AR_C_ROWS] = rows;
    counts_out[AKZ_AR_C_OBSERVATIONS] = bad ? n_obs : total;
    counts_out[AKZ_AR_C_RECONSTRUCTIONS] = n_recons + n_scenes;
    counts_out[AKZ_AR_C_ACCEPTED] = accepted_n;
    *call_verdict = bad ? AKZ_AR_BAD_TABLE : AKZ_AR_OK;
    free(map);
    free(taken);
}
#endif /* !__HIP_DEVICE_COMPILE__ */

#endif /* AKZ_BOOTSTRAP_TABLE_MATH_H */
