/* akz_landmark_table_math.h — the bookkeeping of cv-sfm's landmark table around the registration of a micro-batch of frames:
 * the graph test behind a merge candidate and the next generation of the table.  Integer decisions only, written once for gcc
 * (the CPU checker, tests/cpp/landmark_table_host.c) and hipcc (the gfx950 kernels of cv_amd/csrc/rs_landmark_table.hip):
 * parity is "host build == HIP" in every byte of every output.
 *
 * Reference code restated here (paths relative to rust-cv/cv):
 *   VSlamData::add_view                      cv-sfm/src/lib.rs:432-483
 *   VSlamData::add_landmark                  cv-sfm/src/lib.rs:487-500
 *   VSlamData::merge_landmarks               cv-sfm/src/lib.rs:699-721
 *   VSlam::are_landmarks_sharing_view        cv-sfm/src/lib.rs:1435-1449
 *
 * Departures:
 *   - the reference adds one frame at a time; a call here adds every accepted frame of a micro-batch to ONE input table.  A
 *     merge (a, b) is applied only when no other match of the call names a or b (akz_lt_merge_applied); otherwise it is
 *     demoted: the observation goes to a, b is left alone.  For one frame nothing is ever demoted and the result is add_view's;
 *   - landmark keys are stable: merge_landmarks removes b from a slotmap, here row b stays as an empty list (a tombstone);
 *   - the order of a list: the reference keeps a HashMap per landmark; here a row is its old list, then the old list of the
 *     landmark merged into it, then the new observations in ascending slot order;
 *   - a slot whose matches name the same feature twice is refused (AKZ_AV_BAD_INDEX): every feature of a view observes one
 *     landmark, and the rooms of the output arrays are counted on it.
 */
#ifndef AKZ_LANDMARK_TABLE_MATH_H
#define AKZ_LANDMARK_TABLE_MATH_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define AKZ_LT_FN __host__ __device__ static inline
#else
#define AKZ_LT_FN static inline
#endif

/* the verdict on a slot, and on a call (RS_AV_* of include/akz.h) */
enum {
    AKZ_AV_OK = 0,
    AKZ_AV_NOT_ACCEPTED = 1,   /* the refinement's verdict was not RS_SV_OK, the caller skipped the slot, or the call was refused */
    AKZ_AV_BAD_INDEX = 2,      /* a count above the capacity or a final match that names nothing: the slot contributes nothing */
    AKZ_AV_BAD_TABLE = 3       /* the call's verdict only: the input table's starts do not ascend inside [0, n_obs] */
};
/* stats words (u32) of a slot */
enum {
    AKZ_AV_S_OBSERVATIONS = 0,   /* observations added to rows of the input table (the slot's final matches) */
    AKZ_AV_S_MERGED = 1,         /* merges applied */
    AKZ_AV_S_DEMOTED = 2,        /* merges demoted */
    AKZ_AV_S_NEW_LANDMARKS = 3,  /* rows added behind the table (the slot's features in no final match) */
    AKZ_AV_STATS = 4
};
/* words of d_counts_out */
enum { AKZ_AV_C_ROWS = 0, AKZ_AV_C_OBSERVATIONS = 1, AKZ_AV_C_MERGED = 2, AKZ_AV_C_DEMOTED = 3, AKZ_AV_COUNTS = 4 };
/* what a final match names */
enum { AKZ_LT_MATCH_BAD = 0, AKZ_LT_MATCH_SINGLE = 1, AKZ_LT_MATCH_MERGED = 2 };
enum { AKZ_LT_SV_OK = 0 };       /* RS_SV_OK: the only verdict of the refinement that registers a frame */
#define AKZ_LT_NONE 0xFFFFFFFFu

/* the observations that are the table's: the first min(start[n_landmarks], n_obs) */
AKZ_LT_FN uint32_t akz_lt_fill(const uint32_t* start, uint32_t n_landmarks, uint32_t n_obs)
{
    const uint32_t e = start[n_landmarks];
    return e < n_obs ? e : n_obs;
}

/* start l <= n_landmarks breaks "the starts ascend inside [0, n_obs]" */
AKZ_LT_FN int akz_lt_start_bad(const uint32_t* start, uint32_t l, uint32_t n_landmarks, uint32_t n_obs)
{
    return l < n_landmarks ? start[l] > start[l + 1] : start[l] > n_obs;
}

/* The list of landmark l: 1 and [*s, *e) when l is a row of the table and its range lies inside the filled observations. */
AKZ_LT_FN int akz_lt_range(const uint32_t* start, uint32_t l, uint32_t n_landmarks, uint32_t fill, uint32_t* s, uint32_t* e)
{
    if (l >= n_landmarks) return 0;
    *s = start[l];
    *e = start[l + 1];
    return *s <= *e && *e <= fill;
}

/* A feature's merge candidate for the graph test: 1 and the two ranges when its decision is 2 and both landmarks have a list
 * inside the table; 0: the byte of the mask is 0.  best6 = the feature's {landmark, distance} x 3 of hm_best_of_views. */
AKZ_LT_FN int akz_lt_candidate(const uint32_t* start, uint32_t n_landmarks, uint32_t fill, uint32_t decision, const uint32_t* best6,
                               uint32_t* sa, uint32_t* ea, uint32_t* sb, uint32_t* eb)
{
    if (decision != 2u) return 0;
    return akz_lt_range(start, best6[0], n_landmarks, fill, sa, ea) && akz_lt_range(start, best6[2], n_landmarks, fill, sb, eb);
}

/* are_landmarks_sharing_view on two lists of {block, feature}: some block of [sb, eb) is a block of [sa, ea) */
AKZ_LT_FN int akz_lt_lists_share(const uint32_t* obs, uint32_t sa, uint32_t ea, uint32_t sb, uint32_t eb)
{
    for (uint32_t j = sb; j < eb; ++j) {
        const uint32_t blk = obs[2 * (size_t)j];
        for (uint32_t i = sa; i < ea; ++i)
            if (obs[2 * (size_t)i] == blk) return 1;
    }
    return 0;
}

/* What final match {feature, row} of slot f names: a landmark (*a), a merge (*a, *b) or nothing.  count = the features of the
 * slot's frame; best = d_best of the call or null. */
AKZ_LT_FN int akz_lt_match(uint32_t feature, uint32_t row, uint32_t count, uint32_t f, uint32_t cap, uint32_t n_world, uint32_t n_landmarks,
                           const uint32_t* best, uint32_t* a, uint32_t* b)
{
    *a = AKZ_LT_NONE;
    *b = AKZ_LT_NONE;
    if (feature >= count) return AKZ_LT_MATCH_BAD;
    if (row < n_world) {
        *a = row;
        return row < n_landmarks ? AKZ_LT_MATCH_SINGLE : AKZ_LT_MATCH_BAD;
    }
    if (!best || (uint64_t)row != (uint64_t)n_world + (uint64_t)f * cap + feature) return AKZ_LT_MATCH_BAD;
    const uint32_t* b6 = best + 6 * ((size_t)f * cap + feature);
    *a = b6[0];
    *b = b6[2];
    return (*a != *b && *a < n_landmarks && *b < n_landmarks) ? AKZ_LT_MATCH_MERGED : AKZ_LT_MATCH_BAD;
}

/* The batch rule: a merge is applied iff nothing else in the call names either landmark. */
AKZ_LT_FN int akz_lt_merge_applied(uint32_t refs_a, uint32_t refs_b) { return refs_a == 1u && refs_b == 1u; }

/* The length of output row l of the input table: nothing for a tombstone, else its old list, the list merged into it and the
 * observations the call adds. */
AKZ_LT_FN uint32_t akz_lt_row_length(uint32_t old_len, uint32_t merged_len, uint32_t adds, int tombstone)
{
    return tombstone ? 0u : old_len + merged_len + adds;
}

/* Start r of the rows behind the input table (n_landmarks <= r <= lm_room): they hold one observation each up to rows_filled
 * and nothing beyond.  total_old = the observations of the rows below n_landmarks. */
AKZ_LT_FN uint32_t akz_lt_tail_start(uint32_t total_old, uint32_t rows_filled, uint32_t n_landmarks, uint32_t r)
{
    return total_old + ((r < rows_filled ? r : rows_filled) - n_landmarks);
}

/* The order of the observations a call adds to one row: ascending slot (and feature, for a caller that broke "a frame names a
 * landmark once") */
AKZ_LT_FN int akz_lt_tail_less(uint32_t slot_a, uint32_t feat_a, uint32_t slot_b, uint32_t feat_b)
{
    return slot_a < slot_b || (slot_a == slot_b && feat_a < feat_b);
}

#endif /* AKZ_LANDMARK_TABLE_MATH_H */
