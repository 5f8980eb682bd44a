/* akz_observation_filter_math.h — cv-sfm's filter of the observations of a reconstruction behind a relaxation of its pose
 * graph (VSlam::filter_non_robust_observations), written as plain IEEE double arithmetic so that gcc (the CPU checker,
 * tests/cpp/observation_filter_host.c) and hipcc (the gfx950 kernels of cv_amd/csrc/rs_observation_filter.hip) execute the
 * same operation sequence (build: -ffp-contract=off, no fast-math; sqrt is the one non-arithmetic primitive).  Parity is
 * "host build == HIP", bit for bit.  Built on akz_triangulate_math.h (the triangulator with and without its robustness
 * test, the pair test, the world bearing), akz_three_view_math.h (akz_tv_loss, akz_tv_bi_landmark_robust,
 * akz_tv_transformed_distance, akz_tv_pose_inverse) and akz_three_view_constraint_math.h (akz_tvc_pose_mul, the product of two
 * isometries): this header adds the decisions around them and no second copy of any of them.
 *
 * Reference code restated here (paths relative to rust-cv/cv):
 *   VSlam::filter_non_robust_observations               cv-sfm/src/lib.rs:2657-2757
 *   VSlam::split_landmark                               cv-sfm/src/lib.rs:2559-2568
 *   VSlamData::split_observation                        cv-sfm/src/lib.rs:552-588
 *   VSlam::triangulate_landmark                         cv-sfm/src/lib.rs:2874-2892
 *   VSlam::are_observations_robust, is_landmark_robust  cv-sfm/src/lib.rs:2907-2934, 2975-2987
 *   VSlam::is_bi_landmark_robust                        cv-sfm/src/lib.rs:1306-1317
 *
 * Unpinned against the reference:
 *   - everything the three headers above list as unpinned (the eigen-solver, the product orders, the product of two
 *     isometries);
 *   - the order of a landmark's observations: the reference walks a HashMap; here it is the order of the caller's list.  The
 *     order decides which observation split_landmark leaves in the landmark (the first) and which one stays when all fail
 *     (the last);
 *   - a landmark without observations: the reference calls it unreachable (lib.rs:2686); here it is a state, nothing happens.
 *
 * What a landmark's filter does NOT depend on is the other landmarks: split_observation moves an observation into a NEW
 * landmark of one observation, which the loop of lib.rs:2679 never visits (its list was collected before) and which can never
 * be robust (the pair test needs two).  So the robust count after the filter is a count over the original rows, and one
 * landmark is one independent problem.
 */
#ifndef AKZ_OBSERVATION_FILTER_MATH_H
#define AKZ_OBSERVATION_FILTER_MATH_H

#include "akz_three_view_constraint_math.h"

/* what became of a landmark (RS_OF_* of include/akz.h) */
enum {
    AKZ_OF_KEPT = 0,        /* two or more observations, all of them stayed */
    AKZ_OF_SINGLE = 1,      /* one observation or none: nothing happens (lib.rs:2686-2687) */
    AKZ_OF_PAIR_SPLIT = 2,  /* two observations that failed is_bi_landmark_robust: the second was split off (lib.rs:2703-2711) */
    AKZ_OF_NO_POINT = 3,    /* three or more and triangulate_landmark gave None: all but the first were split off (lib.rs:2728-2732) */
    AKZ_OF_KICKED = 4,      /* three or more, a point, and at least one observation disagreed with it (lib.rs:2721-2726) */
    AKZ_OF_BAD_INDEX = 5,   /* an observation names a block or a feature outside the caller's arrays: left as it is, not robust */
    AKZ_OF_SKIPPED = 6      /* the landmark belongs to no reconstruction that ran: left as it is, nothing computed */
};
/* the verdict on a reconstruction */
enum {
    AKZ_OF_OK = 0,
    AKZ_OF_FEW_LANDMARKS = 1,   /* fewer than minimum_robust_landmarks robust after the filter (lib.rs:2747-2753) */
    AKZ_OF_BAD_RANGE = 2,       /* its ranges in the start arrays are not ascending inside the arrays' bounds */
    AKZ_OF_RECON_SKIPPED = 3    /* the caller asked to pass it through */
};
/* stats words (u32) of a reconstruction */
enum {
    AKZ_OF_S_LANDMARKS = 0,      /* rows of the table it owns */
    AKZ_OF_S_ROBUST_BEFORE = 1,  /* initial_num_landmarks (lib.rs:2670-2676) */
    AKZ_OF_S_ROBUST_AFTER = 2,   /* final_num_landmarks (lib.rs:2738-2744) */
    AKZ_OF_S_OBS_SPLIT = 3,      /* observations split off, over all its landmarks */
    AKZ_OF_S_PAIR_SPLIT = 4,     /* landmarks in state AKZ_OF_PAIR_SPLIT */
    AKZ_OF_S_NO_POINT = 5,       /* landmarks in state AKZ_OF_NO_POINT */
    AKZ_OF_S_KICKED = 6,         /* landmarks in state AKZ_OF_KICKED */
    AKZ_OF_STATS = 8             /* word 7 is 0 */
};
enum { AKZ_OF_NO_SOLVE = 255 };  /* tri_reason of a landmark whose filter ran no triangulation */
enum { AKZ_OF_ROBUST_BEFORE = 1, AKZ_OF_ROBUST_AFTER = 2 };   /* the bits of `robust` */

typedef struct akz_of_settings {
    double maximum_cosine_distance;      /* 1e-5 (cv-sfm/src/settings.rs:324-330) */
    double maximum_sine_distance;        /* 1e-1 (settings.rs:332-343) */
    unsigned minimum_robust_landmarks;   /* 32 (settings.rs:429-431) */
    akz_tri_settings tri;                /* tri.n_views = the views of the landmark's reconstruction */
} akz_of_settings;

typedef struct akz_of_result {
    int tri_reason;     /* AKZ_TRI_* of triangulate_landmark where it ran, AKZ_TRI_BAD_INDEX for a bad index, else AKZ_OF_NO_SOLVE */
    unsigned robust;    /* AKZ_OF_ROBUST_BEFORE | AKZ_OF_ROBUST_AFTER */
    unsigned n_split;   /* observations split off */
} akz_of_result;

/* min(robust_minimum_observations, views) of lib.rs:2913-2917 */
AKZ_RM_FN unsigned akz_of_need(const akz_tri_settings* t)
{
    return t->robust_minimum_observations < t->n_views ? t->robust_minimum_observations : t->n_views;
}

/* The verdict on a reconstruction from its count of robust landmarks after the filter (lib.rs:2747-2756) */
AKZ_RM_FN int akz_of_verdict(unsigned robust_after, unsigned minimum_robust_landmarks)
{
    return robust_after < minimum_robust_landmarks ? AKZ_OF_FEW_LANDMARKS : AKZ_OF_OK;
}

/* The filter of ONE landmark, for any source of observations: NAME(src, n, settings, keep, result) -> AKZ_OF_* state, with
 * FETCH(src, i, pose[12], bearing[3]) as AKZ_TRI_DEFINE_TRIANGULATE wants it and TRIANGULATE the function that macro made from
 * the same FETCH.  keep[i], i < n, is written in every case: 1 = observation i stays in the landmark, 0 = it was split off and
 * is a landmark of its own now.  The flags are the only per-observation state (a list may be longer than any register file):
 * observations are fetched again rather than held.
 *
 *   1. every observation is fetched once before any is judged — a bad index anywhere leaves the whole list as it is — and
 *      the pairs (0, j) of are_observations_robust are tried on the way, as the triangulator does;
 *   2. robust before: n >= min(robust_minimum_observations, views) and SOME pair with enough incidence (a disjunction: the
 *      order the pairs are tried in does not matter);
 *   3. the decision by the length of the list (lib.rs:2685-2734).  In the walk over a triangulated list an observation is
 *      split off when 1 - bearing(pose * point) . b > maximum_cosine_distance — `>`, so a NaN keeps it — and
 *      split_observation refuses to take the last observation out of a landmark (lib.rs:560-586), which it only meets when
 *      every observation fails: the last one in list order stays then;
 *   4. robust after: the same test on the observations that stayed, in their order.  A list nothing was taken from has the
 *      value it had before; one that kept a single observation is not robust; only a kicked list is searched again.
 * NAME##_pairs(src, n, keep, m, tri) is are_observations_robust on the m observations of the list whose flag is set. */
#define AKZ_OF_DEFINE_FILTER(NAME, SRC_T, FETCH, TRIANGULATE)                                                            \
    AKZ_RM_FN int NAME##_pairs(const SRC_T* src, unsigned n, const unsigned char* keep, unsigned m, const akz_tri_settings* tri) \
    {                                                                                                                    \
        double pose[12], b[3] = {0.0, 0.0, 0.0}, d0[3], d[3];                                                            \
        if (m < akz_of_need(tri)) return 0;                                                                              \
        for (unsigned i = 0; i + 1u < n; ++i) {                                                                          \
            if (!keep[i]) continue;                                                                                      \
            FETCH(src, i, pose, b);                                                                                      \
            akz_tri_world_bearing(pose, b, d0);                                                                          \
            for (unsigned j = i + 1u; j < n; ++j) {                                                                      \
                if (!keep[j]) continue;                                                                                  \
                FETCH(src, j, pose, b);                                                                                  \
                akz_tri_world_bearing(pose, b, d);                                                                       \
                if (akz_tri_pair_robust(d0, d, tri->incidence_minimum_cosine_distance)) return 1;                        \
            }                                                                                                            \
        }                                                                                                                \
        return 0;                                                                                                        \
    }                                                                                                                    \
    AKZ_RM_FN int NAME(const SRC_T* src, unsigned n, const akz_of_settings* st, unsigned char* keep, akz_of_result* res) \
    {                                                                                                                    \
        double pose[12], b[3] = {0.0, 0.0, 0.0}, d0[3] = {0.0, 0.0, 0.0}, d[3], p[4];                                    \
        int pair_ok = 0;                                                                                                 \
        res->tri_reason = AKZ_OF_NO_SOLVE;                                                                               \
        res->robust = 0u;                                                                                                \
        res->n_split = 0u;                                                                                               \
        for (unsigned i = 0; i < n; ++i) {                                                                               \
            if (!FETCH(src, i, pose, b)) {                                                                               \
                for (unsigned k = 0; k < n; ++k) keep[k] = 1;                                                            \
                res->tri_reason = AKZ_TRI_BAD_INDEX;                                                                     \
                return AKZ_OF_BAD_INDEX;                                                                                 \
            }                                                                                                            \
            akz_tri_world_bearing(pose, b, d);                                                                           \
            if (i == 0) {                                                                                                \
                d0[0] = d[0]; d0[1] = d[1]; d0[2] = d[2];                                                                \
            } else if (!pair_ok)                                                                                         \
                pair_ok = akz_tri_pair_robust(d0, d, st->tri.incidence_minimum_cosine_distance);                         \
        }                                                                                                                \
        int before = 0;                                                                                                  \
        if (n >= 2u && n >= akz_of_need(&st->tri)) {                                                                     \
            for (unsigned i = 1; i + 1u < n && !pair_ok; ++i) {                                                          \
                FETCH(src, i, pose, b);                                                                                  \
                akz_tri_world_bearing(pose, b, d0);                                                                      \
                for (unsigned j = i + 1u; j < n && !pair_ok; ++j) {                                                      \
                    FETCH(src, j, pose, b);                                                                              \
                    akz_tri_world_bearing(pose, b, d);                                                                   \
                    pair_ok = akz_tri_pair_robust(d0, d, st->tri.incidence_minimum_cosine_distance);                     \
                }                                                                                                        \
            }                                                                                                            \
            before = pair_ok;                                                                                            \
        }                                                                                                                \
        if (before) res->robust = AKZ_OF_ROBUST_BEFORE;                                                                  \
        if (n < 2u) {                                                                                                    \
            if (n == 1u) keep[0] = 1;                                                                                    \
            return AKZ_OF_SINGLE;                                                                                        \
        }                                                                                                                \
        if (n == 2u) {                                                                                                   \
            double first[12], inv[12], total[12], b0[3] = {0.0, 0.0, 0.0};                                               \
            FETCH(src, 0u, first, b0);                                                                                   \
            FETCH(src, 1u, pose, b);                                                                                     \
            akz_tv_pose_inverse(first, inv);                                                                             \
            akz_tvc_pose_mul(pose, inv, total);                                                                          \
            keep[0] = 1;                                                                                                 \
            if (akz_tv_bi_landmark_robust(total, b0, b, st->maximum_sine_distance)) {                                    \
                keep[1] = 1;                                                                                             \
                if (before) res->robust |= AKZ_OF_ROBUST_AFTER;                                                          \
                return AKZ_OF_KEPT;                                                                                      \
            }                                                                                                            \
            keep[1] = 0;                                                                                                 \
            res->n_split = 1u;                                                                                           \
            return AKZ_OF_PAIR_SPLIT;                                                                                    \
        }                                                                                                                \
        res->tri_reason = TRIANGULATE(src, n, 0, &st->tri, p);                                                           \
        if (res->tri_reason != AKZ_TRI_OK) {                                                                             \
            keep[0] = 1;                                                                                                 \
            for (unsigned i = 1; i < n; ++i) keep[i] = 0;                                                                \
            res->n_split = n - 1u;                                                                                       \
            return AKZ_OF_NO_POINT;                                                                                      \
        }                                                                                                                \
        unsigned left = n;                                                                                               \
        for (unsigned i = 0; i < n; ++i) {                                                                               \
            FETCH(src, i, pose, b);                                                                                      \
            const int off = akz_tv_transformed_distance(pose, p, b) > st->maximum_cosine_distance && left >= 2u;         \
            keep[i] = off ? 0 : 1;                                                                                       \
            left -= off ? 1u : 0u;                                                                                       \
        }                                                                                                                \
        res->n_split = n - left;                                                                                         \
        if (left == n) {                                                                                                 \
            if (before) res->robust |= AKZ_OF_ROBUST_AFTER;                                                              \
            return AKZ_OF_KEPT;                                                                                          \
        }                                                                                                                \
        if (NAME##_pairs(src, n, keep, left, &st->tri)) res->robust |= AKZ_OF_ROBUST_AFTER;                              \
        return AKZ_OF_KICKED;                                                                                            \
    }

#endif /* AKZ_OBSERVATION_FILTER_MATH_H */
