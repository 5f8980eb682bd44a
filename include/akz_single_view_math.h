/* akz_single_view_math.h — what cv-sfm's register_frame_subset does behind its consensus (the single-view L2 optimiser and
 * the consistency filter around it), written as plain IEEE double arithmetic so that gcc (the CPU checker,
 * tests/cpp/single_view_host.c) and hipcc (the gfx950 kernel of cv_amd/csrc/rs_single_view.hip) execute the same operation
 * sequence (build: -ffp-contract=off, no fast-math; sqrt is the one non-arithmetic primitive).  Parity is
 * "host build == HIP", bit for bit.  Built on akz_three_view_math.h (akz_tv_dot / cross / norm, akz_tv_apply_delta,
 * akz_tv_from_scaled_axis, akz_tv_pose_inverse, akz_tv_bi_landmark_robust, akz_tv_transformed_distance),
 * akz_three_view_constraint_math.h (akz_tvc_pose_mul, the product of two isometries) and akz_triangulate_math.h (the
 * triangulator): this header adds the gradient, the optimiser's state, the consistency test and the control flow, and no
 * second copy of any of those.
 *
 * Reference code restated here (paths relative to rust-cv/cv):
 *   world_pose_gradient                                 cv-geom/src/epipolar.rs:188-193
 *   landmark_delta, single_view_simple_optimize_l2      cv-optimize/src/single_view_optimizer.rs:4-14, 80-135
 *   Se3TangentSpace::new / scale / isometry             cv-core/src/so3.rs:23-60, 78-82
 *   Pose::transform, Projective::point                  cv-core/src/pose.rs:125-133, cv-core/src/point.rs:37-39
 *   VSlam::is_observation_consistent                    cv-sfm/src/lib.rs:2622-2655
 *   VSlam::is_bi_landmark_robust                        cv-sfm/src/lib.rs:1306-1317
 *   register_frame_subset behind its consensus          cv-sfm/src/lib.rs:1625-1775
 *
 * Unpinned against the reference:
 *   - THE ORDER OF THE SUM OVER MATCHES: akz_sum_order.h, a workgroup's; thread t's partial is the 6 gradient components of
 *     matches t, t + 256, ..., a match whose landmark_delta is None adding nothing.  akz_sv_sum_tree executes it on the host;
 *     akz_sv_sum_sequential is the reference's order, kept for the test that documents what the choice costs;
 *   - Rotation3::from_scaled_axis (akz_tv_from_scaled_axis: Rodrigues with the sine and cosine of akz_portable_math.h);
 *   - the eigen-solver and the product orders of akz_triangulate_math.h's own list;
 *   - the order of a landmark's observations: the reference walks a HashMap; here it is the order of the caller's list.  A
 *     merged match contributes the observations of its first landmark followed by those of its second;
 *   - the point of a chosen match is kept as the Euclidean xyz / w, divided once when the match is chosen, and landmark_delta
 *     transforms that (R x + t) where the reference transforms the homogeneous vector, normalises it and divides by w in
 *     every iteration: the same value in exact arithmetic, other roundings.  w == 0 (Projective::point gives None) is kept
 *     as a NaN point, and a NaN point is skipped in the sum — while inv_landmark_len still counts it, as the reference's.
 *   - is_observation_consistent on a match with no other observation: "unreachable" in the reference; here the match is not
 *     consistent, and a stats word counts such matches.
 *
 * Read against delta.isometry() * pose (so3.rs:57-60): with t the point in camera axes and b the bearing, the translation
 * gradient (t.b) b - t moves the point towards its ray and the rotation gradient (t / |t|) x b turns t towards b
 * ((u x b) x u = b - u (u.b)): both descend, unlike the three-view translation gradients.
 */
#ifndef AKZ_SINGLE_VIEW_MATH_H
#define AKZ_SINGLE_VIEW_MATH_H

#include "akz_three_view_constraint_math.h"

enum { AKZ_SV_THREADS = AKZ_SUM_THREADS, AKZ_SV_WAVE = AKZ_SUM_WAVE, AKZ_SV_MAX_MATCHES = 2048, AKZ_SV_MAX_RUNS = 9, AKZ_SV_NO_IMPROVE = 50 };

/* verdicts (RS_SV_* of include/akz.h) */
enum {
    AKZ_SV_OK = 0,
    AKZ_SV_NO_MODEL = 1,        /* the consensus found no pose (lib.rs:1619-1622): passed through */
    AKZ_SV_FEW_LANDMARKS = 2,   /* fewer than single_view_minimum_landmarks robust matches (lib.rs:1606) */
    AKZ_SV_LOST_HALF = 3,       /* no more than half of the inliers taken left (lib.rs:1650, 1697, 1737) */
    AKZ_SV_FEW_ROBUST = 4,      /* final_matches.len() < single_view_minimum_robust_landmarks (lib.rs:1766) */
    AKZ_SV_BAD_INDEX = 5
};
/* the stage a verdict was reached at (stats word AKZ_SV_S_STAGE) */
enum {
    AKZ_SV_STAGE_INDEX = 0, AKZ_SV_STAGE_LANDMARKS = 1, AKZ_SV_STAGE_MODEL = 2, AKZ_SV_STAGE_RUN0 = 3 /* + run */,
    AKZ_SV_STAGE_FINAL = 12 /* final_num_robust_matches */, AKZ_SV_STAGE_MINIMUM = 13 /* final_matches.len(), and OK */
};
/* stats words (u32) */
enum {
    AKZ_SV_S_INLIERS = 0,       /* inliers taken (lib.rs:1626-1630) */
    AKZ_SV_S_RUN_MATCHES = 1,   /* [9] matches entering run r; 0xFFFFFFFF for a run not reached */
    AKZ_SV_S_RUN_STOP = 10,     /* [9] the `iteration` run r left its loop at; 0xFFFFFFFF for a run not made */
    AKZ_SV_S_ROBUST = 19,       /* final_num_robust_matches */
    AKZ_SV_S_NO_OTHER = 20,     /* original matches with no other observation */
    AKZ_SV_S_STAGE = 21,
    AKZ_SV_STATS = 24           /* words 22, 23 are 0 */
};

typedef struct akz_sv_settings {
    double maximum_cosine_distance;                      /* 1e-5 */
    double maximum_sine_distance;                        /* 1e-1 */
    double single_view_optimization_rate;                /* 1e-3 */
    unsigned single_view_optimization_num_matches;       /* 2048 (<= AKZ_SV_MAX_MATCHES) */
    unsigned single_view_filter_loop_iterations;         /* 5 (<= AKZ_SV_MAX_RUNS - 1) */
    unsigned single_view_patience;                       /* 100000: the optimiser's `iterations` */
    unsigned single_view_minimum_landmarks;              /* 32 */
    unsigned single_view_minimum_robust_landmarks;       /* 64 */
    akz_tri_settings tri;
} akz_sv_settings;

/* world_pose_gradient (epipolar.rs:188-193) behind Se3TangentSpace::new (so3.rs:23-34: a vector with a NaN in ANY component
 * becomes the zero vector, each of the two on its own).  t = the point in the camera's axes, g = {translation, rotation}. */
AKZ_RM_FN void akz_sv_world_pose_gradient(const double* t, const double* b, double* g)
{
    const double d = akz_tv_dot(t, b);
    AKZ_RM_UNROLL
    for (int k = 0; k < 3; ++k) g[k] = d * b[k] - t[k];
    const double n = akz_tv_norm(t);
    const double u[3] = {t[0] / n, t[1] / n, t[2] / n};
    akz_tv_cross(u, b, g + 3);
    AKZ_RM_UNROLL
    for (int v = 0; v < 2; ++v) {
        if (akz_tv_any_nan(g + 3 * v)) {
            g[3 * v] = 0.0; g[3 * v + 1] = 0.0; g[3 * v + 2] = 0.0;
        }
    }
}

/* The Euclidean point of a homogeneous one, as a chosen match keeps it (see the head of this file): xyz / w, NaN for w == 0. */
AKZ_RM_FN void akz_sv_point(const double* world, double* x)
{
    if (world[3] == 0.0) {
        const double nan = __builtin_nan("");
        x[0] = nan; x[1] = nan; x[2] = nan;
        return;
    }
    x[0] = world[0] / world[3]; x[1] = world[1] / world[3]; x[2] = world[2] / world[3];
}

/* "the world row is Some": w >= 0, the matcher's own test (a row with w < 0, or a NaN, says None) */
AKZ_RM_FN int akz_sv_some(const double* world) { return world[3] >= 0.0; }

/* landmark_delta (single_view_optimizer.rs:4-14): 1 and g [6], or 0 ("None": the match is skipped in the sum). */
AKZ_RM_FN int akz_sv_landmark_delta(const double* pose, const double* b, const double* x, double* g)
{
    if (x[0] != x[0]) return 0;
    double t[3];
    AKZ_RM_UNROLL
    for (int i = 0; i < 3; ++i) t[i] = ((pose[i * 4] * x[0] + pose[i * 4 + 1] * x[1]) + pose[i * 4 + 2] * x[2]) + pose[i * 4 + 3];
    akz_sv_world_pose_gradient(t, b, g);
    return 1;
}

/* The state of one optimiser run between iterations (single_view_optimizer.rs:89-91). */
typedef struct akz_sv_opt_state {
    double best_trans, best_rot;
    unsigned no_improve_for;
} akz_sv_opt_state;
AKZ_RM_FN void akz_sv_opt_begin(akz_sv_opt_state* st)
{
    st->best_trans = __builtin_inf();
    st->best_rot = __builtin_inf();
    st->no_improve_for = 0;
}
/* One iteration after the sum (single_view_optimizer.rs:101-132): net [6] the summed gradient.  tangent = l2sum.scale(
 * inv_landmark_len), delta = tangent.scale(rate): two products.  The comparisons are strict (best > norm), a NaN norm
 * never improves.  Returns 0 to go on, 1 for the no-improvement break (taken BEFORE the pose moves), 2 for the
 * last-iteration break (after). */
AKZ_RM_FN int akz_sv_opt_step(akz_sv_opt_state* st, const double* net, double inv_landmark_len, double rate, double* pose, unsigned iteration,
                              unsigned iterations)
{
    double delta[6];
    AKZ_RM_UNROLL
    for (int k = 0; k < 6; ++k) delta[k] = (net[k] * inv_landmark_len) * rate;
    st->no_improve_for += 1;
    const double t = akz_tv_norm(net), r = akz_tv_norm(net + 3);
    if (st->best_trans > t) {
        st->best_trans = t;
        st->no_improve_for = 0;
    }
    if (st->best_rot > r) {
        st->best_rot = r;
        st->no_improve_for = 0;
    }
    if (st->no_improve_for >= (unsigned)AKZ_SV_NO_IMPROVE) return 1;
    akz_tv_apply_delta(delta, pose);
    if (iteration == iterations - 1u) return 2;
    return 0;
}

/* is_observation_consistent (lib.rs:2622-2655) for any source of observations: NAME(src, k, pose, bearing, settings) -> 1
 * or 0, with FETCH(src, i, pose[12], bearing[3]) as AKZ_TRI_DEFINE_TRIANGULATE wants it — observation i < k is the i-th
 * OTHER observation, observation k is (pose, bearing) itself — and TRIANGULATE the function that macro made from the same
 * FETCH.  A FETCH that refuses gives 0.
 *   k == 0: not consistent (see the head of this file);
 *   k == 1: is_bi_landmark_robust(other_pose * pose^-1, bearing, other_bearing, maximum_sine_distance);
 *   k >= 2: triangulate_observations over the others followed by (pose, bearing), no robustness test, then EVERY one of the
 *           k + 1 must satisfy 1 - bearing(pose * point) . b < maximum_cosine_distance — `<`, so a NaN fails, where the
 *           observation filter's walk splits on `>` and a NaN stays: the two comparisons are not shared. */
#define AKZ_SV_DEFINE_CONSISTENT(NAME, SRC_T, FETCH, TRIANGULATE)                                                        \
    AKZ_RM_FN int NAME(const SRC_T* src, unsigned k, const double* pose, const double* bearing, const akz_sv_settings* st) \
    {                                                                                                                    \
        double op[12], ob[3] = {0.0, 0.0, 0.0}, p[4];                                                                    \
        if (k == 0u) return 0;                                                                                           \
        if (k == 1u) {                                                                                                   \
            double inv[12], total[12];                                                                                   \
            if (!FETCH(src, 0u, op, ob)) return 0;                                                                       \
            akz_tv_pose_inverse(pose, inv);                                                                              \
            akz_tvc_pose_mul(op, inv, total);                                                                            \
            return akz_tv_bi_landmark_robust(total, bearing, ob, st->maximum_sine_distance);                             \
        }                                                                                                                \
        if (TRIANGULATE(src, k + 1u, 0, &st->tri, p) != AKZ_TRI_OK) return 0;                                            \
        for (unsigned i = 0; i <= k; ++i) {                                                                              \
            FETCH(src, i, op, ob);                                                                                       \
            if (!(akz_tv_transformed_distance(op, p, ob) < st->maximum_cosine_distance)) return 0;                       \
        }                                                                                                                \
        return 1;                                                                                                        \
    }

/* the verdict behind the final pass (lib.rs:1737-1772): robust = final_num_robust_matches, n_final = final_matches.len() */
AKZ_RM_FN int akz_sv_final_verdict(unsigned robust, unsigned n_final, unsigned robust_minimum_matches, unsigned minimum_robust_landmarks,
                                   unsigned* stage)
{
    *stage = AKZ_SV_STAGE_FINAL;
    if (robust <= robust_minimum_matches) return AKZ_SV_LOST_HALF;
    *stage = AKZ_SV_STAGE_MINIMUM;
    if (n_final < minimum_robust_landmarks) return AKZ_SV_FEW_ROBUST;
    return AKZ_SV_OK;
}

/* ---- the host's execution of the whole procedure (the kernel restates the control flow with a workgroup) ---- */
#if !defined(__HIP_DEVICE_COMPILE__)
#define AKZ_SV_HOST_FN static inline

/* chosen matches as the kernel keeps them: lm[k * AKZ_SV_MAX_MATCHES + i] = component k (bearing xyz, point xyz) of match i */
AKZ_SV_HOST_FN void akz_sv_sum_tree(const double* pose, const double* lm, unsigned n, double* net)
{
    double part[AKZ_SV_THREADS][6];
    for (unsigned t = 0; t < (unsigned)AKZ_SV_THREADS; ++t) {
        for (int k = 0; k < 6; ++k) part[t][k] = 0.0;
        for (unsigned i = t; i < n; i += (unsigned)AKZ_SV_THREADS) {
            double b[3], x[3], g[6];
            for (int k = 0; k < 3; ++k) {
                b[k] = lm[k * AKZ_SV_MAX_MATCHES + i];
                x[k] = lm[(3 + k) * AKZ_SV_MAX_MATCHES + i];
            }
            if (!akz_sv_landmark_delta(pose, b, x, g)) continue;
            for (int k = 0; k < 6; ++k) part[t][k] = part[t][k] + g[k];
        }
    }
    akz_sum_block(&part[0][0], 6, net);
}
AKZ_SV_HOST_FN void akz_sv_sum_sequential(const double* pose, const double* lm, unsigned n, double* net)
{
    for (int k = 0; k < 6; ++k) net[k] = 0.0;
    for (unsigned i = 0; i < n; ++i) {
        double b[3], x[3], g[6];
        for (int k = 0; k < 3; ++k) {
            b[k] = lm[k * AKZ_SV_MAX_MATCHES + i];
            x[k] = lm[(3 + k) * AKZ_SV_MAX_MATCHES + i];
        }
        if (!akz_sv_landmark_delta(pose, b, x, g)) continue;
        for (int k = 0; k < 6; ++k) net[k] += g[k];
    }
}

/* single_view_simple_optimize_l2 (single_view_optimizer.rs:80-135): pose [12] in and out; returns the `iteration` the loop
 * was left at (0 for iterations == 0 or no landmarks: the pose is untouched). */
AKZ_SV_HOST_FN unsigned akz_sv_optimize(double* pose, double rate, unsigned iterations, const double* lm, unsigned n, int sequential)
{
    double net[6];
    akz_sv_opt_state st;
    unsigned iteration = 0;
    if (n == 0) return 0;
    const double inv_landmark_len = 1.0 / (double)n;
    akz_sv_opt_begin(&st);
    for (; iteration < iterations; ++iteration) {
        if (sequential) akz_sv_sum_sequential(pose, lm, n, net);
        else akz_sv_sum_tree(pose, lm, n, net);
        if (akz_sv_opt_step(&st, net, inv_landmark_len, rate, pose, iteration, iterations)) break;
    }
    return iteration;
}

/* One scene on the host: the original matches in their order, every one with its bearing in the new frame, its world point
 * (w < 0: "None") and its other observations obs_start[i] .. obs_start[i + 1] of obs_pose / obs_bearing (a merged match:
 * the first landmark's followed by the second's). */
typedef struct akz_sv_scene {
    unsigned n;
    const double* bearing;        /* [n][3] */
    const double* world;          /* [n][4] */
    const unsigned* obs_start;    /* [n + 1] */
    const double* obs_pose;       /* [..][12] */
    const double* obs_bearing;    /* [..][3] */
} akz_sv_scene;
typedef struct akz_sv_host_src {
    const akz_sv_scene* sc;
    unsigned s0, k;
    const double* pose;
    const double* bearing;
} akz_sv_host_src;
AKZ_SV_HOST_FN int akz_sv_host_fetch(const akz_sv_host_src* s, unsigned i, double* pose, double* b)
{
    const double* p = i < s->k ? s->sc->obs_pose + 12 * (size_t)(s->s0 + i) : s->pose;
    const double* v = i < s->k ? s->sc->obs_bearing + 3 * (size_t)(s->s0 + i) : s->bearing;
    for (int k = 0; k < 12; ++k) pose[k] = p[k];
    b[0] = v[0]; b[1] = v[1]; b[2] = v[2];
    return 1;
}
AKZ_TRI_DEFINE_TRIANGULATE(akz_sv_host_triangulate, akz_sv_host_src, akz_sv_host_fetch)
AKZ_SV_DEFINE_CONSISTENT(akz_sv_host_consistent_src, akz_sv_host_src, akz_sv_host_fetch, akz_sv_host_triangulate)
AKZ_SV_HOST_FN int akz_sv_host_consistent(const akz_sv_scene* sc, unsigned i, const double* pose, const akz_sv_settings* st)
{
    akz_sv_host_src src;
    src.sc = sc; src.s0 = sc->obs_start[i]; src.k = sc->obs_start[i + 1] - sc->obs_start[i];
    src.pose = pose; src.bearing = sc->bearing + 3 * (size_t)i;
    return akz_sv_host_consistent_src(&src, src.k, pose, src.bearing, st);
}
AKZ_SV_HOST_FN void akz_sv_host_put(const akz_sv_scene* sc, unsigned i, double* lm, unsigned slot)
{
    double x[3];
    akz_sv_point(sc->world + 4 * (size_t)i, x);
    for (int k = 0; k < 3; ++k) {
        lm[k * AKZ_SV_MAX_MATCHES + slot] = sc->bearing[3 * (size_t)i + k];
        lm[(3 + k) * AKZ_SV_MAX_MATCHES + slot] = x[k];
    }
}

/* The first num_matches original matches, in list order, that are consistent under `pose` and whose world row is Some
 * (lib.rs:1664-1693).  Matches behind the last one taken are not looked at. */
AKZ_SV_HOST_FN unsigned akz_sv_take(const akz_sv_scene* sc, const double* pose, const akz_sv_settings* st, double* lm)
{
    unsigned m = 0;
    for (unsigned i = 0; i < sc->n && m < st->single_view_optimization_num_matches; ++i) {
        if (!akz_sv_some(sc->world + 4 * (size_t)i)) continue;
        if (!akz_sv_host_consistent(sc, i, pose, st)) continue;
        akz_sv_host_put(sc, i, lm, m++);
    }
    return m;
}

/* register_frame_subset from its consensus on (lib.rs:1606-1775).  pose_in [12] and the inlier indices are the consensus'
 * (has_model == 0: it found none); inlier index k names the k-th original match whose world row is Some.  lm: scratch for
 * 6 * AKZ_SV_MAX_MATCHES doubles.  pose_out [12] is written for AKZ_SV_OK and AKZ_SV_NO_MODEL (a copy); final_mask [n] and
 * *n_final once the final pass is reached (*n_final = 0 before); stats [AKZ_SV_STATS] always.  Returns the verdict. */
AKZ_SV_HOST_FN int akz_sv_refine_scene(const akz_sv_scene* sc, const double* pose_in, int has_model, const unsigned* inliers, unsigned n_inliers,
                                       const akz_sv_settings* st, int sequential, double* lm, double* pose_out, unsigned char* final_mask,
                                       unsigned* n_final, unsigned* stats)
{
    double pose[12];
    unsigned n_rob = 0, no_other = 0;
    for (int k = 0; k < AKZ_SV_STATS; ++k) stats[k] = 0u;
    for (int r = 0; r < 2 * AKZ_SV_MAX_RUNS; ++r) stats[AKZ_SV_S_RUN_MATCHES + r] = 0xFFFFFFFFu;
    *n_final = 0u;
    for (unsigned i = 0; i < sc->n; ++i) {
        n_rob += akz_sv_some(sc->world + 4 * (size_t)i) ? 1u : 0u;
        no_other += sc->obs_start[i + 1] == sc->obs_start[i] ? 1u : 0u;
    }
    stats[AKZ_SV_S_NO_OTHER] = no_other;
    stats[AKZ_SV_S_STAGE] = AKZ_SV_STAGE_LANDMARKS;
    if (n_rob < st->single_view_minimum_landmarks) return AKZ_SV_FEW_LANDMARKS;
    stats[AKZ_SV_S_STAGE] = AKZ_SV_STAGE_MODEL;
    if (!has_model) {
        for (int k = 0; k < 12; ++k) pose_out[k] = pose_in[k];
        return AKZ_SV_NO_MODEL;
    }
    for (int k = 0; k < 12; ++k) pose[k] = pose_in[k];
    /* take(num_matches) of the inliers (lib.rs:1626-1630) */
    unsigned n_opt = n_inliers < st->single_view_optimization_num_matches ? n_inliers : st->single_view_optimization_num_matches;
    for (unsigned k = 0; k < n_opt; ++k)
        if (inliers[k] >= n_rob) {
            stats[AKZ_SV_S_STAGE] = AKZ_SV_STAGE_INDEX;
            return AKZ_SV_BAD_INDEX;
        }
    for (unsigned i = 0, r = 0; i < sc->n; ++i) {
        if (!akz_sv_some(sc->world + 4 * (size_t)i)) continue;
        for (unsigned k = 0; k < n_opt; ++k)
            if (inliers[k] == r) akz_sv_host_put(sc, i, lm, k);
        ++r;
    }
    stats[AKZ_SV_S_INLIERS] = n_opt;
    const unsigned robust_minimum_matches = n_opt / 2u;
    for (unsigned run = 0; run <= st->single_view_filter_loop_iterations; ++run) {
        stats[AKZ_SV_S_STAGE] = AKZ_SV_STAGE_RUN0 + run;
        stats[AKZ_SV_S_RUN_MATCHES + run] = n_opt;
        if (n_opt <= robust_minimum_matches) return AKZ_SV_LOST_HALF;
        stats[AKZ_SV_S_RUN_STOP + run] = akz_sv_optimize(pose, st->single_view_optimization_rate, st->single_view_patience, lm, n_opt, sequential);
        if (run < st->single_view_filter_loop_iterations) n_opt = akz_sv_take(sc, pose, st, lm);
    }
    /* the consistent flag once; both final counts from it (lib.rs:1712-1759) */
    unsigned robust = 0, nf = 0;
    for (unsigned i = 0; i < sc->n; ++i) {
        const int ok = akz_sv_host_consistent(sc, i, pose, st);
        final_mask[i] = (unsigned char)ok;
        nf += ok ? 1u : 0u;
        robust += ok && akz_sv_some(sc->world + 4 * (size_t)i) ? 1u : 0u;
    }
    *n_final = nf;
    stats[AKZ_SV_S_ROBUST] = robust;
    unsigned stage;
    const int v = akz_sv_final_verdict(robust, nf, robust_minimum_matches, st->single_view_minimum_robust_landmarks, &stage);
    stats[AKZ_SV_S_STAGE] = stage;
    if (v == AKZ_SV_OK)
        for (int k = 0; k < 12; ++k) pose_out[k] = pose[k];
    return v;
}
#endif /* !__HIP_DEVICE_COMPILE__ */

#endif /* AKZ_SINGLE_VIEW_MATH_H */
