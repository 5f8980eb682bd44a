/* akz_three_view_constraint_math.h — one three-view constraint of cv-sfm's pose graph (VSlam::optimize_three_view) and the
 * adaptive L2 three-view optimiser it runs, written as plain IEEE double arithmetic so that gcc (the CPU checker,
 * tests/cpp/three_view_constraint_host.c) and hipcc (the gfx950 kernel of cv_amd/csrc/rs_three_view_constraint.hip) execute
 * the same operation sequence (build: -ffp-contract=off, no fast-math; sqrt is the one non-arithmetic primitive).  Parity is
 * "host build == HIP", bit for bit.  Built on akz_three_view_math.h, which this file leaves as it is: the gradients of a
 * landmark, the exponential map, the pose inverse, the bearing-pair test and Pose::scale are that header's.
 *
 * Reference code restated here (paths relative to rust-cv/cv):
 *   three_view_adaptive_optimize_l2                     cv-optimize/src/three_view_optimizer.rs:203-272
 *   Se3TangentSpace::scale / scale_translation /
 *   scale_rotation / isometry                           cv-core/src/so3.rs:57-60, 78-98
 *   optimize_three_view                                 cv-sfm/src/lib.rs:1939-2062
 *   the settings it reads                               cv-sfm/src/settings.rs:332-338, 465-483
 *
 * Unpinned against the reference (nalgebra 0.30 is not vendored in the reference tree):
 *   - everything akz_three_view_math.h lists: Rotation3::from_scaled_axis, the order of nalgebra's products and norms;
 *   - the product of two isometries (akz_tvc_pose_mul): R = Ra Rb, t = Ra tb + ta, every three-term sum ((x0 + x1) + x2);
 *   - the sign and payload of a NaN (a pose table with a NaN in it): every NaN written is the quiet NaN of akz_tvc_canonical;
 *   - landmarks.shuffle (the caller's RNG) and sort_unstable_by_key (Rust's order among equal keys): both stay with the
 *     caller, who hands over the list in the order the reference would walk it in;
 *   - THE ORDER OF THE SUM OVER LANDMARKS: akz_sum_order.h, one wave's; lane l's partial is the 16 quantities (12 gradient
 *     components, then the norms of the first translation, first rotation, second translation, second rotation) of landmarks
 *     l, l + 64, ...  akz_tvc_sum_wave below executes it on the host; akz_tvc_sum_sequential is the reference's order, kept
 *     for the test that documents what the choice costs.
 *
 * The finding of akz_three_view_math.h holds here as well: on a well-posed scene every translation gradient is exactly
 * zero, so the translation's rate is 0 / 0, which the reference's is_finite test turns into 0.  The text is shipped as it is.
 */
#ifndef AKZ_THREE_VIEW_CONSTRAINT_MATH_H
#define AKZ_THREE_VIEW_CONSTRAINT_MATH_H

#include "akz_three_view_math.h"

enum { AKZ_TVC_WAVE = AKZ_SUM_WAVE, AKZ_TVC_MAX_LANDMARKS = 256, AKZ_TVC_MAX_ITERATIONS = 1 << 20 };

/* verdicts (RS_TVC_* of include/akz.h) */
enum {
    AKZ_TVC_OK = 0,
    AKZ_TVC_FEW_LANDMARKS = 1,      /* lib.rs:1949 */
    AKZ_TVC_FEW_BEARING_PAIRS = 2,  /* lib.rs:2026 */
    AKZ_TVC_BAD_INDEX = 3
};
/* the stage a verdict was reached at (stats word AKZ_TVC_S_STAGE) */
enum { AKZ_TVC_STAGE_INDEX = 0, AKZ_TVC_STAGE_LANDMARKS = 1, AKZ_TVC_STAGE_PAIRS = 2, AKZ_TVC_STAGE_FINAL = 3 };
/* stats words (u32); a word behind the stage the verdict fell at is 0 */
enum {
    AKZ_TVC_S_LANDMARKS = 0,        /* the length of the constraint's list */
    AKZ_TVC_S_USED = 1,             /* min(length, optimization_maximum_landmarks) */
    AKZ_TVC_S_PAIRS = 2,            /* robust bearing pairs among the used landmarks */
    AKZ_TVC_S_ORIGINAL_SCALE = 3,   /* [2] the bits of its f64, low word first */
    AKZ_TVC_S_FINAL_SCALE = 5,      /* [2] */
    AKZ_TVC_S_STAGE = 7,
    AKZ_TVC_STATS = 8
};

typedef struct akz_tvc_settings {
    double robust_view_bearing_pair_minimum_cosine_distance;   /* 1e-2 */
    unsigned optimization_minimum_landmarks;                   /* 24 */
    unsigned optimization_maximum_landmarks;                   /* 64 (<= AKZ_TVC_MAX_LANDMARKS) */
    unsigned constraint_patience;                              /* 4096: the optimiser's `iterations` */
    unsigned robust_view_num_robust_bearing_pair;              /* 3 */
} akz_tvc_settings;

/* a * b of two isometries [R | t], row-major [12] (nalgebra: R = Ra Rb, t = Ra tb + ta); out may not alias a or b */
AKZ_RM_FN void akz_tvc_pose_mul(const double* a, const double* b, double* out)
{
    AKZ_RM_UNROLL
    for (int i = 0; i < 3; ++i) {
        AKZ_RM_UNROLL
        for (int j = 0; j < 3; ++j) out[i * 4 + j] = (a[i * 4] * b[j] + a[i * 4 + 1] * b[4 + j]) + a[i * 4 + 2] * b[8 + j];
        out[i * 4 + 3] = ((a[i * 4] * b[3] + a[i * 4 + 1] * b[7]) + a[i * 4 + 2] * b[11]) + a[i * 4 + 3];
    }
}

/* the relative poses of lib.rs:1962-1963 from three WorldToCamera poses: rel = {w1 * w0^-1, w2 * w0^-1}, [2][12] */
AKZ_RM_FN void akz_tvc_relative_poses(const double* w0, const double* w1, const double* w2, double* rel)
{
    double inv0[12];
    akz_tv_pose_inverse(w0, inv0);
    akz_tvc_pose_mul(w1, inv0, rel);
    akz_tvc_pose_mul(w2, inv0, rel + 12);
}

/* ||t_first|| + ||t_second|| (lib.rs:1965-1966, 2045-2046) */
AKZ_RM_FN double akz_tvc_scale_of(const double* rel)
{
    const double t0[3] = {rel[3], rel[7], rel[11]}, t1[3] = {rel[15], rel[19], rel[23]};
    return akz_tv_norm(t0) + akz_tv_norm(t1);
}

/* What one landmark adds to the 16 running sums (three_view_optimizer.rs:223-231): acc[k] = acc[k] + q[k]. */
AKZ_RM_FN void akz_tvc_accumulate(const double* inv, const double* c, const double* f, const double* s, double* acc)
{
    double g[12];
    akz_tv_landmark_gradients(inv, c, f, s, g);
    AKZ_RM_UNROLL
    for (int k = 0; k < 12; ++k) acc[k] = acc[k] + g[k];
    AKZ_RM_UNROLL
    for (int v = 0; v < 4; ++v) acc[12 + v] = acc[12 + v] + akz_tv_norm(g + 3 * v);
}

/* a rate that is not finite (NaN, +inf, -inf) becomes 0 (three_view_optimizer.rs:244, 246) */
AKZ_RM_FN double akz_tvc_rate(double norm, double std)
{
    const double rate = norm / std;
    return AKZ_TRI_FINITE(rate) ? rate : 0.0;
}

/* One iteration after the sum (three_view_optimizer.rs:233-254): nets16 = the 12 summed gradient components, then the four
 * summed norms {|t1|, |r1|, |t2|, |r2|}; inv [2][12] the inverted poses, moved in place. */
AKZ_RM_FN void akz_tvc_adaptive_step(const double* nets16, double inv_len, double* inv)
{
    AKZ_RM_UNROLL
    for (int p = 0; p < 2; ++p) {
        double l2[6], delta[6];
        AKZ_RM_UNROLL
        for (int k = 0; k < 6; ++k) l2[k] = nets16[6 * p + k] * inv_len;
        const double tstd = nets16[12 + 2 * p] * inv_len, rstd = nets16[13 + 2 * p] * inv_len;
        const double trate = akz_tvc_rate(akz_tv_norm(l2), tstd);
        const double rrate = akz_tvc_rate(akz_tv_norm(l2 + 3), rstd);
        AKZ_RM_UNROLL
        for (int k = 0; k < 3; ++k) {
            delta[k] = l2[k] * trate;
            delta[3 + k] = l2[3 + k] * rrate;
        }
        akz_tv_apply_delta(delta, inv + 12 * p);
    }
}

/* What leaves a constraint as NaN leaves it as THE quiet NaN 0x7FF8000000000000: which operand's sign and payload a NaN
 * inherits on its way through a product differs between x86 and gfx950, and the reference fixes neither. */
AKZ_RM_FN double akz_tvc_canonical(double x)
{
    if (x != x) {
        const unsigned long long u = 0x7FF8000000000000ull;
        __builtin_memcpy(&x, &u, sizeof x);
    }
    return x;
}

/* ---- the host's execution of the whole procedure (the kernel restates the control flow with one wavefront) ---- */
#if !defined(__HIP_DEVICE_COMPILE__)
#define AKZ_TVC_HOST_FN static inline

/* landmarks [n][9] = {c xyz, f xyz, s xyz}, n <= AKZ_TVC_MAX_LANDMARKS */
AKZ_TVC_HOST_FN void akz_tvc_sum_wave(const double* inv, const double* lm9, unsigned n, double* nets16)
{
    double part[AKZ_TVC_WAVE][16];
    for (unsigned l = 0; l < (unsigned)AKZ_TVC_WAVE; ++l) {
        for (int k = 0; k < 16; ++k) part[l][k] = 0.0;
        for (unsigned i = l; i < n; i += (unsigned)AKZ_TVC_WAVE) akz_tvc_accumulate(inv, lm9 + 9 * (size_t)i, lm9 + 9 * (size_t)i + 3, lm9 + 9 * (size_t)i + 6, part[l]);
    }
    for (int k = 0; k < 16; ++k) nets16[k] = akz_sum_wave(&part[0][k], 16);
}
AKZ_TVC_HOST_FN void akz_tvc_sum_sequential(const double* inv, const double* lm9, unsigned n, double* nets16)
{
    for (int k = 0; k < 16; ++k) nets16[k] = 0.0;
    for (unsigned i = 0; i < n; ++i) akz_tvc_accumulate(inv, lm9 + 9 * (size_t)i, lm9 + 9 * (size_t)i + 3, lm9 + 9 * (size_t)i + 6, nets16);
}

/* three_view_adaptive_optimize_l2 (three_view_optimizer.rs:203-272): poses [2][12] in and out.  No early exit: every
 * iteration runs.  More iterations than AKZ_TVC_MAX_ITERATIONS count as that (the bound that makes the time finite). */
AKZ_TVC_HOST_FN void akz_tvc_adaptive_optimize(double* poses, unsigned iterations, const double* lm9, unsigned n, int sequential)
{
    double inv[24], nets[16];
    if (n == 0) return;
    if (iterations > (unsigned)AKZ_TVC_MAX_ITERATIONS) iterations = (unsigned)AKZ_TVC_MAX_ITERATIONS;
    const double inv_len = 1.0 / (double)n;
    akz_tv_pose_inverse(poses, inv);
    akz_tv_pose_inverse(poses + 12, inv + 12);
    for (unsigned iteration = 0; iteration < iterations; ++iteration) {
        if (sequential) akz_tvc_sum_sequential(inv, lm9, n, nets);
        else akz_tvc_sum_wave(inv, lm9, n, nets);
        akz_tvc_adaptive_step(nets, inv_len, inv);
    }
    akz_tv_pose_inverse(inv, poses);
    akz_tv_pose_inverse(inv + 12, poses + 12);
}

AKZ_TVC_HOST_FN void akz_tvc_put_f64(unsigned* stats, int at, double x)
{
    unsigned long long u;
    __builtin_memcpy(&u, &x, sizeof u);
    stats[at] = (unsigned)(u & 0xFFFFFFFFull);
    stats[at + 1] = (unsigned)(u >> 32);
}

/* optimize_three_view (lib.rs:1939-2062) behind the caller's shuffle and sort: world [3][12] the three views' WorldToCamera
 * poses, lm9 [n_list][9] the bearings of the list's landmarks in the caller's order (only the first
 * min(n_list, optimization_maximum_landmarks) are read).  pose_out [2][12] is written for AKZ_TVC_OK only, stats
 * [AKZ_TVC_STATS] always. */
AKZ_TVC_HOST_FN int akz_tvc_constraint(const double* world, const double* lm9, unsigned n_list, const akz_tvc_settings* st, int sequential,
                                       double* pose_out, unsigned* stats)
{
    double rel[24];
    for (int k = 0; k < AKZ_TVC_STATS; ++k) stats[k] = 0u;
    stats[AKZ_TVC_S_LANDMARKS] = n_list;
    stats[AKZ_TVC_S_STAGE] = AKZ_TVC_STAGE_LANDMARKS;
    if (n_list < st->optimization_minimum_landmarks) return AKZ_TVC_FEW_LANDMARKS;
    akz_tvc_relative_poses(world, world + 12, world + 24, rel);
    const double original_scale = akz_tvc_scale_of(rel);
    const unsigned used = n_list < st->optimization_maximum_landmarks ? n_list : st->optimization_maximum_landmarks;
    unsigned pairs = 0;
    for (unsigned i = 0; i < used; ++i)
        for (unsigned j = i + 1; j < used; ++j) {
            const double *a = lm9 + 9 * (size_t)i, *b = lm9 + 9 * (size_t)j;
            pairs += akz_tv_bearing_pair_robust(a, a + 3, a + 6, b, b + 3, b + 6, st->robust_view_bearing_pair_minimum_cosine_distance) ? 1u : 0u;
        }
    stats[AKZ_TVC_S_USED] = used;
    stats[AKZ_TVC_S_PAIRS] = pairs;
    akz_tvc_put_f64(stats, AKZ_TVC_S_ORIGINAL_SCALE, akz_tvc_canonical(original_scale));
    stats[AKZ_TVC_S_STAGE] = AKZ_TVC_STAGE_PAIRS;
    if (pairs < st->robust_view_num_robust_bearing_pair) return AKZ_TVC_FEW_BEARING_PAIRS;
    akz_tvc_adaptive_optimize(rel, st->constraint_patience, lm9, used, sequential);
    const double final_scale = akz_tvc_scale_of(rel);
    const double relative_scale = original_scale / final_scale;
    akz_tv_pose_scale(rel, relative_scale);
    akz_tv_pose_scale(rel + 12, relative_scale);
    akz_tvc_put_f64(stats, AKZ_TVC_S_FINAL_SCALE, akz_tvc_canonical(final_scale));
    stats[AKZ_TVC_S_STAGE] = AKZ_TVC_STAGE_FINAL;
    for (int k = 0; k < 24; ++k) pose_out[k] = akz_tvc_canonical(rel[k]);
    return AKZ_TVC_OK;
}
#endif /* !__HIP_DEVICE_COMPILE__ */

#endif /* AKZ_THREE_VIEW_CONSTRAINT_MATH_H */
