/* akz_three_view_math.h — cv-sfm's three-view bootstrap (VSlam::init_reconstruction after its two consensuses) and the
 * L2 three-view optimiser it runs, written as plain IEEE double arithmetic so that gcc (the CPU checker,
 * tests/cpp/three_view_host.c) and hipcc (the gfx950 kernel of cv_amd/csrc/rs_three_view.hip) execute the same operation
 * sequence (build: -ffp-contract=off, no fast-math; sqrt is the one non-arithmetic primitive).  Parity is
 * "host build == HIP", bit for bit.  Built on akz_triangulate_math.h (the triangulator, from_homogeneous, the FloatOrd key,
 * calibrate) and akz_portable_math.h (the sine and cosine of the exponential map).
 *
 * Reference code restated here (paths relative to rust-cv/cv):
 *   two_view_same_space_triangulate_sine_l1, two_view_rotation_gradient,
 *   three_view_gradients, loss                          cv-geom/src/epipolar.rs:9-166, 197-233
 *   Se3TangentSpace::new / scale / isometry             cv-core/src/so3.rs:23-60, 78-82
 *   landmark_gradients, three_view_simple_optimize_l2   cv-optimize/src/three_view_optimizer.rs:7-21, 126-200
 *   Pose::scale, Pose::transform                        cv-core/src/pose.rs:37-41, 125-133
 *   Point3::from_homogeneous behind Projective::point   cv-core/src/point.rs:37-39
 *   is_bi_landmark_robust, is_tri_landmark_robust       cv-sfm/src/lib.rs:1306-1360
 *   init_reconstruction from the common matches on      cv-sfm/src/lib.rs:1002-1300
 *
 * Unpinned against the reference (nalgebra 0.30 is not vendored in the reference tree):
 *   - Rotation3::from_scaled_axis: Rodrigues' formula in nalgebra's from_axis_angle arrangement, with the sine and cosine
 *     of akz_portable_math.h (akz_pm_reduce, akz_pm_sin_poly, akz_pm_cos_poly) instead of the host libm's.  A zero or NaN
 *     angle gives the identity (Unit::try_new refuses the axis); an infinite angle or one of 2^20 and more, which the
 *     reduction does not cover, gives a matrix of NaN (what sin(inf) gives the reference);
 *   - the eigen-solver and the product orders of akz_triangulate_math.h's own list;
 *   - the order of nalgebra's products, cross products and norms: fixed below, every three-term sum ((x0 + x1) + x2);
 *   - THE ORDER OF THE SUM OVER LANDMARKS: akz_sum_order.h, a workgroup's; thread t's partial is the 12 gradient components of
 *     landmarks t, t + 256, ...  akz_tv_sum_tree below executes it on the host; akz_tv_sum_sequential is the reference's
 *     order, kept for the test that documents what the choice costs.
 *
 * A finding: three_view_gradients hands two_view_same_space_triangulate_sine_l1 the NEGATED translations
 * (epipolar.rs:118, 128, 139), while that function's w = |z|^2 / z.(t x b) is the inverse depth along `a` for t = the
 * position of B's centre in A's axes, which is the translation itself.  With the negated one w < 0 for every point in
 * front of both cameras; from_homogeneous (point.rs:20-25) then negates the vector, its bearing is -a, and the cheirality
 * filter of epipolar.rs:48-51 drops it.  So on a well-posed scene all three translation gradients are zero and only the
 * rotations move (the translations are carried along by delta.isometry() * pose).  This header does what the text does.
 */
#ifndef AKZ_THREE_VIEW_MATH_H
#define AKZ_THREE_VIEW_MATH_H

#include "akz_portable_math.h"
#include "akz_sum_order.h"
#include "akz_triangulate_math.h"

enum { AKZ_TV_THREADS = AKZ_SUM_THREADS, AKZ_TV_WAVE = AKZ_SUM_WAVE, AKZ_TV_MAX_LANDMARKS = 1024, AKZ_TV_MAX_RUNS = 9, AKZ_TV_NO_IMPROVE = 50 };

/* verdicts (RS_TV_* of include/akz.h) */
enum {
    AKZ_TV_OK = 0,
    AKZ_TV_FEW_SCALES = 1,         /* lib.rs:1039: continue */
    AKZ_TV_FEW_BEARING_PAIRS = 2,  /* lib.rs:1100: return None, the whole search ends */
    AKZ_TV_FEW_MATCHES = 3,        /* lib.rs:1118, 1167: continue */
    AKZ_TV_LOST_HALF = 4,          /* lib.rs:1126, 1175, 1281: continue */
    AKZ_TV_FEW_ROBUST = 5,         /* lib.rs:1286: continue */
    AKZ_TV_BAD_INDEX = 6
};
/* the stage a verdict was reached at (stats word AKZ_TV_S_STAGE) */
enum { AKZ_TV_STAGE_INDEX = 0, AKZ_TV_STAGE_SCALES = 1, AKZ_TV_STAGE_PAIRS = 2, AKZ_TV_STAGE_RUN0 = 3 /* + run */, AKZ_TV_STAGE_FINAL = 12 };
/* stats words (u32) */
enum {
    AKZ_TV_S_SCALES = 0,       /* relative scales found (lib.rs:1039) */
    AKZ_TV_S_MEDIAN_LO = 1,    /* median_scale (after the sqrt), the bits of its f64, low word first; 0 when not reached */
    AKZ_TV_S_MEDIAN_HI = 2,
    AKZ_TV_S_PAIRS = 3,        /* robust bearing pairs (lib.rs:1085-1096) */
    AKZ_TV_S_RUN_MATCHES = 4,  /* [9] optimisation matches entering run r; 0xFFFFFFFF for a run not reached */
    AKZ_TV_S_RUN_STOP = 13,    /* [9] the `iteration` run r left its loop at; 0xFFFFFFFF for a run not made */
    AKZ_TV_S_ROBUST = 22,      /* num_robust_matches (lib.rs:1248-1268) */
    AKZ_TV_S_STAGE = 23,
    AKZ_TV_STATS = 24
};

typedef struct akz_tv_settings {
    double maximum_cosine_distance;                               /* 1e-5 */
    double maximum_sine_distance;                                 /* 1e-1 */
    double robust_observation_incidence_minimum_cosine_distance;  /* 1e-3 */
    double robust_view_bearing_pair_minimum_cosine_distance;      /* 1e-2 */
    double optimization_rate;                                     /* the literal 0.001 of lib.rs:1133, 1182 */
    unsigned robust_view_num_robust_bearing_pair;                 /* 3 */
    unsigned three_view_minimum_relative_scales;                  /* 16 */
    unsigned three_view_filter_loop_iterations;                   /* 8 (<= AKZ_TV_MAX_RUNS - 1) */
    unsigned three_view_optimization_landmarks;                   /* 1024 (<= AKZ_TV_MAX_LANDMARKS) */
    unsigned three_view_patience;                                 /* 65536: the optimiser's `iterations` */
    unsigned three_view_minimum_robust_matches;                   /* 32 */
    unsigned hard_minimum_matches;                                /* the literal 32 of lib.rs:1118, 1167 */
    akz_tri_settings tri;
} akz_tv_settings;

/* ---- small vectors: every sum ((x0 + x1) + x2) ---- */
AKZ_RM_FN double akz_tv_dot(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
AKZ_RM_FN void akz_tv_cross(const double* a, const double* b, double* o)
{
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}
AKZ_RM_FN double akz_tv_norm(const double* a) { return AKZ_RM_SQRT(akz_tv_dot(a, a)); }
/* M v for the rotation of a row-major [R | t] (stride 4) */
AKZ_RM_FN void akz_tv_rotate(const double* pose, const double* v, double* o)
{
    AKZ_RM_UNROLL
    for (int i = 0; i < 3; ++i) o[i] = (pose[i * 4] * v[0] + pose[i * 4 + 1] * v[1]) + pose[i * 4 + 2] * v[2];
}
AKZ_RM_FN int akz_tv_any_nan(const double* v) { return v[0] != v[0] || v[1] != v[1] || v[2] != v[2]; }

/* Isometry3::inverse (nalgebra): R^T, and R^T applied to the negated translation */
AKZ_RM_FN void akz_tv_pose_inverse(const double* p, double* o)
{
    const double nt[3] = {-p[3], -p[7], -p[11]};
    AKZ_RM_UNROLL
    for (int i = 0; i < 3; ++i) {
        o[i * 4] = p[i]; o[i * 4 + 1] = p[4 + i]; o[i * 4 + 2] = p[8 + i];
        o[i * 4 + 3] = (p[i] * nt[0] + p[4 + i] * nt[1]) + p[8 + i] * nt[2];
    }
}

/* two_view_rotation_gradient (epipolar.rs:56-71) */
AKZ_RM_FN void akz_tv_rotation_gradient(const double* t, const double* a, const double* b, double* o)
{
    double ca[3], cb[3];
    akz_tv_cross(a, t, ca);
    akz_tv_cross(b, t, cb);
    const double na = akz_tv_norm(ca), nb = akz_tv_norm(cb);
    const double ua[3] = {ca[0] / na, ca[1] / na, ca[2] / na}, ub[3] = {cb[0] / nb, cb[1] / nb, cb[2] / nb};
    akz_tv_cross(ub, ua, o);
}

/* two_view_same_space_triangulate_sine_l1 (epipolar.rs:9-53): 1 and the point with A as the origin, or 0 ("None"). */
AKZ_RM_FN int akz_tv_triangulate_sine_l1(const double* t, const double* a_in, const double* b_in, double* point)
{
    double ca[3], cb[3], a[3], b[3], z[3], tb[3], p[4];
    akz_tv_cross(a_in, t, ca);
    const double can = akz_tv_norm(ca);
    akz_tv_cross(b_in, t, cb);
    const double cbn = akz_tv_norm(cb);
    if (can < cbn) {
        const double nb[3] = {cb[0] / cbn, cb[1] / cbn, cb[2] / cbn};
        const double d = akz_tv_dot(a_in, nb);
        const double v[3] = {a_in[0] - d * nb[0], a_in[1] - d * nb[1], a_in[2] - d * nb[2]};
        const double n = akz_tv_norm(v);
        a[0] = v[0] / n; a[1] = v[1] / n; a[2] = v[2] / n;
        b[0] = b_in[0]; b[1] = b_in[1]; b[2] = b_in[2];
    } else {
        const double na[3] = {ca[0] / can, ca[1] / can, ca[2] / can};
        const double d = akz_tv_dot(b_in, na);
        const double v[3] = {b_in[0] - d * na[0], b_in[1] - d * na[1], b_in[2] - d * na[2]};
        const double n = akz_tv_norm(v);
        b[0] = v[0] / n; b[1] = v[1] / n; b[2] = v[2] / n;
        a[0] = a_in[0]; a[1] = a_in[1]; a[2] = a_in[2];
    }
    akz_tv_cross(a, b, z);
    akz_tv_cross(t, b, tb);
    p[0] = a[0]; p[1] = a[1]; p[2] = a[2];
    p[3] = akz_tv_dot(z, z) / akz_tv_dot(z, tb);
    akz_tri_from_homogeneous(p);
    if (!(AKZ_TRI_FINITE(p[0]) && AKZ_TRI_FINITE(p[1]) && AKZ_TRI_FINITE(p[2]) && AKZ_TRI_FINITE(p[3]))) return 0;
    if (__builtin_signbit(akz_tv_dot(p, a)) || __builtin_signbit(akz_tv_dot(p, b))) return 0;
    if (p[3] == 0.0) return 0;                          /* Point3::from_homogeneous */
    point[0] = p[0] / p[3]; point[1] = p[1] / p[3]; point[2] = p[2] / p[3];
    return 1;
}

/* three_view_gradients (epipolar.rs:85-166) behind Se3TangentSpace::new (so3.rs:23-34: a vector with a NaN in ANY
 * component becomes the zero vector, each of the four vectors on its own).
 * g = {first translation, first rotation, second translation, second rotation}. */
AKZ_RM_FN void akz_tv_three_view_gradients(const double* c, const double* f, const double* ftoc, const double* s, const double* stoc,
                                           double* g)
{
    const double stof[3] = {stoc[0] - ftoc[0], stoc[1] - ftoc[1], stoc[2] - ftoc[2]};
    double rot_cf[3], rot_cs[3], rot_fs[3], p[3], trans_f[3] = {0.0, 0.0, 0.0}, trans_s[3] = {0.0, 0.0, 0.0}, trans_c[3] = {0.0, 0.0, 0.0};
    akz_tv_rotation_gradient(ftoc, c, f, rot_cf);
    akz_tv_rotation_gradient(stoc, c, s, rot_cs);
    akz_tv_rotation_gradient(stof, f, s, rot_fs);
    const double two3 = 2.0 / 3.0, one3 = 1.0 / 3.0;
    const double nstoc[3] = {-stoc[0], -stoc[1], -stoc[2]}, nftoc[3] = {-ftoc[0], -ftoc[1], -ftoc[2]}, nstof[3] = {-stof[0], -stof[1], -stof[2]};
    if (akz_tv_triangulate_sine_l1(nstoc, c, s, p)) {
        const double q[3] = {p[0] - ftoc[0], p[1] - ftoc[1], p[2] - ftoc[2]};
        const double d = akz_tv_dot(q, f);
        AKZ_RM_UNROLL
        for (int k = 0; k < 3; ++k) trans_f[k] = q[k] - d * f[k];
    }
    if (akz_tv_triangulate_sine_l1(nftoc, c, f, p)) {
        const double q[3] = {p[0] - stoc[0], p[1] - stoc[1], p[2] - stoc[2]};
        const double d = akz_tv_dot(q, s);
        AKZ_RM_UNROLL
        for (int k = 0; k < 3; ++k) trans_s[k] = q[k] - d * s[k];
    }
    if (akz_tv_triangulate_sine_l1(nstof, f, s, p)) {
        const double q[3] = {p[0] + ftoc[0], p[1] + ftoc[1], p[2] + ftoc[2]};
        const double d = akz_tv_dot(q, c);
        AKZ_RM_UNROLL
        for (int k = 0; k < 3; ++k) trans_c[k] = d * c[k] - q[k];
    }
    AKZ_RM_UNROLL
    for (int k = 0; k < 3; ++k) {
        g[k] = trans_f[k] * two3 + trans_c[k] * one3;
        g[3 + k] = rot_cf[k] * two3 + (-rot_fs[k]) * one3;
        g[6 + k] = trans_s[k] * two3 + trans_c[k] * one3;
        g[9 + k] = rot_cs[k] * two3 + rot_fs[k] * one3;
    }
    AKZ_RM_UNROLL
    for (int v = 0; v < 4; ++v) {
        if (akz_tv_any_nan(g + 3 * v)) {
            g[3 * v] = 0.0; g[3 * v + 1] = 0.0; g[3 * v + 2] = 0.0;
        }
    }
}

/* landmark_gradients (three_view_optimizer.rs:7-21): inv = the two inverted poses {ftoc, stoc}, [2][12] */
AKZ_RM_FN void akz_tv_landmark_gradients(const double* inv, const double* c, const double* f, const double* s, double* g)
{
    double fc[3], sc[3];
    akz_tv_rotate(inv, f, fc);
    akz_tv_rotate(inv + 12, s, sc);
    const double ftoc[3] = {inv[3], inv[7], inv[11]}, stoc[3] = {inv[15], inv[19], inv[23]};
    akz_tv_three_view_gradients(c, fc, ftoc, sc, stoc, g);
}

/* Rotation3::from_scaled_axis (unpinned, see the head of this file), r row-major [9] */
AKZ_RM_FN void akz_tv_from_scaled_axis(const double* w, double* r)
{
    const double theta = akz_tv_norm(w);
    if (!(theta > 0.0)) {
        AKZ_RM_UNROLL
        for (int k = 0; k < 9; ++k) r[k] = (k == 0 || k == 4 || k == 8) ? 1.0 : 0.0;
        return;
    }
    if (!(theta < 1048576.0)) {
        const double nan = theta - theta == 0.0 ? (theta - theta) / (theta - theta) : theta - theta;
        AKZ_RM_UNROLL
        for (int k = 0; k < 9; ++k) r[k] = nan;
        return;
    }
    int q;
    const double red = akz_pm_reduce(theta, &q);
    const double sp = akz_pm_sin_poly(red), cp = akz_pm_cos_poly(red);
    double sn = (q & 1) ? cp : sp, cs = (q & 1) ? sp : cp;
    if (q & 2) sn = -sn;
    if ((q + 1) & 2) cs = -cs;
    const double ux = w[0] / theta, uy = w[1] / theta, uz = w[2] / theta, omc = 1.0 - cs;
    r[0] = (ux * ux) * omc + cs;      r[1] = (ux * uy) * omc - uz * sn; r[2] = (ux * uz) * omc + uy * sn;
    r[3] = (ux * uy) * omc + uz * sn; r[4] = (uy * uy) * omc + cs;      r[5] = (uy * uz) * omc - ux * sn;
    r[6] = (ux * uz) * omc - uy * sn; r[7] = (uy * uz) * omc + ux * sn; r[8] = (uz * uz) * omc + cs;
}

/* pose = delta.isometry() * pose (so3.rs:57-60, three_view_optimizer.rs:188): R_d = exp(rotation), t_d = R_d translation;
 * the product of two isometries is {t_d + R_d t, R_d R}. */
AKZ_RM_FN void akz_tv_apply_delta(const double* delta, double* pose)
{
    double r[9], o[12];
    akz_tv_from_scaled_axis(delta + 3, r);
    AKZ_RM_UNROLL
    for (int i = 0; i < 3; ++i) {
        const double td = (r[i * 3] * delta[0] + r[i * 3 + 1] * delta[1]) + r[i * 3 + 2] * delta[2];
        AKZ_RM_UNROLL
        for (int j = 0; j < 3; ++j) o[i * 4 + j] = (r[i * 3] * pose[j] + r[i * 3 + 1] * pose[4 + j]) + r[i * 3 + 2] * pose[8 + j];
        o[i * 4 + 3] = td + ((r[i * 3] * pose[3] + r[i * 3 + 1] * pose[7]) + r[i * 3 + 2] * pose[11]);
    }
    AKZ_RM_UNROLL
    for (int k = 0; k < 12; ++k) pose[k] = o[k];
}

/* The state of one optimiser run between iterations (three_view_optimizer.rs:137-138). */
typedef struct akz_tv_opt_state {
    double best[4];   /* {best_t, best_r} of the first pose, then of the second */
    unsigned no_improve_for;
} akz_tv_opt_state;
AKZ_RM_FN void akz_tv_opt_begin(akz_tv_opt_state* st)
{
    const double inf = __builtin_inf();
    st->best[0] = inf; st->best[1] = inf; st->best[2] = inf; st->best[3] = inf;
    st->no_improve_for = 0;
}
/* One iteration after the sum (three_view_optimizer.rs:150-197): nets [12] the summed gradients, scale = inv_landmark_len *
 * optimization_rate, inv [2][12] the inverted poses.  The comparisons are strict (best > norm), a NaN norm never improves.
 * Returns 0 to go on, 1 for the no-improvement break (taken BEFORE the poses move), 2 for the last-iteration break (after). */
AKZ_RM_FN int akz_tv_opt_step(akz_tv_opt_state* st, const double* nets, double scale, double* inv, unsigned iteration, unsigned iterations)
{
    double deltas[12];
    AKZ_RM_UNROLL
    for (int k = 0; k < 12; ++k) deltas[k] = nets[k] * scale;
    st->no_improve_for += 1;
    AKZ_RM_UNROLL
    for (int p = 0; p < 2; ++p) {
        const double t = akz_tv_norm(nets + 6 * p), r = akz_tv_norm(nets + 6 * p + 3);
        if (st->best[2 * p] > t) {
            st->best[2 * p] = t;
            st->no_improve_for = 0;
        }
        if (st->best[2 * p + 1] > r) {
            st->best[2 * p + 1] = r;
            st->no_improve_for = 0;
        }
    }
    if (st->no_improve_for >= (unsigned)AKZ_TV_NO_IMPROVE) return 1;
    akz_tv_apply_delta(deltas, inv);
    akz_tv_apply_delta(deltas + 6, inv + 12);
    if (iteration == iterations - 1u) return 2;
    return 0;
}

/* ---- classification ---- */
/* the three observations of a common match as akz_tri_* wants them: (identity, c), (first, f), (second, s) */
typedef struct akz_tv_obs {
    const double* c; const double* f; const double* s;
    const double* first; const double* second;   /* CameraToCamera [12] */
} akz_tv_obs;
AKZ_RM_FN int akz_tv_obs_fetch(const akz_tv_obs* o, unsigned i, double* pose, double* b)
{
    const double* src = i == 0 ? o->c : (i == 1 ? o->f : o->s);
    const double* p = i == 1 ? o->first : o->second;
    AKZ_RM_UNROLL
    for (int k = 0; k < 12; ++k) pose[k] = i == 0 ? ((k == 0 || k == 5 || k == 10) ? 1.0 : 0.0) : p[k];
    b[0] = src[0]; b[1] = src[1]; b[2] = src[2];
    return 1;
}
AKZ_TRI_DEFINE_TRIANGULATE(akz_tv_tri_obs, akz_tv_obs, akz_tv_obs_fetch)
/* the two observations of triangulate_relative(pose, a, b): o->c = a, o->s = b, o->second = pose */
AKZ_RM_FN int akz_tv_rel_fetch(const akz_tv_obs* o, unsigned i, double* pose, double* b) { return akz_tv_obs_fetch(o, i == 0 ? 0u : 2u, pose, b); }
AKZ_TRI_DEFINE_TRIANGULATE(akz_tv_tri_rel, akz_tv_obs, akz_tv_rel_fetch)

/* 1 - bearing(pose.transform(point)) . b (pose.rs:125-133): M p = {R xyz + t w, w}, then from_homogeneous */
AKZ_RM_FN double akz_tv_transformed_distance(const double* pose, const double* point, const double* b)
{
    double q[4];
    AKZ_RM_UNROLL
    for (int i = 0; i < 3; ++i)
        q[i] = ((pose[i * 4] * point[0] + pose[i * 4 + 1] * point[1]) + pose[i * 4 + 2] * point[2]) + pose[i * 4 + 3] * point[3];
    q[3] = point[3];
    akz_tri_from_homogeneous(q);
    return 1.0 - akz_tv_dot(q, b);
}

/* is_tri_landmark_robust (lib.rs:1320-1360).  triangulate_observations_to_camera passes the WorldPoint through
 * CameraPoint::from_homogeneous once more (cv-core/src/triangulation.rs:35). */
AKZ_RM_FN int akz_tv_tri_landmark_robust(const double* first, const double* second, const double* c, const double* f, const double* s,
                                         double maximum_cosine_distance, double incidence_minimum_cosine_distance, const akz_tri_settings* tri)
{
    akz_tv_obs o;
    o.c = c; o.f = f; o.s = s; o.first = first; o.second = second;
    double p[4], fc[3], sc[3];
    if (akz_tv_tri_obs(&o, 3u, 0, tri, p) != AKZ_TRI_OK) return 0;
    akz_tri_from_homogeneous(p);
    akz_tri_world_bearing(first, f, fc);
    akz_tri_world_bearing(second, s, sc);
    const int cosine = 1.0 - akz_tv_dot(p, c) < maximum_cosine_distance &&
                       akz_tv_transformed_distance(first, p, f) < maximum_cosine_distance &&
                       akz_tv_transformed_distance(second, p, s) < maximum_cosine_distance;
    const int incidence = akz_tri_pair_robust(c, fc, incidence_minimum_cosine_distance) ||
                          akz_tri_pair_robust(c, sc, incidence_minimum_cosine_distance) ||
                          akz_tri_pair_robust(fc, sc, incidence_minimum_cosine_distance);
    return cosine && incidence;
}

/* epipolar::loss (epipolar.rs:197-233) */
AKZ_RM_FN double akz_tv_loss(const double* t, const double* a, const double* b)
{
    double ca[3], cb[3], residual;
    akz_tv_cross(a, t, ca);
    const double can2 = akz_tv_dot(ca, ca);
    akz_tv_cross(b, t, cb);
    const double cbn2 = akz_tv_dot(cb, cb);
    if (can2 < cbn2) {
        const double k = 1.0 / AKZ_RM_SQRT(cbn2);
        const double n[3] = {cb[0] * k, cb[1] * k, cb[2] * k};
        residual = akz_tv_dot(a, n);
    } else {
        const double k = 1.0 / AKZ_RM_SQRT(can2);
        const double n[3] = {ca[0] * k, ca[1] * k, ca[2] * k};
        residual = akz_tv_dot(b, n);
    }
    residual = residual < 0.0 ? -residual : residual;
    if (residual != residual || __builtin_signbit(akz_tv_dot(a, b))) return 1.0;
    return residual;
}
/* is_bi_landmark_robust (lib.rs:1306-1317) */
AKZ_RM_FN int akz_tv_bi_landmark_robust(const double* pose, const double* a, const double* b, double maximum_sine_distance)
{
    double ra[3];
    akz_tv_rotate(pose, a, ra);
    const double t[3] = {pose[3], pose[7], pose[11]};
    return akz_tv_loss(t, ra, b) < maximum_sine_distance;
}

/* The squared depth ratio of one common match (lib.rs:1011-1036), 1 and *ratio, or 0 ("None"). */
AKZ_RM_FN int akz_tv_relative_scale(const double* first, const double* second, const double* c, const double* f, const double* s,
                                    const akz_tv_settings* st, double* ratio)
{
    if (!akz_tv_tri_landmark_robust(first, second, c, f, s, 1.0, st->robust_observation_incidence_minimum_cosine_distance, &st->tri)) return 0;
    akz_tv_obs o;
    double p[4];
    o.c = c; o.f = f; o.s = f; o.first = first; o.second = first;
    if (akz_tv_tri_rel(&o, 2u, 0, &st->tri, p) != AKZ_TRI_OK) return 0;
    akz_tri_from_homogeneous(p);
    if (p[3] == 0.0) return 0;
    const double fp[3] = {p[0] / p[3], p[1] / p[3], p[2] / p[3]};
    o.s = s; o.second = second;
    if (akz_tv_tri_rel(&o, 2u, 0, &st->tri, p) != AKZ_TRI_OK) return 0;
    akz_tri_from_homogeneous(p);
    if (p[3] == 0.0) return 0;
    const double sp[3] = {p[0] / p[3], p[1] / p[3], p[2] / p[3]};
    const double r = akz_tv_dot(fp, fp) / akz_tv_dot(sp, sp);
    /* f64::is_normal: not zero, subnormal, infinite or NaN */
    const double ar = r < 0.0 ? -r : r;
    if (!(ar >= 0x1p-1022) || !AKZ_TRI_FINITE(r)) return 0;
    *ratio = r;
    return 1;
}

/* the rank of key i among n keys, ties by position: the element a stable ascending sort puts at that place */
AKZ_RM_FN unsigned akz_tv_rank(const unsigned long long* keys, unsigned n, unsigned i)
{
    unsigned r = 0;
    const unsigned long long k = keys[i];
    for (unsigned j = 0; j < n; ++j) r += (keys[j] < k || (keys[j] == k && j < i)) ? 1u : 0u;
    return r;
}
AKZ_RM_FN double akz_tv_key_value(unsigned long long u)
{
    double x;
    u = (u >> 63) ? (u & 0x7FFFFFFFFFFFFFFFull) : ~u;
    __builtin_memcpy(&x, &u, sizeof x);
    return x;
}

/* a robust bearing pair (lib.rs:1088-1095): all three of 1 - a_k . b_k > minimum */
AKZ_RM_FN int akz_tv_bearing_pair_robust(const double* ca, const double* fa, const double* sa, const double* cb, const double* fb,
                                         const double* sb, double minimum)
{
    return 1.0 - akz_tv_dot(ca, cb) > minimum && 1.0 - akz_tv_dot(fa, fb) > minimum && 1.0 - akz_tv_dot(sa, sb) > minimum;
}

/* Pose::scale (pose.rs:37-41): the translation only */
AKZ_RM_FN void akz_tv_pose_scale(double* pose, double scale)
{
    pose[3] = pose[3] * scale; pose[7] = pose[7] * scale; pose[11] = pose[11] * scale;
}

/* ---- the host's execution of the whole procedure (the kernel restates the control flow with a workgroup) ---- */
#if !defined(__HIP_DEVICE_COMPILE__)
#define AKZ_TV_HOST_FN static inline

/* landmarks as the kernel keeps them: lm[k * AKZ_TV_MAX_LANDMARKS + i] = component k (c xyz, f xyz, s xyz) of landmark i */
AKZ_TV_HOST_FN void akz_tv_sum_tree(const double* inv, const double* lm, unsigned n, double* nets)
{
    double part[AKZ_TV_THREADS][12];
    for (unsigned t = 0; t < (unsigned)AKZ_TV_THREADS; ++t) {
        for (int k = 0; k < 12; ++k) part[t][k] = 0.0;
        for (unsigned i = t; i < n; i += (unsigned)AKZ_TV_THREADS) {
            double c[3], f[3], s[3], g[12];
            for (int k = 0; k < 3; ++k) {
                c[k] = lm[k * AKZ_TV_MAX_LANDMARKS + i];
                f[k] = lm[(3 + k) * AKZ_TV_MAX_LANDMARKS + i];
                s[k] = lm[(6 + k) * AKZ_TV_MAX_LANDMARKS + i];
            }
            akz_tv_landmark_gradients(inv, c, f, s, g);
            for (int k = 0; k < 12; ++k) part[t][k] = part[t][k] + g[k];
        }
    }
    akz_sum_block(&part[0][0], 12, nets);
}
AKZ_TV_HOST_FN void akz_tv_sum_sequential(const double* inv, const double* lm, unsigned n, double* nets)
{
    for (int k = 0; k < 12; ++k) nets[k] = 0.0;
    for (unsigned i = 0; i < n; ++i) {
        double c[3], f[3], s[3], g[12];
        for (int k = 0; k < 3; ++k) {
            c[k] = lm[k * AKZ_TV_MAX_LANDMARKS + i];
            f[k] = lm[(3 + k) * AKZ_TV_MAX_LANDMARKS + i];
            s[k] = lm[(6 + k) * AKZ_TV_MAX_LANDMARKS + i];
        }
        akz_tv_landmark_gradients(inv, c, f, s, g);
        for (int k = 0; k < 12; ++k) nets[k] += g[k];
    }
}

/* three_view_simple_optimize_l2 (three_view_optimizer.rs:126-200): poses [2][12] in and out; returns the `iteration` the
 * loop was left at (0 for iterations == 0 or no landmarks). */
AKZ_TV_HOST_FN unsigned akz_tv_optimize(double* poses, double rate, unsigned iterations, const double* lm, unsigned n, int sequential)
{
    double inv[24], nets[12];
    akz_tv_opt_state st;
    unsigned iteration = 0;
    if (n == 0) return 0;
    const double scale = (1.0 / (double)n) * rate;
    akz_tv_pose_inverse(poses, inv);
    akz_tv_pose_inverse(poses + 12, inv + 12);
    akz_tv_opt_begin(&st);
    for (; iteration < iterations; ++iteration) {
        if (sequential) akz_tv_sum_sequential(inv, lm, n, nets);
        else akz_tv_sum_tree(inv, lm, n, nets);
        if (akz_tv_opt_step(&st, nets, scale, inv, iteration, iterations)) break;
    }
    akz_tv_pose_inverse(inv, poses);
    akz_tv_pose_inverse(inv + 12, poses + 12);
    return iteration;
}

/* The first optimization_landmarks matches, in list order, that pass is_tri_landmark_robust (lib.rs:1064-1083, 1140-1159) */
AKZ_TV_HOST_FN unsigned akz_tv_take(const double* first, const double* second, const double* c, const double* f, const double* s, unsigned n,
                               double maximum_cosine_distance, const akz_tv_settings* st, double* lm)
{
    unsigned m = 0;
    for (unsigned i = 0; i < n && m < st->three_view_optimization_landmarks; ++i) {
        if (!akz_tv_tri_landmark_robust(first, second, c + 3 * i, f + 3 * i, s + 3 * i, maximum_cosine_distance,
                                        st->robust_observation_incidence_minimum_cosine_distance, &st->tri))
            continue;
        for (int k = 0; k < 3; ++k) {
            lm[k * AKZ_TV_MAX_LANDMARKS + m] = c[3 * i + k];
            lm[(3 + k) * AKZ_TV_MAX_LANDMARKS + m] = f[3 * i + k];
            lm[(6 + k) * AKZ_TV_MAX_LANDMARKS + m] = s[3 * i + k];
        }
        ++m;
    }
    return m;
}

/* One triple from its common matches on (lib.rs:1002-1300).  c, f, s [n][3] the bearings of the common matches in the
 * caller's order; first_c, first_f [n_first][3] and second_c, second_s [n_second][3] those of the matches only one pair
 * has; pose_in [2][12].  keys: scratch for n u64; lm: scratch for 9 * AKZ_TV_MAX_LANDMARKS doubles.  pose_out [2][12] and
 * the masks are written for AKZ_TV_OK only; stats [AKZ_TV_STATS] always. */
AKZ_TV_HOST_FN int akz_tv_init_triple(const double* pose_in, const double* c, const double* f, const double* s, unsigned n, const double* first_c,
                                 const double* first_f, unsigned n_first, const double* second_c, const double* second_s,
                                 unsigned n_second, const akz_tv_settings* st, int sequential, unsigned long long* keys, double* lm,
                                 double* pose_out, unsigned char* combined, unsigned char* first_ok, unsigned char* second_ok,
                                 unsigned* stats)
{
    double poses[24];
    unsigned n_scales = 0;
    for (int k = 0; k < AKZ_TV_STATS; ++k) stats[k] = 0u;
    for (int r = 0; r < 2 * AKZ_TV_MAX_RUNS; ++r) stats[AKZ_TV_S_RUN_MATCHES + r] = 0xFFFFFFFFu;
    for (int k = 0; k < 24; ++k) poses[k] = pose_in[k];
    for (unsigned i = 0; i < n; ++i) {
        double ratio;
        if (akz_tv_relative_scale(poses, poses + 12, c + 3 * i, f + 3 * i, s + 3 * i, st, &ratio)) keys[n_scales++] = akz_tri_float_ord(ratio);
    }
    stats[AKZ_TV_S_SCALES] = n_scales;
    stats[AKZ_TV_S_STAGE] = AKZ_TV_STAGE_SCALES;
    if (n_scales < st->three_view_minimum_relative_scales) return AKZ_TV_FEW_SCALES;
    double median = 0.0;
    for (unsigned i = 0; i < n_scales; ++i)
        if (akz_tv_rank(keys, n_scales, i) == n_scales / 2u) median = AKZ_RM_SQRT(akz_tv_key_value(keys[i]));
    {
        unsigned long long u;
        __builtin_memcpy(&u, &median, sizeof u);
        stats[AKZ_TV_S_MEDIAN_LO] = (unsigned)(u & 0xFFFFFFFFull);
        stats[AKZ_TV_S_MEDIAN_HI] = (unsigned)(u >> 32);
    }
    akz_tv_pose_scale(poses + 12, median);

    unsigned n_opt = akz_tv_take(poses, poses + 12, c, f, s, n, 1.0, st, lm);
    unsigned pairs = 0;
    for (unsigned i = 0; i < n_opt; ++i)
        for (unsigned j = i + 1; j < n_opt; ++j) {
            double a[9], b[9];
            for (int k = 0; k < 9; ++k) {
                a[k] = lm[k * AKZ_TV_MAX_LANDMARKS + i];
                b[k] = lm[k * AKZ_TV_MAX_LANDMARKS + j];
            }
            pairs += akz_tv_bearing_pair_robust(a, a + 3, a + 6, b, b + 3, b + 6, st->robust_view_bearing_pair_minimum_cosine_distance) ? 1u : 0u;
        }
    stats[AKZ_TV_S_PAIRS] = pairs;
    stats[AKZ_TV_S_STAGE] = AKZ_TV_STAGE_PAIRS;
    if (pairs < st->robust_view_num_robust_bearing_pair) return AKZ_TV_FEW_BEARING_PAIRS;

    const unsigned robust_minimum_matches = n_opt / 2u;
    for (unsigned run = 0; run <= st->three_view_filter_loop_iterations; ++run) {
        stats[AKZ_TV_S_STAGE] = AKZ_TV_STAGE_RUN0 + run;
        stats[AKZ_TV_S_RUN_MATCHES + run] = n_opt;
        if (n_opt < st->hard_minimum_matches) return AKZ_TV_FEW_MATCHES;
        if (n_opt <= robust_minimum_matches) return AKZ_TV_LOST_HALF;
        stats[AKZ_TV_S_RUN_STOP + run] = akz_tv_optimize(poses, st->optimization_rate, st->three_view_patience, lm, n_opt, sequential);
        if (run < st->three_view_filter_loop_iterations)
            n_opt = akz_tv_take(poses, poses + 12, c, f, s, n, st->maximum_cosine_distance, st, lm);
    }

    unsigned robust = 0;
    for (unsigned i = 0; i < n; ++i)
        robust += akz_tv_tri_landmark_robust(poses, poses + 12, c + 3 * i, f + 3 * i, s + 3 * i, st->maximum_cosine_distance,
                                             st->robust_observation_incidence_minimum_cosine_distance, &st->tri) ? 1u : 0u;
    stats[AKZ_TV_S_ROBUST] = robust;
    stats[AKZ_TV_S_STAGE] = AKZ_TV_STAGE_FINAL;
    if (robust <= robust_minimum_matches) return AKZ_TV_LOST_HALF;
    if (robust < st->three_view_minimum_robust_matches) return AKZ_TV_FEW_ROBUST;
    for (unsigned i = 0; i < n; ++i)
        combined[i] = (unsigned char)akz_tv_tri_landmark_robust(poses, poses + 12, c + 3 * i, f + 3 * i, s + 3 * i, st->maximum_cosine_distance,
                                                                0.0, &st->tri);
    for (unsigned i = 0; i < n_first; ++i)
        first_ok[i] = (unsigned char)akz_tv_bi_landmark_robust(poses, first_c + 3 * i, first_f + 3 * i, st->maximum_sine_distance);
    for (unsigned i = 0; i < n_second; ++i)
        second_ok[i] = (unsigned char)akz_tv_bi_landmark_robust(poses + 12, second_c + 3 * i, second_s + 3 * i, st->maximum_sine_distance);
    for (int k = 0; k < 24; ++k) pose_out[k] = poses[k];
    return AKZ_TV_OK;
}
#endif /* !__HIP_DEVICE_COMPILE__ */

#endif /* AKZ_THREE_VIEW_MATH_H */
