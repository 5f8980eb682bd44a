/* akz_pose_graph_math.h — the relaxation of cv-sfm's pose graph under its three-view constraints (VSlam::apply_constraints),
 * written as plain IEEE double arithmetic so that gcc (the CPU checker, tests/cpp/pose_graph_host.c) and hipcc (the gfx950
 * kernels of cv_amd/csrc/rs_pose_graph.hip) execute the same operation sequence (build: -ffp-contract=off, no fast-math; sqrt
 * is the one non-arithmetic primitive).  Parity is "host build == HIP", bit for bit.  Built on
 * akz_three_view_constraint_math.h, which this file leaves as it is: the product of two isometries (akz_tvc_pose_mul), the
 * inverse (akz_tv_pose_inverse), the exponential map (akz_tv_from_scaled_axis) and the canonical NaN (akz_tvc_canonical) are
 * that header's and the one below it.
 *
 * Reference code restated here (paths relative to rust-cv/cv):
 *   ThreeViewConstraint::edge_constraints               cv-sfm/src/lib.rs:167-180
 *   VSlam::constrain_view                               cv-sfm/src/lib.rs:1892-1936
 *   apply_constraints / compute_momentum_bundle_adjust  cv-sfm/src/lib.rs:2358-2414
 *   flatten_constraints                                 cv-sfm/src/lib.rs:2519-2532
 *   apply_bundle_adjust                                 cv-sfm/src/lib.rs:502-515
 *   CameraToCamera::se3 / from_se3                      cv-core/src/pose.rs:54-66
 *   Skew3 from Rotation3                                cv-core/src/so3.rs:263-275
 *   optimization_iterations, graph_optimization_rate    cv-sfm/src/settings.rs:461-463, 477-479
 *
 * Unpinned against the reference (nalgebra 0.30 is not vendored in the reference tree):
 *   - THE LOG MAP.  Rotation3::scaled_axis is, from memory, axis * angle with
 *       angle = acos(clamp((trace - 1) / 2, -1, 1)),
 *       axis  = Unit::try_new((m32 - m23, m13 - m31, m21 - m12), f64::EPSILON)      (1-based, row then column),
 *     and the zero vector when try_new refuses.  try_new is taken as "squared norm > EPSILON * EPSILON, then every component
 *     divided by the square root of the squared norm".  The Skew3 conversion additionally replaces a vector holding a NaN by
 *     zero (so3.rs:268-272).  Exactly that text is akz_pg_log below.
 *   - the f64 acos: akz_pm_acos of akz_portable_math.h (+ - * / and sqrt; its distance to the host libm is measured there);
 *   - the exponential map: akz_tv_from_scaled_axis, as it is;
 *   - the product of isometries: akz_tvc_pose_mul, as it is; the inverse: akz_tv_pose_inverse;
 *   - the order of a view's edges: the reference walks the values of a HashMap and defines none; ours is the caller's row
 *     order;
 *   - THE ORDER OF THE SUM OVER A VIEW'S EDGES: akz_sum_order.h, one wave's per view; lane l's partial is the 6 se3 components
 *     of entries l, l + 64, ... of the view's row, an edge of a refused constraint adding nothing.  akz_pg_sum_wave executes
 *     it on the host; akz_pg_sum_sequential is the reference's order, kept for the test that documents what the choice costs.
 *   - the sign and payload of a NaN: every NaN written is the quiet NaN of akz_tvc_canonical.
 *
 * Findings: a rotation below about 1.5e-8 rad (acos(1 - 2^-53), the smallest angle acos can return; a cosine
 * rounds to 1.0 below 1.05e-8 rad) has (trace - 1) / 2 == 1.0, so its log is exactly zero and the relaxation has a floor —
 * clean only while the trace is exact: the rounding of the two products in front of the log can leave the trace an ulp
 * below 3, which reads as 1.5e-8 rad or more; and the reference panics in the round after a view with edges was removed
 * for a non-finite delta, so a graph stops here at the first such round.  The text is shipped as it is.
 */
#ifndef AKZ_POSE_GRAPH_MATH_H
#define AKZ_POSE_GRAPH_MATH_H

#include "akz_three_view_constraint_math.h"

enum { AKZ_PG_WAVE = AKZ_SUM_WAVE, AKZ_PG_RESIDENT_VIEWS = 256, AKZ_PG_MAX_ITERATIONS = 1 << 20 };

/* a graph's verdict (RS_PG_* of include/akz.h) */
enum {
    AKZ_PG_OK = 0,
    AKZ_PG_FEW_VIEWS = 1,    /* fewer than 3 views would be updated (lib.rs:2413) */
    AKZ_PG_NONFINITE = 2,    /* a view's net delta was not finite (lib.rs:1929) */
    AKZ_PG_BAD_INDEX = 3
};
/* a view's state (RS_PG_VIEW_*) */
enum { AKZ_PG_VIEW_UPDATED = 0, AKZ_PG_VIEW_NO_CONSTRAINT = 1 /* lib.rs:1900-1902 */, AKZ_PG_VIEW_NONFINITE = 2 };
/* the stage a verdict was reached at (stats word AKZ_PG_S_STAGE) */
enum { AKZ_PG_STAGE_INDEX = 0, AKZ_PG_STAGE_VIEWS = 1, AKZ_PG_STAGE_ROUNDS = 2 };
/* stats words (u32) of a graph; a word behind the stage the verdict fell at is 0 */
enum {
    AKZ_PG_S_VIEWS = 0,           /* the views the graph owns */
    AKZ_PG_S_UPDATED = 1,         /* those with an edge of an accepted constraint in their row */
    AKZ_PG_S_EDGES = 2,           /* row entries of accepted constraints, over all rows of the graph */
    AKZ_PG_S_ROUNDS = 3,          /* rounds run */
    AKZ_PG_S_STAGE = 4,
    AKZ_PG_S_FIRST_BAD_VIEW = 5,  /* the lowest view whose net was not finite; AKZ_PG_NO_VIEW when there is none */
    AKZ_PG_STATS = 8              /* words 6, 7: 0 */
};
#define AKZ_PG_NO_VIEW 0xFFFFFFFFu

typedef struct akz_pg_settings {
    double graph_optimization_rate;     /* 1e-3 */
    unsigned optimization_iterations;   /* 1024 (more than AKZ_PG_MAX_ITERATIONS count as that) */
} akz_pg_settings;

/* Edge slot s of a constraint: its target is the constraint's view T[s], its other view O[s], T = {0,0,1,1,2,2},
 * O = {2,1,0,2,1,0} (lib.rs:167-180). */
AKZ_RM_FN unsigned akz_pg_slot_target(unsigned slot) { return slot >> 1; }
AKZ_RM_FN unsigned akz_pg_slot_other(unsigned slot) { return 2u - slot % 3u; }

/* The six expected other-to-target isometries of a constraint, in slot order (lib.rs:167-180): pose2 [2][12] = {first,
 * second}, edges [6][12] = {second^-1, first^-1, first, (second first^-1)^-1, second first^-1, second}. */
AKZ_RM_FN void akz_pg_constraint_edges(const double* pose2, double* edges)
{
    double fi[12], f2s[12];
    akz_tv_pose_inverse(pose2, fi);
    akz_tvc_pose_mul(pose2 + 12, fi, f2s);
    akz_tv_pose_inverse(pose2 + 12, edges);
    akz_tv_pose_inverse(f2s, edges + 36);
    AKZ_RM_UNROLL
    for (int k = 0; k < 12; ++k) {
        edges[12 + k] = fi[k];
        edges[24 + k] = pose2[k];
        edges[48 + k] = f2s[k];
        edges[60 + k] = pose2[12 + k];
    }
    AKZ_RM_UNROLL
    for (int k = 0; k < 72; ++k) edges[k] = akz_tvc_canonical(edges[k]);
}

/* Skew3::from(Rotation3) (so3.rs:263-275) over Rotation3::scaled_axis (unpinned, see the head of this file): the rotation
 * of a row-major [R | t] (stride 4) -> w [3]. */
AKZ_RM_FN void akz_pg_log(const double* pose, double* w)
{
    const double eps = 0x1p-52;   /* f64::EPSILON */
    double c = (((pose[0] + pose[5]) + pose[10]) - 1.0) / 2.0;
    const double v[3] = {pose[9] - pose[6], pose[2] - pose[8], pose[4] - pose[1]};
    if (c < -1.0) c = -1.0;
    if (c > 1.0) c = 1.0;
    const double angle = akz_pm_acos(c);
    const double sq = akz_tv_dot(v, v);
    w[0] = 0.0; w[1] = 0.0; w[2] = 0.0;
    if (sq > eps * eps) {
        const double n = AKZ_RM_SQRT(sq);
        const double u[3] = {(v[0] / n) * angle, (v[1] / n) * angle, (v[2] / n) * angle};
        if (!akz_tv_any_nan(u)) { w[0] = u[0]; w[1] = u[1]; w[2] = u[2]; }
    }
}

/* CameraToCamera::se3 (pose.rs:54-59): the translation, then the Skew3 of the rotation */
AKZ_RM_FN void akz_pg_se3(const double* delta, double* se3)
{
    se3[0] = delta[3]; se3[1] = delta[7]; se3[2] = delta[11];
    akz_pg_log(delta, se3 + 3);
}

/* What one edge adds to its view's sum (lib.rs:1915-1925): se3((expected * world_to_other) * view_to_world) */
AKZ_RM_FN void akz_pg_edge_se3(const double* expected, const double* world_to_other, const double* view_to_world, double* se3)
{
    double eo[12], delta[12];
    akz_tvc_pose_mul(expected, world_to_other, eo);
    akz_tvc_pose_mul(eo, view_to_world, delta);
    akz_pg_se3(delta, se3);
}

/* CameraToCamera::from_se3(net) * pose (pose.rs:62-66, lib.rs:1933-1934): from_se3 is from_parts(translation,
 * exp(rotation)) — the translation is NOT rotated (Se3TangentSpace::isometry, akz_tv_apply_delta, rotates it). */
AKZ_RM_FN void akz_pg_from_se3_mul(const double* net, const double* pose, double* out)
{
    double r[9], d[12];
    akz_tv_from_scaled_axis(net + 3, r);
    AKZ_RM_UNROLL
    for (int i = 0; i < 3; ++i) {
        d[i * 4] = r[i * 3]; d[i * 4 + 1] = r[i * 3 + 1]; d[i * 4 + 2] = r[i * 3 + 2];
        d[i * 4 + 3] = net[i];
    }
    akz_tvc_pose_mul(d, pose, out);
}

/* One view's update from the sum of its edges' se3 (lib.rs:1926-1935): 1 and the new pose in out, or 0 (a component of
 * sum * rate is not finite) and out = pose.  out may not alias pose. */
AKZ_RM_FN int akz_pg_view_update(const double* sum6, double rate, const double* pose, double* out)
{
    double net[6];
    int finite = 1;
    AKZ_RM_UNROLL
    for (int k = 0; k < 6; ++k) {
        net[k] = sum6[k] * rate;
        finite &= AKZ_TRI_FINITE(net[k]) ? 1 : 0;
    }
    if (!finite) {
        AKZ_RM_UNROLL
        for (int k = 0; k < 12; ++k) out[k] = pose[k];
        return 0;
    }
    akz_pg_from_se3_mul(net, pose, out);
    AKZ_RM_UNROLL
    for (int k = 0; k < 12; ++k) out[k] = akz_tvc_canonical(out[k]);
    return 1;
}

/* The index test of one row entry of view v in a graph that owns views [gs, ge): 0 the entry is of a refused constraint
 * (skipped through its verdict, not its contents), 1 an edge to add, -1 a bad index.  *other: the edge's other view. */
AKZ_RM_FN int akz_pg_entry(unsigned entry, unsigned v, unsigned gs, unsigned ge, const unsigned* views, const unsigned* cverdict,
                           unsigned n_constraints, unsigned* other)
{
    if (entry / 6u >= n_constraints) return -1;
    const unsigned c = entry / 6u, slot = entry % 6u;
    if (cverdict[c] != (unsigned)AKZ_TVC_OK) return 0;
    const unsigned t = views[3 * (size_t)c + akz_pg_slot_target(slot)], o = views[3 * (size_t)c + akz_pg_slot_other(slot)];
    if (t != v || o < gs || o >= ge) return -1;
    *other = o;
    return 1;
}

/* ---- the host's execution of the whole procedure (the kernels restate the control flow with one wavefront per view) ---- */
#if !defined(__HIP_DEVICE_COMPILE__)
#define AKZ_PG_HOST_FN static inline

/* the sum of a view's edges: row [n] entries that passed akz_pg_entry, `cur` the pose table of the round before */
AKZ_PG_HOST_FN void akz_pg_sum_wave(const double* cur, unsigned v, const unsigned* row, unsigned n, const unsigned* views,
                                    const unsigned* cverdict, const double* edges, double* sum6)
{
    double part[AKZ_PG_WAVE][6], inv[12], q[6];
    akz_tv_pose_inverse(cur + 12 * (size_t)v, inv);
    for (unsigned l = 0; l < (unsigned)AKZ_PG_WAVE; ++l) {
        for (int k = 0; k < 6; ++k) part[l][k] = 0.0;
        for (unsigned i = l; i < n; i += (unsigned)AKZ_PG_WAVE) {
            const unsigned c = row[i] / 6u;
            if (cverdict[c] != (unsigned)AKZ_TVC_OK) continue;   /* + 0.0 leaves a sum that began at + 0.0 as it is */
            const unsigned o = views[3 * (size_t)c + akz_pg_slot_other(row[i] % 6u)];
            akz_pg_edge_se3(edges + 12 * (size_t)row[i], cur + 12 * (size_t)o, inv, q);
            for (int k = 0; k < 6; ++k) part[l][k] = part[l][k] + q[k];
        }
    }
    for (int k = 0; k < 6; ++k) sum6[k] = akz_sum_wave(&part[0][k], 6);
}
AKZ_PG_HOST_FN void akz_pg_sum_sequential(const double* cur, unsigned v, const unsigned* row, unsigned n, const unsigned* views,
                                          const unsigned* cverdict, const double* edges, double* sum6)
{
    double inv[12], q[6];
    akz_tv_pose_inverse(cur + 12 * (size_t)v, inv);
    for (int k = 0; k < 6; ++k) sum6[k] = 0.0;
    for (unsigned i = 0; i < n; ++i) {
        const unsigned c = row[i] / 6u;
        if (cverdict[c] != (unsigned)AKZ_TVC_OK) continue;
        const unsigned o = views[3 * (size_t)c + akz_pg_slot_other(row[i] % 6u)];
        akz_pg_edge_se3(edges + 12 * (size_t)row[i], cur + 12 * (size_t)o, inv, q);
        for (int k = 0; k < 6; ++k) sum6[k] = sum6[k] + q[k];
    }
}

/* apply_constraints (lib.rs:2358-2375) for graph g of a batch: poses [n_views][12] in and out, scratch [n_views][12] the
 * second table of the Jacobi sweep.  graph_verdict [g], stats [g][AKZ_PG_STATS]: always written; view_state [n_views] and
 * the poses: the graph's views only, and not for AKZ_PG_BAD_INDEX. */
AKZ_PG_HOST_FN void akz_pg_relax_graph(double* poses, double* scratch, unsigned n_views, const unsigned* graph_start, unsigned g,
                                       const unsigned* row_start, const unsigned* row_edges, unsigned n_rows, const unsigned* views,
                                       const unsigned* cverdict, const double* edges, unsigned n_constraints, const akz_pg_settings* st,
                                       int sequential, unsigned* graph_verdict, unsigned* view_state, unsigned* stats_all)
{
    unsigned* stats = stats_all + (size_t)AKZ_PG_STATS * g;
    const unsigned gs = graph_start[g], ge = graph_start[g + 1];
    unsigned iterations = st->optimization_iterations, other = 0, updated = 0, n_edges = 0;
    if (iterations > (unsigned)AKZ_PG_MAX_ITERATIONS) iterations = (unsigned)AKZ_PG_MAX_ITERATIONS;
    for (int k = 0; k < AKZ_PG_STATS; ++k) stats[k] = 0u;
    stats[AKZ_PG_S_FIRST_BAD_VIEW] = AKZ_PG_NO_VIEW;
    graph_verdict[g] = AKZ_PG_BAD_INDEX;
    /* ---- nothing is read through an index before every index of the graph has been looked at ---- */
    for (unsigned k = 0; k < g; ++k)
        if (graph_start[k] > gs) return;          /* the start array does not ascend up to this graph */
    if (gs > ge || ge > n_views) return;
    for (unsigned v = gs; v < ge; ++v) {
        if (row_start[v] > row_start[v + 1] || row_start[v + 1] > n_rows) return;
        for (unsigned i = row_start[v]; i < row_start[v + 1]; ++i)
            if (akz_pg_entry(row_edges[i], v, gs, ge, views, cverdict, n_constraints, &other) < 0) return;
    }
    for (unsigned v = gs; v < ge; ++v) {
        unsigned has = 0;
        for (unsigned i = row_start[v]; i < row_start[v + 1]; ++i) has += akz_pg_entry(row_edges[i], v, gs, ge, views, cverdict, n_constraints, &other) > 0;
        view_state[v] = has ? AKZ_PG_VIEW_UPDATED : AKZ_PG_VIEW_NO_CONSTRAINT;
        updated += has ? 1u : 0u;
        n_edges += has;
    }
    stats[AKZ_PG_S_VIEWS] = ge - gs;
    stats[AKZ_PG_S_UPDATED] = updated;
    stats[AKZ_PG_S_EDGES] = n_edges;
    stats[AKZ_PG_S_STAGE] = AKZ_PG_STAGE_VIEWS;
    graph_verdict[g] = AKZ_PG_FEW_VIEWS;
    if (updated < 3u) return;
    /* ---- the rounds: every view reads the table of the round before ---- */
    stats[AKZ_PG_S_STAGE] = AKZ_PG_STAGE_ROUNDS;
    graph_verdict[g] = AKZ_PG_OK;
    double *cur = poses, *nxt = scratch;
    unsigned round = 0;
    for (; round < iterations && graph_verdict[g] == AKZ_PG_OK; ++round) {
        for (unsigned v = gs; v < ge; ++v) {
            double sum6[6];
            int ok = 1;
            if (view_state[v] == AKZ_PG_VIEW_UPDATED) {
                const unsigned *row = row_edges + row_start[v], n = row_start[v + 1] - row_start[v];
                if (sequential) akz_pg_sum_sequential(cur, v, row, n, views, cverdict, edges, sum6);
                else akz_pg_sum_wave(cur, v, row, n, views, cverdict, edges, sum6);
                ok = akz_pg_view_update(sum6, st->graph_optimization_rate, cur + 12 * (size_t)v, nxt + 12 * (size_t)v);
            } else
                for (int k = 0; k < 12; ++k) nxt[12 * (size_t)v + k] = cur[12 * (size_t)v + k];
            if (!ok) {
                view_state[v] = AKZ_PG_VIEW_NONFINITE;
                graph_verdict[g] = AKZ_PG_NONFINITE;
                if (stats[AKZ_PG_S_FIRST_BAD_VIEW] == AKZ_PG_NO_VIEW) stats[AKZ_PG_S_FIRST_BAD_VIEW] = v;
            }
        }
        double* t = cur; cur = nxt; nxt = t;
    }
    stats[AKZ_PG_S_ROUNDS] = round;
    if (cur != poses)
        for (size_t k = 12 * (size_t)gs; k < 12 * (size_t)ge; ++k) poses[k] = cur[k];
}
#endif /* !__HIP_DEVICE_COMPILE__ */

#endif /* AKZ_POSE_GRAPH_MATH_H */
