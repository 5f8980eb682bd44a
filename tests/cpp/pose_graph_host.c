/* The CPU checker of the pose-graph relaxation: thin exported wrappers around include/akz_pose_graph_math.h, the text
 * cv_amd/csrc/rs_pose_graph.hip compiles for the device.  tests/pose_graph_checker.py has tests/host_build.py build this
 * with the host compiler (its `load`: -O2, no contraction to FMA) into a shared object and loads it with ctypes.  The
 * arithmetic and the control flow of a graph are the header's. */
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/akz_pose_graph_math.h"

double pg_acos(double c) { return akz_pm_acos(c); }
void pg_acos_many(const double* c, uint32_t n, double* out)
{
    for (uint32_t i = 0; i < n; ++i) out[i] = akz_pm_acos(c[i]);
}
void pg_log(const double* pose, double* w) { akz_pg_log(pose, w); }
void pg_exp(const double* w, double* r9) { akz_tv_from_scaled_axis(w, r9); }
void pg_se3(const double* delta, double* se3) { akz_pg_se3(delta, se3); }
void pg_edge_se3(const double* expected, const double* other, const double* inv, double* se3) { akz_pg_edge_se3(expected, other, inv, se3); }
void pg_from_se3_mul(const double* net, const double* pose, double* out) { akz_pg_from_se3_mul(net, pose, out); }
int pg_view_update(const double* sum6, double rate, const double* pose, double* out) { return akz_pg_view_update(sum6, rate, pose, out); }
void pg_apply_delta(const double* delta, double* pose) { akz_tv_apply_delta(delta, pose); }
uint32_t pg_slot_target(uint32_t slot) { return akz_pg_slot_target(slot); }
uint32_t pg_slot_other(uint32_t slot) { return akz_pg_slot_other(slot); }

/* rs_pose_graph_edges_device: [n][6][12] from the constraint call's poses [n][2][12] and verdicts */
void pg_edges(const double* cposes, const uint32_t* cverdict, uint32_t n, double* edges)
{
    for (uint32_t c = 0; c < n; ++c) {
        if (cverdict[c] == AKZ_TVC_OK) akz_pg_constraint_edges(cposes + 24 * (size_t)c, edges + 72 * (size_t)c);
        else
            for (int k = 0; k < 72; ++k) edges[72 * (size_t)c + k] = 0.0;
    }
}

/* the sum of view v's row in either order */
void pg_sum(const double* poses, uint32_t v, const uint32_t* row, uint32_t n, const uint32_t* views, const uint32_t* cverdict,
            const double* edges, int sequential, double* sum6)
{
    if (sequential) akz_pg_sum_sequential(poses, v, row, n, views, cverdict, edges, sum6);
    else akz_pg_sum_wave(poses, v, row, n, views, cverdict, edges, sum6);
}

/* rs_pose_graph_relax_batch_device on host arrays */
int pg_relax_batch(double* poses, uint32_t n_views, const uint32_t* graph_start, uint32_t n_graphs, const uint32_t* row_start,
                   const uint32_t* row_edges, uint32_t n_rows, const uint32_t* views, const uint32_t* cverdict, const double* edges,
                   uint32_t n_constraints, const akz_pg_settings* st, int sequential, uint32_t* graph_verdict, uint32_t* view_state,
                   uint32_t* stats)
{
    double* scratch = (double*)calloc(12 * (size_t)(n_views ? n_views : 1), sizeof(double));
    if (!scratch) return -1;
    for (uint32_t g = 0; g < n_graphs; ++g)
        akz_pg_relax_graph(poses, scratch, n_views, graph_start, g, row_start, row_edges, n_rows, views, cverdict, edges, n_constraints, st,
                           sequential, graph_verdict, view_state, stats);
    free(scratch);
    return 0;
}
