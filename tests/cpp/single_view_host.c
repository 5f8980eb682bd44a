/* The CPU checker of the single-view refinement: thin exported wrappers around include/akz_single_view_math.h, the text
 * cv_amd/csrc/rs_single_view.hip compiles for the device.  tests/single_view_checker.py has tests/host_build.py build this
 * with the host compiler (its `load`: -O2, no contraction to FMA) into a shared object and loads it with ctypes.  The
 * gather around the header (match -> landmarks -> observations -> keypoint -> bearing, the index checks) restates the
 * kernel's; the arithmetic is the header's. */
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/akz_single_view_math.h"

typedef struct sv_camera {   /* rs_camera of include/akz.h */
    double fx, fy, cx, cy, skew, k1;
    int32_t use_k1, reserved;
} sv_camera;

#define KP_BYTES 28   /* akz_keypoint: x, y (f32) first */

void sv_world_pose_gradient(const double* t, const double* b, double* g) { akz_sv_world_pose_gradient(t, b, g); }
int sv_landmark_delta(const double* pose, const double* b, const double* x, double* g) { return akz_sv_landmark_delta(pose, b, x, g); }
void sv_point(const double* world, double* x) { akz_sv_point(world, x); }

static double* to_soa(const double* lm6, uint32_t n)
{
    double* lm = (double*)calloc(6 * AKZ_SV_MAX_MATCHES, sizeof(double));
    if (!lm || n > AKZ_SV_MAX_MATCHES) { free(lm); return NULL; }
    for (uint32_t i = 0; i < n; ++i)
        for (int k = 0; k < 6; ++k) lm[k * AKZ_SV_MAX_MATCHES + i] = lm6[6 * (size_t)i + k];
    return lm;
}

/* the summed gradient of n matches [n][6] {bearing, Euclidean point}, n <= 2048, in the shipped order or the reference's */
int sv_sum(const double* pose, const double* lm6, uint32_t n, int sequential, double* net)
{
    double* lm = to_soa(lm6, n);
    if (!lm) return -1;
    if (sequential) akz_sv_sum_sequential(pose, lm, n, net);
    else akz_sv_sum_tree(pose, lm, n, net);
    free(lm);
    return 0;
}

/* one optimiser run: pose [12] in and out; returns the stopping iteration */
uint32_t sv_optimize(double* pose, double rate, uint32_t iterations, const double* lm6, uint32_t n, int sequential)
{
    double* lm = to_soa(lm6, n);
    if (!lm) return 0xFFFFFFFFu;
    const uint32_t it = akz_sv_optimize(pose, rate, iterations, lm, n, sequential);
    free(lm);
    return it;
}

static akz_sv_scene scene_of(uint32_t n, const double* bearing, const double* world, const uint32_t* obs_start, const double* obs_pose,
                             const double* obs_bearing)
{
    akz_sv_scene sc;
    sc.n = n; sc.bearing = bearing; sc.world = world; sc.obs_start = obs_start; sc.obs_pose = obs_pose; sc.obs_bearing = obs_bearing;
    return sc;
}

/* is_observation_consistent of original match i of a scene given as arrays */
int sv_consistent(uint32_t n, const double* bearing, const double* world, const uint32_t* obs_start, const double* obs_pose,
                  const double* obs_bearing, uint32_t i, const double* pose, const akz_sv_settings* st)
{
    const akz_sv_scene sc = scene_of(n, bearing, world, obs_start, obs_pose, obs_bearing);
    return akz_sv_host_consistent(&sc, i, pose, st);
}

/* one scene given as arrays */
int sv_refine(uint32_t n, const double* bearing, const double* world, const uint32_t* obs_start, const double* obs_pose,
              const double* obs_bearing, const double* pose_in, int has_model, const uint32_t* inliers, uint32_t n_inliers,
              const akz_sv_settings* st, int sequential, double* pose_out, unsigned char* final_mask, uint32_t* n_final, uint32_t* stats)
{
    const akz_sv_scene sc = scene_of(n, bearing, world, obs_start, obs_pose, obs_bearing);
    double* lm = (double*)calloc(6 * AKZ_SV_MAX_MATCHES, sizeof(double));
    int v = -1;
    if (lm && st->single_view_optimization_num_matches <= AKZ_SV_MAX_MATCHES && st->single_view_filter_loop_iterations < AKZ_SV_MAX_RUNS)
        v = akz_sv_refine_scene(&sc, pose_in, has_model, inliers, n_inliers, st, sequential, lm, pose_out, final_mask, n_final, stats);
    free(lm);
    return v;
}

static void bearing_of(const unsigned char* kps, uint32_t cap, uint32_t blk, uint32_t feat, const sv_camera* cam, double* b)
{
    const float* kp = (const float*)(kps + ((size_t)blk * cap + feat) * KP_BYTES);
    akz_tri_calibrate(&cam->fx, cam->use_k1, cam->k1, kp[0], kp[1], b);
}

/* the observation ranges of original match i, as sv_resolve of the kernel: 0 = it names something outside the arrays */
static int resolve(const uint32_t* m, uint32_t i, uint32_t cap, uint32_t n_world, uint32_t n_rows, const uint32_t* best, const uint32_t* obs_start,
                   uint32_t n_obs, uint32_t n_landmarks, uint32_t* r /* s0 n0 s1 n1 */)
{
    const uint32_t feat = m[2 * (size_t)i], row = m[2 * (size_t)i + 1];
    r[0] = r[1] = r[2] = r[3] = 0;
    if (feat >= cap || row >= n_rows) return 0;
    uint32_t l0 = row;
    if (row >= n_world) {
        const size_t e = (size_t)(row - n_world) * 3;
        l0 = best[2 * e];
        const uint32_t l1 = best[2 * (e + 1)];
        if (l1 >= n_landmarks) return 0;
        if (obs_start[l1] > obs_start[l1 + 1] || obs_start[l1 + 1] > n_obs) return 0;
        r[2] = obs_start[l1]; r[3] = obs_start[l1 + 1] - obs_start[l1];
    }
    if (l0 >= n_landmarks) return 0;
    if (obs_start[l0] > obs_start[l0 + 1] || obs_start[l0 + 1] > n_obs) return 0;
    r[0] = obs_start[l0]; r[1] = obs_start[l0 + 1] - obs_start[l0];
    return 1;
}

/* one scene as rs_refine_poses_batch_device sees it: `matches`, `inliers` the scene's own rows; `best` the whole array or NULL;
 * n_rows = n_world, or n_world + n_scenes * cap with `best` */
int sv_refine_scene(const unsigned char* kps, uint32_t cap, uint32_t n_blocks, const double* poses, const sv_camera* cam, const uint32_t* obs_start,
                    const uint32_t* obs, uint32_t n_obs, uint32_t n_landmarks, const double* world, uint32_t n_world, uint32_t n_rows,
                    uint32_t ik, const uint32_t* matches, uint32_t n, const uint32_t* best, const double* pose_in, uint32_t best_id,
                    const uint32_t* inliers, uint32_t n_inliers, const akz_sv_settings* st, double* pose_out, unsigned char* final_mask,
                    uint32_t* n_final, uint32_t* stats)
{
    if (n > cap) n = cap;
    if (n_inliers > cap) n_inliers = cap;
    for (int k = 0; k < AKZ_SV_STATS; ++k) stats[k] = 0u;
    for (int r = 0; r < 2 * AKZ_SV_MAX_RUNS; ++r) stats[AKZ_SV_S_RUN_MATCHES + r] = 0xFFFFFFFFu;
    *n_final = 0u;
    int bad = ik >= n_blocks;
    size_t total = 0;
    for (uint32_t i = 0; i < n && !bad; ++i) {
        uint32_t r[4];
        if (!resolve(matches, i, cap, n_world, n_rows, best, obs_start, n_obs, n_landmarks, r)) {
            bad = 1;
            break;
        }
        for (uint32_t k = 0; k < r[1] + r[3]; ++k) {
            const size_t at = k < r[1] ? (size_t)r[0] + k : (size_t)r[2] + (k - r[1]);
            bad |= obs[2 * at] >= n_blocks || obs[2 * at + 1] >= cap;
        }
        total += (size_t)r[1] + r[3];
    }
    if (bad) return AKZ_SV_BAD_INDEX;
    double* bearing = (double*)calloc(3 * (size_t)(n ? n : 1), sizeof(double));
    double* wpt = (double*)calloc(4 * (size_t)(n ? n : 1), sizeof(double));
    uint32_t* start = (uint32_t*)calloc((size_t)n + 1, sizeof(uint32_t));
    double* op = (double*)calloc(12 * (total ? total : 1), sizeof(double));
    double* ob = (double*)calloc(3 * (total ? total : 1), sizeof(double));
    int v = -1;
    if (bearing && wpt && start && op && ob) {
        size_t at_out = 0;
        for (uint32_t i = 0; i < n; ++i) {
            uint32_t r[4];
            resolve(matches, i, cap, n_world, n_rows, best, obs_start, n_obs, n_landmarks, r);
            bearing_of(kps, cap, ik, matches[2 * (size_t)i], cam, bearing + 3 * (size_t)i);
            for (int k = 0; k < 4; ++k) wpt[4 * (size_t)i + k] = world[4 * (size_t)matches[2 * (size_t)i + 1] + k];
            start[i] = (uint32_t)at_out;
            for (uint32_t k = 0; k < r[1] + r[3]; ++k, ++at_out) {
                const size_t at = k < r[1] ? (size_t)r[0] + k : (size_t)r[2] + (k - r[1]);
                const uint32_t blk = obs[2 * at], feat = obs[2 * at + 1];
                bearing_of(kps, cap, blk, feat, cam, ob + 3 * at_out);
                for (int q = 0; q < 12; ++q) op[12 * at_out + q] = poses[12 * (size_t)blk + q];
            }
        }
        start[n] = (uint32_t)at_out;
        v = sv_refine(n, bearing, wpt, start, op, ob, pose_in, best_id != 0xFFFFFFFFu, inliers, n_inliers, st, 0, pose_out, final_mask, n_final,
                      stats);
    }
    free(bearing); free(wpt); free(start); free(op); free(ob);
    return v;
}

/* the values is_observation_consistent compares for original match i under `pose`: out[0] = the sine distance for one other
 * observation, out[0 .. k] = the k + 1 cosine distances for k >= 2 (NaN where no point came out); returns how many */
uint32_t sv_consistency_values(uint32_t n, const double* bearing, const double* world, const uint32_t* obs_start, const double* obs_pose,
                               const double* obs_bearing, uint32_t i, const double* pose, const akz_sv_settings* st, double* out, uint32_t cap)
{
    const akz_sv_scene sc = scene_of(n, bearing, world, obs_start, obs_pose, obs_bearing);
    akz_sv_host_src src;
    src.sc = &sc; src.s0 = obs_start[i]; src.k = obs_start[i + 1] - obs_start[i];
    src.pose = pose; src.bearing = bearing + 3 * (size_t)i;
    double op[12], ob[3], p[4];
    if (src.k == 0u || src.k + 1u > cap) return 0;
    if (src.k == 1u) {
        double inv[12], total[12], ra[3];
        akz_sv_host_fetch(&src, 0u, op, ob);
        akz_tv_pose_inverse(pose, inv);
        akz_tvc_pose_mul(op, inv, total);
        akz_tv_rotate(total, src.bearing, ra);
        const double t[3] = {total[3], total[7], total[11]};
        out[0] = akz_tv_loss(t, ra, ob);
        return 1;
    }
    const int why = akz_sv_host_triangulate(&src, src.k + 1u, 0, &st->tri, p);
    for (uint32_t k = 0; k <= src.k; ++k) {
        akz_sv_host_fetch(&src, k, op, ob);
        out[k] = why == AKZ_TRI_OK ? akz_tv_transformed_distance(op, p, ob) : __builtin_nan("");
    }
    return src.k + 1u;
}
