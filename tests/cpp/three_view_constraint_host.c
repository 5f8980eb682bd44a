/* The CPU checker of the three-view constraints: thin exported wrappers around include/akz_three_view_constraint_math.h,
 * the text cv_amd/csrc/rs_three_view_constraint.hip compiles for the device.  tests/three_view_constraint_checker.py has
 * tests/host_build.py build this with the host compiler (its `load`: -O2, no contraction to FMA) into a shared object and
 * loads it with ctypes.  The gather around the header (keypoint -> bearing, the index checks) restates the kernel's; the
 * arithmetic is the header's. */
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/akz_three_view_constraint_math.h"

typedef struct tvc_camera {   /* rs_camera of include/akz.h */
    double fx, fy, cx, cy, skew, k1;
    int32_t use_k1, reserved;
} tvc_camera;

#define KP_BYTES 28   /* akz_keypoint: x, y (f32) first */

void tvc_pose_mul(const double* a, const double* b, double* out) { akz_tvc_pose_mul(a, b, out); }
void tvc_relative_poses(const double* world, double* rel) { akz_tvc_relative_poses(world, world + 12, world + 24, rel); }
double tvc_rate(double norm, double std) { return akz_tvc_rate(norm, std); }
void tvc_adaptive_step(const double* nets16, double inv_len, double* inv) { akz_tvc_adaptive_step(nets16, inv_len, inv); }
/* the 16 sums of one iteration under the inverted poses inv [2][12]; n <= 256 */
int tvc_sums(const double* inv, const double* lm9, uint32_t n, int sequential, double* nets16)
{
    if (n > AKZ_TVC_MAX_LANDMARKS) return -1;
    if (sequential) akz_tvc_sum_sequential(inv, lm9, n, nets16);
    else akz_tvc_sum_wave(inv, lm9, n, nets16);
    return 0;
}
/* three_view_adaptive_optimize_l2: poses [2][12] in and out, landmarks [n][9] */
int tvc_adaptive_optimize(double* poses, uint32_t iterations, const double* lm9, uint32_t n, int sequential)
{
    if (n > AKZ_TVC_MAX_LANDMARKS) return -1;
    akz_tvc_adaptive_optimize(poses, iterations, lm9, n, sequential);
    return 0;
}
/* optimize_three_view from bearings: world [3][12], landmarks [n_list][9] */
int tvc_constraint(const double* world, const double* lm9, uint32_t n_list, const akz_tvc_settings* st, int sequential, double* pose_out,
                   uint32_t* stats)
{
    if (st->optimization_maximum_landmarks > AKZ_TVC_MAX_LANDMARKS) return -1;
    return akz_tvc_constraint(world, lm9, n_list, st, sequential, pose_out, stats);
}

/* one constraint as rs_three_view_constraint_batch_device sees it: keypoint blocks, the pose table, the views, the CSR lists */
int tvc_constraint_scene(const unsigned char* kps, uint32_t cap, uint32_t n_blocks, const double* poses, const tvc_camera* cam,
                         const uint32_t* views, const uint32_t* lm_start, const uint32_t* lm, uint32_t n_lm, uint32_t s,
                         const akz_tvc_settings* st, double* pose_out, uint32_t* stats)
{
    const uint32_t v[3] = {views[3 * (size_t)s], views[3 * (size_t)s + 1], views[3 * (size_t)s + 2]};
    const uint32_t begin = lm_start[s], end = lm_start[s + 1];
    if (st->optimization_maximum_landmarks > AKZ_TVC_MAX_LANDMARKS) return -1;
    int bad = v[0] >= n_blocks || v[1] >= n_blocks || v[2] >= n_blocks || begin > end || end > n_lm;
    const uint32_t n_list = bad ? 0u : end - begin;
    const uint32_t* list = lm + 3 * (size_t)(bad ? 0u : begin);
    for (size_t i = 0; i < 3 * (size_t)n_list && !bad; ++i) bad = list[i] >= cap;
    if (bad) {
        for (int k = 0; k < AKZ_TVC_STATS; ++k) stats[k] = 0u;
        return AKZ_TVC_BAD_INDEX;
    }
    const uint32_t used = n_list < st->optimization_maximum_landmarks ? n_list : st->optimization_maximum_landmarks;
    double* lm9 = (double*)calloc(9 * (size_t)(used ? used : 1), sizeof(double));
    if (!lm9) return -1;
    for (uint32_t i = 0; i < used; ++i)
        for (int k = 0; k < 3; ++k) {
            const float* kp = (const float*)(kps + ((size_t)v[k] * cap + list[3 * (size_t)i + k]) * KP_BYTES);
            akz_tri_calibrate(&cam->fx, cam->use_k1, cam->k1, kp[0], kp[1], lm9 + 9 * (size_t)i + 3 * k);
        }
    double world[36];
    for (int k = 0; k < 12; ++k) {
        world[k] = poses[(size_t)12 * v[0] + k];
        world[12 + k] = poses[(size_t)12 * v[1] + k];
        world[24 + k] = poses[(size_t)12 * v[2] + k];
    }
    /* akz_tvc_constraint reads the first min(n_list, maximum) landmarks only: the list's length goes in, `used` rows exist */
    const int verdict = akz_tvc_constraint(world, lm9, n_list, st, 0, pose_out, stats);
    free(lm9);
    return verdict;
}
