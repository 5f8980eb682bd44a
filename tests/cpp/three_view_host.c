/* The CPU checker of the three-view bootstrap: thin exported wrappers around include/akz_three_view_math.h, the text
 * cv_amd/csrc/rs_three_view.hip compiles for the device.  tests/three_view_checker.py has tests/host_build.py build this
 * with the host compiler (its `load`: -O2, no contraction to FMA) into a shared object and loads it with ctypes.  The
 * gather around the header (keypoint -> bearing, the index checks) restates the kernel's; the arithmetic is the header's. */
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/akz_three_view_math.h"

typedef struct tv_camera {   /* rs_camera of include/akz.h */
    double fx, fy, cx, cy, skew, k1;
    int32_t use_k1, reserved;
} tv_camera;

#define KP_BYTES 28   /* akz_keypoint: x, y (f32) first */

void tv_gradients(const double* inv, const double* c, const double* f, const double* s, double* g) { akz_tv_landmark_gradients(inv, c, f, s, g); }
void tv_three_view_gradients(const double* c, const double* f, const double* ftoc, const double* s, const double* stoc, double* g)
{
    akz_tv_three_view_gradients(c, f, ftoc, s, stoc, g);
}
int tv_sine_l1(const double* t, const double* a, const double* b, double* point) { return akz_tv_triangulate_sine_l1(t, a, b, point); }
void tv_pose_inverse(const double* p, double* o) { akz_tv_pose_inverse(p, o); }
void tv_from_scaled_axis(const double* w, double* r) { akz_tv_from_scaled_axis(w, r); }
double tv_loss(const double* t, const double* a, const double* b) { return akz_tv_loss(t, a, b); }
int tv_tri_robust(const double* first, const double* second, const double* c, const double* f, const double* s, double max_cos, double inc,
                  const akz_tv_settings* st)
{
    return akz_tv_tri_landmark_robust(first, second, c, f, s, max_cos, inc, &st->tri);
}
int tv_bi_robust(const double* pose, const double* a, const double* b, double max_sine) { return akz_tv_bi_landmark_robust(pose, a, b, max_sine); }
int tv_relative_scale(const double* first, const double* second, const double* c, const double* f, const double* s, const akz_tv_settings* st,
                      double* ratio)
{
    return akz_tv_relative_scale(first, second, c, f, s, st, ratio);
}

static void to_soa(const double* lm9, uint32_t n, double* lm)
{
    for (uint32_t i = 0; i < n; ++i)
        for (int k = 0; k < 9; ++k) lm[k * AKZ_TV_MAX_LANDMARKS + i] = lm9[9 * (size_t)i + k];
}

/* the summed gradients of n landmarks [n][9] {c, f, s}, n <= 1024, in the shipped order or the reference's */
int tv_sum(const double* inv, const double* lm9, uint32_t n, int sequential, double* nets)
{
    double* lm = (double*)calloc(9 * AKZ_TV_MAX_LANDMARKS, sizeof(double));
    if (!lm || n > AKZ_TV_MAX_LANDMARKS) { free(lm); return -1; }
    to_soa(lm9, n, lm);
    if (sequential) akz_tv_sum_sequential(inv, lm, n, nets);
    else akz_tv_sum_tree(inv, lm, n, nets);
    free(lm);
    return 0;
}

/* one optimiser run: poses [2][12] in and out, landmarks [n][9] {c, f, s}, n <= 1024; returns the stopping iteration */
uint32_t tv_optimize(double* poses, double rate, uint32_t iterations, const double* lm9, uint32_t n, int sequential)
{
    double* lm = (double*)calloc(9 * AKZ_TV_MAX_LANDMARKS, sizeof(double));
    if (!lm || n > AKZ_TV_MAX_LANDMARKS) { free(lm); return 0xFFFFFFFFu; }
    to_soa(lm9, n, lm);
    const uint32_t it = akz_tv_optimize(poses, rate, iterations, lm, n, sequential);
    free(lm);
    return it;
}

/* one triple from bearings */
int tv_init_triple(const double* pose_in, const double* c, const double* f, const double* s, uint32_t n, const double* first_c,
                   const double* first_f, uint32_t n_first, const double* second_c, const double* second_s, uint32_t n_second,
                   const akz_tv_settings* st, int sequential, double* pose_out, unsigned char* combined, unsigned char* first_ok,
                   unsigned char* second_ok, uint32_t* stats)
{
    unsigned long long* keys = (unsigned long long*)calloc(n ? n : 1, sizeof *keys);
    double* lm = (double*)calloc(9 * AKZ_TV_MAX_LANDMARKS, sizeof(double));
    int v = -1;
    if (keys && lm && st->three_view_optimization_landmarks <= AKZ_TV_MAX_LANDMARKS && st->three_view_filter_loop_iterations < AKZ_TV_MAX_RUNS)
        v = akz_tv_init_triple(pose_in, c, f, s, n, first_c, first_f, n_first, second_c, second_s, n_second, st, sequential, keys, lm, pose_out,
                               combined, first_ok, second_ok, stats);
    free(keys);
    free(lm);
    return v;
}

static void bearing_of(const unsigned char* kps, uint32_t cap, uint32_t blk, uint32_t feat, const tv_camera* cam, double* b)
{
    const float* kp = (const float*)(kps + ((size_t)blk * cap + feat) * KP_BYTES);
    akz_tri_calibrate(&cam->fx, cam->use_k1, cam->k1, kp[0], kp[1], b);
}

/* one scene as rs_three_view_init_batch_device sees it: keypoint blocks, block ids, index lists [cap][3] / [cap][2] */
int tv_init_scene(const unsigned char* kps, uint32_t cap, uint32_t n_blocks, uint32_t ic, uint32_t i_first, uint32_t i_second,
                  const tv_camera* cam, const double* pose_in, const uint32_t* triples, uint32_t n, const uint32_t* first_only,
                  uint32_t n_first, const uint32_t* second_only, uint32_t n_second, const akz_tv_settings* st, double* pose_out,
                  unsigned char* combined, unsigned char* first_ok, unsigned char* second_ok, uint32_t* stats)
{
    if (n > cap) n = cap;
    if (n_first > cap) n_first = cap;
    if (n_second > cap) n_second = cap;
    int bad = ic >= n_blocks || i_first >= n_blocks || i_second >= n_blocks;
    for (uint32_t i = 0; i < 3 * n && !bad; ++i) bad = triples[i] >= cap;
    for (uint32_t i = 0; i < 2 * n_first && !bad; ++i) bad = first_only[i] >= cap;
    for (uint32_t i = 0; i < 2 * n_second && !bad; ++i) bad = second_only[i] >= cap;
    if (bad) {
        for (int k = 0; k < AKZ_TV_STATS; ++k) stats[k] = 0u;
        for (int r = 0; r < 2 * AKZ_TV_MAX_RUNS; ++r) stats[AKZ_TV_S_RUN_MATCHES + r] = 0xFFFFFFFFu;
        return AKZ_TV_BAD_INDEX;
    }
    const size_t total = (size_t)3 * n + 2 * (size_t)n_first + 2 * (size_t)n_second;
    double* b = (double*)calloc(3 * (total ? total : 1), sizeof(double));
    if (!b) return -1;
    double *c = b, *f = c + 3 * (size_t)n, *s = f + 3 * (size_t)n, *fc = s + 3 * (size_t)n, *ff = fc + 3 * (size_t)n_first,
           *sc = ff + 3 * (size_t)n_first, *ss = sc + 3 * (size_t)n_second;
    for (uint32_t i = 0; i < n; ++i) {
        bearing_of(kps, cap, ic, triples[3 * i], cam, c + 3 * i);
        bearing_of(kps, cap, i_first, triples[3 * i + 1], cam, f + 3 * i);
        bearing_of(kps, cap, i_second, triples[3 * i + 2], cam, s + 3 * i);
    }
    for (uint32_t i = 0; i < n_first; ++i) {
        bearing_of(kps, cap, ic, first_only[2 * i], cam, fc + 3 * i);
        bearing_of(kps, cap, i_first, first_only[2 * i + 1], cam, ff + 3 * i);
    }
    for (uint32_t i = 0; i < n_second; ++i) {
        bearing_of(kps, cap, ic, second_only[2 * i], cam, sc + 3 * i);
        bearing_of(kps, cap, i_second, second_only[2 * i + 1], cam, ss + 3 * i);
    }
    const int v = tv_init_triple(pose_in, c, f, s, n, fc, ff, n_first, sc, ss, n_second, st, 0, pose_out, combined, first_ok, second_ok, stats);
    free(b);
    return v;
}
