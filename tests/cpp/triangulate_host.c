/* The CPU checker of the triangulation kernels: thin exported wrappers around include/akz_triangulate_math.h, the text
 * cv_amd/csrc/rs_triangulate.hip compiles for the device.  tests/triangulate_checker.py has tests/host_build.py build this
 * with the host compiler (its `load`: -O2, no contraction to FMA) into a shared object and loads it with ctypes.  The loops
 * around the header (which list belongs to which row) restate the kernels'; the arithmetic is the header's. */
#include <stddef.h>
#include <stdint.h>

#include "../../include/akz_triangulate_math.h"

typedef struct tri_camera {   /* rs_camera of include/akz.h */
    double fx, fy, cx, cy, skew, k1;
    int32_t use_k1, reserved;
} tri_camera;

#define KP_BYTES 28   /* akz_keypoint: x, y (f32) first */

/* ---- a list handed over as arrays ---- */
typedef struct array_src {
    const double* poses;
    const double* bearings;
} array_src;
static inline int array_fetch(const array_src* s, unsigned i, double* pose, double* b)
{
    for (int k = 0; k < 12; ++k) pose[k] = s->poses[(size_t)12 * i + k];
    for (int k = 0; k < 3; ++k) b[k] = s->bearings[(size_t)3 * i + k];
    return 1;
}
AKZ_TRI_DEFINE_TRIANGULATE(tri_array, array_src, array_fetch)

int tri_observations(const double* poses, const double* bearings, uint32_t n, int robust, const akz_tri_settings* st, double* out)
{
    array_src s = {poses, bearings};
    return tri_array(&s, n, robust, st, out);
}

/* ---- CSR lists of {block, feature} ---- */
typedef struct list_src {
    const uint32_t* obs;
    const unsigned char* kps;
    const double* poses;
    const tri_camera* cam;
    uint32_t s0, n0, s1, cap, n_blocks;
} list_src;
static inline int list_fetch(const list_src* s, unsigned i, double* pose, double* b)
{
    const size_t at = i < s->n0 ? (size_t)s->s0 + i : (size_t)s->s1 + (i - s->n0);
    const uint32_t blk = s->obs[2 * at], feat = s->obs[2 * at + 1];
    if (blk >= s->n_blocks || feat >= s->cap) return 0;
    const float* kp = (const float*)(s->kps + ((size_t)blk * s->cap + feat) * KP_BYTES);
    akz_tri_calibrate(&s->cam->fx, s->cam->use_k1, s->cam->k1, kp[0], kp[1], b);
    for (int k = 0; k < 12; ++k) pose[k] = s->poses[(size_t)12 * blk + k];
    return 1;
}
AKZ_TRI_DEFINE_TRIANGULATE(tri_list, list_src, list_fetch)

static int range_ok(const uint32_t* start, uint32_t l, uint32_t n_obs, uint32_t* s, uint32_t* n)
{
    const uint32_t a = start[l], b = start[l + 1];
    *s = a;
    *n = b >= a ? b - a : 0u;
    return a <= b && b <= n_obs;
}

void tri_landmarks(const unsigned char* kps, uint32_t cap, uint32_t n_blocks, const double* poses, const tri_camera* cam,
                   const uint32_t* obs_start, const uint32_t* obs, uint32_t n_obs, uint32_t n_landmarks, const akz_tri_settings* st,
                   double* world, unsigned char* reason)
{
    for (uint32_t l = 0; l < n_landmarks; ++l) {
        list_src s = {obs, kps, poses, cam, 0, 0, 0, cap, n_blocks};
        int why = AKZ_TRI_BAD_INDEX;
        akz_tri_none(world + 4 * (size_t)l);
        if (range_ok(obs_start, l, n_obs, &s.s0, &s.n0)) why = tri_list(&s, s.n0, 1, st, world + 4 * (size_t)l);
        if (reason) reason[l] = (unsigned char)why;
    }
}

/* best [n_frames][cap][3][2] u32 {landmark, distance}, decision [n_frames][cap] u32, merge_ok [n_frames][cap] u8 */
void tri_merged(const unsigned char* kps, uint32_t cap, uint32_t n_blocks, const double* poses, const tri_camera* cam,
                const uint32_t* obs_start, const uint32_t* obs, uint32_t n_obs, uint32_t n_landmarks, const akz_tri_settings* st,
                const uint32_t* best, const uint32_t* decision, const unsigned char* merge_ok, uint32_t n_frames, uint32_t n_world,
                double* world, unsigned char* reason)
{
    for (size_t fj = 0; fj < (size_t)n_frames * cap; ++fj) {
        if (decision[fj] != 2u || !merge_ok[fj]) continue;
        const uint32_t l0 = best[fj * 6], l1 = best[fj * 6 + 2];
        list_src s = {obs, kps, poses, cam, 0, 0, 0, cap, n_blocks};
        double* row = world + 4 * ((size_t)n_world + fj);
        int why = AKZ_TRI_BAD_INDEX;
        uint32_t n1 = 0;
        akz_tri_none(row);
        if (l0 < n_landmarks && l1 < n_landmarks && range_ok(obs_start, l0, n_obs, &s.s0, &s.n0) && range_ok(obs_start, l1, n_obs, &s.s1, &n1))
            why = tri_list(&s, s.n0 + n1, 1, st, row);
        if (reason) reason[fj] = (unsigned char)why;
    }
}

/* ---- the inliers of a two-view consensus ---- */
typedef struct pair_src {
    double a[3], b[3];
    const double* pose;
} pair_src;
static inline int pair_fetch(const pair_src* s, unsigned i, double* pose, double* b)
{
    for (int k = 0; k < 12; ++k) pose[k] = i == 0 ? ((k == 0 || k == 5 || k == 10) ? 1.0 : 0.0) : s->pose[k];
    for (int k = 0; k < 3; ++k) b[k] = i == 0 ? s->a[k] : s->b[k];
    return 1;
}
AKZ_TRI_DEFINE_TRIANGULATE(tri_pair, pair_src, pair_fetch)

/* one scene: kps_a / kps_b the scene's two keypoint blocks ([cap] each), pairs [cap][2], the consensus' pose and inliers */
void tri_pairs_scene(const unsigned char* kps_a, const unsigned char* kps_b, uint32_t cap, const uint32_t* pairs, uint32_t npairs,
                     const tri_camera* cam_a, const tri_camera* cam_b, const double* pose, const uint32_t* inliers, uint32_t n_inliers,
                     const akz_tri_settings* st, double* points, unsigned char* reason)
{
    if (n_inliers > cap) n_inliers = cap;
    if (npairs > cap) npairs = cap;
    for (uint32_t i = 0; i < n_inliers; ++i) {
        int why = AKZ_TRI_BAD_INDEX;
        const uint32_t m = inliers[i];
        akz_tri_none(points + 4 * (size_t)i);
        if (m < npairs && pairs[2 * m] < cap && pairs[2 * m + 1] < cap) {
            pair_src s;
            const float* ka = (const float*)(kps_a + (size_t)pairs[2 * m] * KP_BYTES);
            const float* kb = (const float*)(kps_b + (size_t)pairs[2 * m + 1] * KP_BYTES);
            akz_tri_calibrate(&cam_a->fx, cam_a->use_k1, cam_a->k1, ka[0], ka[1], s.a);
            akz_tri_calibrate(&cam_b->fx, cam_b->use_k1, cam_b->k1, kb[0], kb[1], s.b);
            s.pose = pose;
            why = tri_pair(&s, 2u, 0, st, points + 4 * (size_t)i);
        }
        if (reason) reason[i] = (unsigned char)why;
    }
}

/* ---- the pieces, for the rule tests ---- */
int tri_solve(const double* a16, double eps, int max_sweeps, double* out)
{
    double a[16];
    for (int k = 0; k < 16; ++k) a[k] = a16[k];
    return akz_tri_solve(a, eps, max_sweeps, out);
}
void tri_from_homogeneous(double* p) { akz_tri_from_homogeneous(p); }
void tri_accumulate(double* a16, const double* pose, const double* bearing) { akz_tri_accumulate(a16, pose, bearing); }
uint64_t tri_float_ord(double x) { return akz_tri_float_ord(x); }
void tri_calibrate(const tri_camera* cam, float x, float y, double* out) { akz_tri_calibrate(&cam->fx, cam->use_k1, cam->k1, x, y, out); }
