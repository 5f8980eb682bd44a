/* akz_export_math.h — cv-sfm's export_reconstruction: which landmarks become points of the cloud, a point's position and colour,
 * a view's camera and the five vertices of its frustum.  Written once for gcc (the CPU checker, tests/cpp/export_host.c) and
 * hipcc (the gfx950 kernels of cv_amd/csrc/rs_export.hip): parity is "host build == HIP" in every byte of every output.
 *
 * Reference code restated here (paths relative to rust-cv/cv):
 *   VSlam::export_reconstruction                    cv-sfm/src/lib.rs:2285-2340
 *   export (the vertices of a camera, their order)  cv-sfm/src/export.rs:95-106
 *
 * Departures:
 *   - order: the reference walks the landmarks' SlotMap; here the points ascend with the landmark key, which is that order;
 *   - a point's colour: the reference takes `observations.iter().next()` of a HashMap, an order it does not define.  Here it is
 *     the colour of the first entry of the landmark's observation list;
 *   - a row with a point whose list is empty, leaves the table, or whose first entry names a block >= n_blocks or a feature >=
 *     cap is skipped alone and counted (the reference's unwrap() would panic); a row of the world table behind the landmark
 *     table has no list and is such a row;
 *   - a w that is NaN is not exported and is counted with w == 0 (Projective::point() would hand on a NaN point);
 *   - the mean (the `average` crate's Mean, not in the tree: unpinned): a sum in akz_sum_order.h's order, T = 256, divided by
 *     the count; a mean over nothing is 0, not the reference's NaN (akz_nr_mean);
 *   - a view's count above the capacity is read as the capacity;
 *   - the isometry inverse and its products with the origin, -y and z (nalgebra, not in the tree: unpinned):
 *     akz_tv_pose_inverse, then each product in full, ((m0 * x + m1 * y) + m2 * z) [+ t], zeros and ones included;
 *   - the frustum corners: ((c + fwd * f) + ((u * up) * f)) + ((r * right) * f), the reference's expression left to right.
 */
#ifndef AKZ_EXPORT_MATH_H
#define AKZ_EXPORT_MATH_H

#include "akz_reconstruction_merge_math.h"

/* the verdict on an export (RS_EX_* of include/akz.h) */
enum {
    AKZ_EX_OK = 0,
    AKZ_EX_OVERFLOW = 1,        /* more points than the room: the first `room` are written */
    AKZ_EX_BAD_TABLE = 2        /* the starts do not begin at 0 or do not ascend inside [0, n_obs]: no point is written */
};
/* words of d_counts_out */
enum { AKZ_EX_C_POINTS = 0, AKZ_EX_C_NO_POINT = 1, AKZ_EX_C_INFINITE = 2, AKZ_EX_C_BAD_ROWS = 3, AKZ_EX_COUNTS = 4 };
/* what a row of the world table is to an export */
enum { AKZ_EX_ROW_POINT = 0, AKZ_EX_ROW_NO_POINT = 1, AKZ_EX_ROW_INFINITE = 2, AKZ_EX_ROW_BAD = 3 };
/* a camera row {centre [3], up [3], forward [3], focal length}; the vertices of its frustum */
enum { AKZ_EX_CAMERA_WORDS = 10, AKZ_EX_CAMERA_VERTICES = 5 };

/* ---- a landmark's exported point (lib.rs:2292-2307) ---- */
/* start l <= n_landmarks breaks "the starts begin at 0 and ascend inside [0, n_obs]" */
AKZ_LT_FN int akz_ex_start_bad(const uint32_t* start, uint32_t l, uint32_t n_landmarks, uint32_t n_obs)
{
    return (l == 0u && start[0] != 0u) || akz_lt_start_bad(start, l, n_landmarks, n_obs);
}
/* Row l < n_world of the world table: AKZ_EX_ROW_*; for AKZ_EX_ROW_POINT the first entry {*block, *feature} of its list, both
 * inside the colour table.  w < 0 is akz_tri_none, w == 0 of either sign Projective::point()'s None.  Nothing is read outside
 * start [n_landmarks + 1] and obs [n_obs][2]. */
AKZ_LT_FN uint32_t akz_ex_row(const double* world, const uint32_t* start, const uint32_t* obs, uint32_t l, uint32_t n_landmarks, uint32_t n_obs,
                              uint32_t n_blocks, uint32_t cap, uint32_t* block, uint32_t* feature)
{
    const double w = world[4 * (size_t)l + 3];
    if (w < 0.0) return AKZ_EX_ROW_NO_POINT;
    if (!(w > 0.0)) return AKZ_EX_ROW_INFINITE;
    if (l >= n_landmarks) return AKZ_EX_ROW_BAD;
    const uint32_t s = start[l], e = start[l + 1];
    if (s >= e || e > n_obs) return AKZ_EX_ROW_BAD;                   /* empty, descending, or leaving the table */
    *block = obs[2 * (size_t)s];
    *feature = obs[2 * (size_t)s + 1];
    if (*block >= n_blocks || *feature >= cap) return AKZ_EX_ROW_BAD;
    return AKZ_EX_ROW_POINT;
}
/* Projective::point(): one IEEE division each */
AKZ_RM_FN void akz_ex_point(const double* p, double* xyz)
{
    xyz[0] = p[0] / p[3];
    xyz[1] = p[1] / p[3];
    xyz[2] = p[2] / p[3];
}
/* the verdict of a call */
AKZ_LT_FN uint32_t akz_ex_verdict(int bad_table, uint32_t points, uint32_t room)
{
    return bad_table ? AKZ_EX_BAD_TABLE : points > room ? AKZ_EX_OVERFLOW : AKZ_EX_OK;
}

/* ---- a view's camera (lib.rs:2315-2331) ---- */
/* the features of a view the mean runs over */
AKZ_LT_FN uint32_t akz_ex_count(uint32_t count, uint32_t cap) { return count < cap ? count : cap; }
/* 1 and the distance of feature j's landmark from the camera when the landmark is a row of the world table with a Euclidean
 * point */
AKZ_RM_FN int akz_ex_feature_distance(const double* pose, const uint32_t* landmarks_of_block, uint32_t j, const double* world, uint32_t n_world,
                                      double* distance)
{
    const uint32_t lm = landmarks_of_block[j];
    if (lm >= n_world) return 0;
    return akz_nr_distance(pose, world + 4 * (size_t)lm, distance);
}
/* cam [AKZ_EX_CAMERA_WORDS] from the view's WorldToCamera pose and its mean distance: with c2w = inverse(pose), the optical
 * centre c2w * origin, up = R(c2w) * (0, -1, 0), forward = R(c2w) * (0, 0, 1), focal length = mean * 0.01 */
AKZ_RM_FN void akz_ex_camera(const double* pose, double mean, double* cam)
{
    double c2w[12];
    akz_tv_pose_inverse(pose, c2w);
    AKZ_RM_UNROLL
    for (int i = 0; i < 3; ++i) {
        const double* m = c2w + i * 4;
        cam[i] = ((m[0] * 0.0 + m[1] * 0.0) + m[2] * 0.0) + m[3];
        cam[3 + i] = (m[0] * 0.0 + m[1] * -1.0) + m[2] * 0.0;
        cam[6 + i] = (m[0] * 0.0 + m[1] * 0.0) + m[2] * 1.0;
    }
    cam[9] = mean * 0.01;
}

/* ---- a camera's five vertices (export.rs:95-106) ---- */
/* vertex k < AKZ_EX_CAMERA_VERTICES of the camera: the centre, then up-right, up-left, down-left, down-right */
AKZ_RM_FN void akz_ex_camera_vertex(const double* cam, int k, double* v)
{
    const double* c = cam;
    const double* up = cam + 3;
    const double* fw = cam + 6;
    const double f = cam[9];
    if (k == 0) {
        v[0] = c[0]; v[1] = c[1]; v[2] = c[2];
        return;
    }
    const double u = (k == 1 || k == 2) ? 1.0 : -1.0;                 /* (up, right) = (1, 1), (1, -1), (-1, -1), (-1, 1) */
    const double r = (k == 1 || k == 4) ? 1.0 : -1.0;
    const double right[3] = {fw[1] * up[2] - fw[2] * up[1], fw[2] * up[0] - fw[0] * up[2], fw[0] * up[1] - fw[1] * up[0]};
    AKZ_RM_UNROLL
    for (int i = 0; i < 3; ++i) v[i] = ((c[i] + fw[i] * f) + ((u * up[i]) * f)) + ((r * right[i]) * f);
}
/* channel ch of CAMERA_COLOR {255, 0, 255} (export.rs:11) */
AKZ_LT_FN unsigned char akz_ex_camera_color(int ch) { return ch == 1 ? (unsigned char)0 : (unsigned char)255; }

#if !defined(__HIP_DEVICE_COMPILE__)
/* ---- the host's execution of the whole procedure (the CPU checker's; the kernels' loops one after another) ---- */
#define AKZ_EX_HOST_FN static inline

/* rs_export_reconstruction_device on host arrays (the refusals of the entry point are not restated).  xyz, rgb
 * [5 * n_views + room][3], key [room], cameras [n_views][AKZ_EX_CAMERA_WORDS], counts_out [AKZ_EX_COUNTS], verdict [1]; what the
 * device call does not write is not written here either. */
AKZ_EX_HOST_FN void akz_ex_export(const double* world, uint32_t n_world, const uint32_t* start, const uint32_t* obs, uint32_t n_obs,
                                  uint32_t n_landmarks, const unsigned char* colors, const uint32_t* view_blocks, uint32_t n_views,
                                  const uint32_t* counts, const uint32_t* landmarks, uint32_t cap, uint32_t n_blocks, const double* poses,
                                  uint32_t room, double* xyz, unsigned char* rgb, uint32_t* key, double* cameras, uint32_t* counts_out,
                                  uint32_t* verdict)
{
    /* k_ex_check */
    int bad_table = 0;
    for (uint32_t l = 0; l <= n_landmarks; ++l) bad_table |= akz_ex_start_bad(start, l, n_landmarks, n_obs);
    /* k_ex_tile_sums .. k_ex_points */
    uint32_t n[AKZ_EX_COUNTS] = {0u, 0u, 0u, 0u};
    const size_t first = (size_t)AKZ_EX_CAMERA_VERTICES * n_views;
    if (!bad_table)
        for (uint32_t l = 0; l < n_world; ++l) {
            uint32_t blk = 0u, feat = 0u;
            const uint32_t what = akz_ex_row(world, start, obs, l, n_landmarks, n_obs, n_blocks, cap, &blk, &feat);
            if (what == (uint32_t)AKZ_EX_ROW_POINT && n[0] < room) {
                const size_t at = first + n[0];
                akz_ex_point(world + 4 * (size_t)l, xyz + 3 * at);
                for (int c = 0; c < 3; ++c) rgb[3 * at + c] = colors[3 * ((size_t)blk * cap + feat) + c];
                key[n[0]] = l;
            }
            ++n[what];                                                /* AKZ_EX_ROW_* is the word of its count */
        }
    for (int k = 0; k < AKZ_EX_COUNTS; ++k) counts_out[k] = n[k];
    *verdict = akz_ex_verdict(bad_table, n[0], room);
    /* k_ex_cameras: one workgroup of AKZ_SUM_THREADS per view */
    for (uint32_t v = 0; v < n_views; ++v) {
        const uint32_t block = view_blocks[v], count = akz_ex_count(counts[block], cap);
        const double* pose = poses + (size_t)12 * block;
        double part[AKZ_SUM_THREADS], net;
        uint32_t used = 0;
        for (uint32_t t = 0; t < (uint32_t)AKZ_SUM_THREADS; ++t) {
            part[t] = 0.0;
            for (uint32_t j = t; j < count; j += (uint32_t)AKZ_SUM_THREADS) {
                double d;
                if (!akz_ex_feature_distance(pose, landmarks + (size_t)block * cap, j, world, n_world, &d)) continue;
                part[t] = part[t] + d;
                ++used;
            }
        }
        akz_sum_block(part, 1, &net);
        double* cam = cameras + (size_t)AKZ_EX_CAMERA_WORDS * v;
        akz_ex_camera(pose, akz_nr_mean(net, used), cam);
        for (int k = 0; k < AKZ_EX_CAMERA_VERTICES; ++k) {
            const size_t at = (size_t)AKZ_EX_CAMERA_VERTICES * v + (size_t)k;
            akz_ex_camera_vertex(cam, k, xyz + 3 * at);
            for (int ch = 0; ch < 3; ++ch) rgb[3 * at + ch] = akz_ex_camera_color(ch);
        }
    }
}
#endif /* !__HIP_DEVICE_COMPILE__ */

#endif /* AKZ_EXPORT_MATH_H */
