// rs_triangulate.hip — the table of world points the registration chain reads, and the points of a two-view consensus'
// inliers, made on gfx950.  One independent 4 x 4 symmetric eigen-problem per landmark (or per inlier), one problem per
// lane, registers only: the design matrix (upper 10 entries) and the 16 eigenvector components never leave the register
// file, no LDS, no scratch (tools/check_isa.py holds the compiled kernels to that).
//
// Reference code implemented here (paths relative to rust-cv/cv); the arithmetic is include/akz_triangulate_math.h, the
// text the CPU checker (tests/cpp/triangulate_host.c) compiles too — parity: host build == HIP, bit for bit:
//   LinearEigenTriangulator::triangulate_observations        cv-geom/src/triangulation.rs:82-130      all kernels
//   VSlam::triangulate_landmark_robust                       cv-sfm/src/lib.rs:2990-3000, 2907-2934   k_tri_landmarks
//   VSlam::triangulate_merged_landmark_robust                cv-sfm/src/lib.rs:2958-2972              k_tri_merged
//   TriangulatorRelative::triangulate_relative on inliers    cv-sfm/src/lib.rs:1023-1029, 1332;
//                                                            cv-core/src/triangulation.rs:21-36, 52-67 k_tri_pairs
// A landmark's observations are {block, feature} pairs in a CSR list (the caller's landmark graph); the lane gathers
// keypoint -> calibrated bearing (CameraIntrinsics::calibrate, as the batched consensus does) and the block's pose.
#include "akz_common.h"
#include "../../include/akz_triangulate_math.h"

namespace {

constexpr int kTriBlock = 256;

// where a lane's observations come from: list A = obs[s0 .. s0 + n0), followed (merge candidates) by obs[s1 ..)
struct TriSrc {
    const uint32_t* obs;        // [n_obs][2] {block, feature}
    const akz_keypoint* kps;    // [n_blocks][cap]
    const double* poses;        // [n_blocks][12] WorldToCamera, row-major [R | t]
    const rs_camera* cam;
    uint32_t s0, n0, s1, cap, n_blocks;
};
__device__ __forceinline__ int tri_fetch(const TriSrc* s, unsigned i, double* pose, double* b)
{
    const size_t at = i < s->n0 ? (size_t)s->s0 + i : (size_t)s->s1 + (i - s->n0);
    const uint32_t blk = s->obs[2 * at], feat = s->obs[2 * at + 1];
    if (blk >= s->n_blocks || feat >= s->cap) return 0;
    const akz_keypoint* kp = s->kps + (size_t)blk * s->cap + feat;
    akz_tri_calibrate(&s->cam->fx, s->cam->use_k1, s->cam->k1, kp->x, kp->y, b);
    const double* p = s->poses + (size_t)12 * blk;
#pragma unroll
    for (int k = 0; k < 12; ++k) pose[k] = p[k];
    return 1;
}
AKZ_TRI_DEFINE_TRIANGULATE(tri_list, TriSrc, tri_fetch)

// the two observations of a two-view inlier: (identity, a), (pose, b)  (cv-core/src/triangulation.rs:31-34)
struct TriPairSrc {
    double a[3], b[3];
    const double* pose;
};
__device__ __forceinline__ int tri_pair_fetch(const TriPairSrc* s, unsigned i, double* pose, double* b)
{
#pragma unroll
    for (int k = 0; k < 12; ++k) pose[k] = i == 0 ? ((k == 0 || k == 5 || k == 10) ? 1.0 : 0.0) : s->pose[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) b[k] = i == 0 ? s->a[k] : s->b[k];
    return 1;
}
AKZ_TRI_DEFINE_TRIANGULATE(tri_pair, TriPairSrc, tri_pair_fetch)

// observations handed over as arrays (rs_triangulate_observations)
struct TriArraySrc {
    const double* poses;     // [n][12]
    const double* bearings;  // [n][3]
};
__device__ __forceinline__ int tri_array_fetch(const TriArraySrc* s, unsigned i, double* pose, double* b)
{
#pragma unroll
    for (int k = 0; k < 12; ++k) pose[k] = s->poses[(size_t)12 * i + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) b[k] = s->bearings[(size_t)3 * i + k];
    return 1;
}
AKZ_TRI_DEFINE_TRIANGULATE(tri_array, TriArraySrc, tri_array_fetch)

__device__ __forceinline__ void tri_store(double* __restrict__ world, unsigned char* __restrict__ reason, size_t row, size_t reason_at,
                                          const double* p, int why)
{
    double2* w = reinterpret_cast<double2*>(world + 4 * row);
    w[0] = make_double2(p[0], p[1]);
    w[1] = make_double2(p[2], p[3]);
    if (reason) reason[reason_at] = (unsigned char)why;
}

// A CSR range that does not lie inside the observation array is the caller's error: reason 6, nothing read.
__device__ __forceinline__ bool tri_range(const uint32_t* __restrict__ start, uint32_t l, uint32_t n_obs, uint32_t* s, uint32_t* n)
{
    const uint32_t a = start[l], b = start[l + 1];
    *s = a;
    *n = b >= a ? b - a : 0u;
    return a <= b && b <= n_obs;
}

// One lane per landmark: row l of the world table = triangulate_landmark_robust(l).
__global__ __launch_bounds__(kTriBlock) void k_tri_landmarks(const akz_keypoint* __restrict__ kps, uint32_t cap, uint32_t n_blocks,
                                                             const double* __restrict__ poses, rs_camera cam,
                                                             const uint32_t* __restrict__ obs_start, const uint32_t* __restrict__ obs,
                                                             uint32_t n_obs, uint32_t n_landmarks, akz_tri_settings st,
                                                             double* __restrict__ world, unsigned char* __restrict__ reason)
{
    const uint32_t l = blockIdx.x * kTriBlock + threadIdx.x;
    if (l >= n_landmarks) return;
    TriSrc src;
    src.obs = obs; src.kps = kps; src.poses = poses; src.cam = &cam;
    src.cap = cap; src.n_blocks = n_blocks; src.s1 = 0;
    double p[4];
    int why = AKZ_TRI_BAD_INDEX;
    akz_tri_none(p);
    if (tri_range(obs_start, l, n_obs, &src.s0, &src.n0)) why = tri_list(&src, src.n0, 1, &st, p);
    tri_store(world, reason, l, l, p, why);
}

// One lane per (frame slot, feature): a merge candidate (decision 2) the caller's graph test admitted gets row
// n_world + f * cap + j = triangulate_merged_landmark_robust([best0, best1]): the observations of best0 followed by those
// of best1 (lib.rs:2958-2972); every other row of that range is left alone.
__global__ __launch_bounds__(kTriBlock) void k_tri_merged(const akz_keypoint* __restrict__ kps, uint32_t cap, uint32_t n_blocks,
                                                          const double* __restrict__ poses, rs_camera cam,
                                                          const uint32_t* __restrict__ obs_start, const uint32_t* __restrict__ obs,
                                                          uint32_t n_obs, uint32_t n_landmarks, akz_tri_settings st,
                                                          const uint2* __restrict__ best, const uint32_t* __restrict__ decision,
                                                          const unsigned char* __restrict__ merge_ok, uint32_t n_world,
                                                          double* __restrict__ world, unsigned char* __restrict__ reason)
{
    const uint32_t j = blockIdx.x * kTriBlock + threadIdx.x, f = blockIdx.y;
    if (j >= cap) return;
    const size_t fj = (size_t)f * cap + j;
    if (decision[fj] != 2u || !merge_ok[fj]) return;
    const uint32_t l0 = best[fj * 3].x, l1 = best[fj * 3 + 1].x;
    TriSrc src;
    src.obs = obs; src.kps = kps; src.poses = poses; src.cam = &cam;
    src.cap = cap; src.n_blocks = n_blocks;
    double p[4];
    int why = AKZ_TRI_BAD_INDEX;
    akz_tri_none(p);
    uint32_t n1 = 0;
    if (l0 < n_landmarks && l1 < n_landmarks && tri_range(obs_start, l0, n_obs, &src.s0, &src.n0) &&
        tri_range(obs_start, l1, n_obs, &src.s1, &n1))
        why = tri_list(&src, src.n0 + n1, 1, &st, p);
    tri_store(world, reason, (size_t)n_world + fj, fj, p, why);
}

// One lane per (scene, inlier): the CameraPoint of inlier i of scene s, triangulate_relative(pose_s, a, b).  A scene
// without a model writes nothing.
__global__ __launch_bounds__(kTriBlock) void k_tri_pairs(const akz_keypoint* __restrict__ kps_a, const akz_keypoint* __restrict__ kps_b,
                                                         uint32_t cap, const uint32_t* __restrict__ fa, const uint32_t* __restrict__ fb,
                                                         const uint32_t* __restrict__ pairs, const uint32_t* __restrict__ npairs,
                                                         rs_camera cam_a, rs_camera cam_b, const double* __restrict__ pose,
                                                         const uint32_t* __restrict__ best_id, const uint32_t* __restrict__ inliers,
                                                         const uint32_t* __restrict__ n_inliers, akz_tri_settings st,
                                                         double* __restrict__ points, unsigned char* __restrict__ reason)
{
    const uint32_t i = blockIdx.x * kTriBlock + threadIdx.x, s = blockIdx.y;
    if (i >= cap || best_id[s] == 0xFFFFFFFFu) return;
    uint32_t ni = n_inliers[s], np = npairs[s];
    ni = ni < cap ? ni : cap;
    np = np < cap ? np : cap;
    if (i >= ni) return;
    const size_t si = (size_t)s * cap + i;
    double p[4];
    int why = AKZ_TRI_BAD_INDEX;
    akz_tri_none(p);
    const uint32_t m = inliers[si];
    if (m < np) {
        const uint32_t ia = pairs[((size_t)s * cap + m) * 2], ib = pairs[((size_t)s * cap + m) * 2 + 1];
        if (ia < cap && ib < cap) {
            TriPairSrc src;
            const akz_keypoint* ka = kps_a + (size_t)fa[s] * cap + ia;
            const akz_keypoint* kb = kps_b + (size_t)fb[s] * cap + ib;
            akz_tri_calibrate(&cam_a.fx, cam_a.use_k1, cam_a.k1, ka->x, ka->y, src.a);
            akz_tri_calibrate(&cam_b.fx, cam_b.use_k1, cam_b.k1, kb->x, kb->y, src.b);
            src.pose = pose + (size_t)12 * s;
            why = tri_pair(&src, 2u, 0, &st, p);
        }
    }
    tri_store(points, reason, si, si, p, why);
}

// one list handed over as arrays, one lane (rs_triangulate_observations); robustness not applied
__global__ void k_tri_observations(const double* __restrict__ poses, const double* __restrict__ bearings, uint32_t n, akz_tri_settings st,
                                   double* __restrict__ point, unsigned char* __restrict__ reason)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    TriArraySrc src;
    src.poses = poses;
    src.bearings = bearings;
    double p[4];
    const int why = tri_array(&src, n, 0, &st, p);
    tri_store(point, reason, 0, 0, p, why);
}

int32_t tri_settings(const rs_triangulate_params* prm, akz_tri_settings* st)
{
    if (!prm) return AKZ_E_INVALID;
    AKZ_TRY(akz_tri_settings_from(*prm, st));
    return AKZ_TRI_FINITE(prm->incidence_minimum_cosine_distance) ? AKZ_OK : AKZ_E_INVALID;
}

}   // namespace

extern "C" int32_t rs_triangulate_params_default(rs_triangulate_params* prm)
{
    if (!prm) return AKZ_E_INVALID;
    prm->struct_size = sizeof(rs_triangulate_params);
    prm->max_sweeps = 1000;                              // LinearEigenTriangulator::default (triangulation.rs:73-80)
    prm->eps = 1e-12;
    prm->robust_minimum_observations = 3;                // cv-sfm/src/settings.rs:344-350
    prm->n_views = 0xFFFFFFFFu;                          // (the min() of lib.rs:2913-2917 then is robust_minimum_observations)
    prm->incidence_minimum_cosine_distance = 1e-3;
    return AKZ_OK;
}

extern "C" int32_t rs_triangulate_observations(rs_ctx* c, const double* poses, const double* bearings, uint32_t n,
                                               const rs_triangulate_params* prm, double* point, uint8_t* reason)
{
    return akz_guard([&]() -> int32_t {
        akz_tri_settings st;
        if (!c || !point || (n != 0 && (!poses || !bearings))) return AKZ_E_INVALID;
        AKZ_TRY(tri_settings(prm, &st));
        const RsHandles h = rs_internal_handles(c);
        AKZ_HIP(hipSetDevice(h.device));
        // one allocation for the call: [n][12] poses, [n][3] bearings, the point, the reason byte; freed on every way out
        struct Scratch {
            double* d = nullptr;
            ~Scratch() { if (d) hipFree(d); }
        } buf;
        const size_t m = n ? n : 1;
        AKZ_HIP(hipMalloc(&buf.d, sizeof(double) * (15 * m + 5)));
        double *d_p = buf.d, *d_b = d_p + 12 * m, *d_o = d_b + 3 * m;
        unsigned char* d_r = reinterpret_cast<unsigned char*>(d_o + 4);
        if (n) {
            AKZ_HIP(hipMemcpyAsync(d_p, poses, sizeof(double) * 12 * n, hipMemcpyHostToDevice, h.stream));
            AKZ_HIP(hipMemcpyAsync(d_b, bearings, sizeof(double) * 3 * n, hipMemcpyHostToDevice, h.stream));
        }
        hipLaunchKernelGGL(k_tri_observations, dim3(1), dim3(64), 0, h.stream, d_p, d_b, n, st, d_o, d_r);
        AKZ_LAUNCH_CHECK();
        double out[5];
        AKZ_HIP(hipMemcpyAsync(out, d_o, sizeof(out), hipMemcpyDeviceToHost, h.stream));
        AKZ_HIP(hipStreamSynchronize(h.stream));
        for (int k = 0; k < 4; ++k) point[k] = out[k];
        if (reason) memcpy(reason, &out[4], 1);
        return AKZ_OK;
    });
}

extern "C" int32_t rs_triangulate_landmarks_device(rs_ctx* c, const void* d_kps, uint32_t cap_per_img, uint32_t n_blocks,
                                                   const void* d_poses, const rs_camera* cam, const void* d_obs_start, const void* d_obs,
                                                   uint32_t n_obs, uint32_t n_landmarks, const rs_triangulate_params* prm, void* d_world,
                                                   void* d_reason, void* stream_to_wait)
{
    return akz_guard([&]() -> int32_t {
        akz_tri_settings st;
        if (!c || !d_kps || !d_poses || !cam || !d_obs_start || (n_obs != 0 && !d_obs) || !d_world) return AKZ_E_INVALID;
        if (cap_per_img == 0 || n_blocks == 0 || cam->reserved != 0) return AKZ_E_INVALID;
        AKZ_TRY(tri_settings(prm, &st));
        if (n_landmarks == 0) return AKZ_OK;
        const RsHandles h = rs_internal_handles(c);
        AKZ_TRY(akz_enqueue_behind(h, stream_to_wait));
        hipLaunchKernelGGL(k_tri_landmarks, dim3((n_landmarks + kTriBlock - 1) / kTriBlock), dim3(kTriBlock), 0, h.stream,
                           (const akz_keypoint*)d_kps, cap_per_img, n_blocks, (const double*)d_poses, *cam, (const uint32_t*)d_obs_start,
                           (const uint32_t*)d_obs, n_obs, n_landmarks, st, (double*)d_world, (unsigned char*)d_reason);
        AKZ_LAUNCH_CHECK();
        return AKZ_OK;
    });
}

extern "C" int32_t rs_triangulate_merged_device(rs_ctx* c, const void* d_kps, uint32_t cap_per_img, uint32_t n_blocks,
                                                const void* d_poses, const rs_camera* cam, const void* d_obs_start, const void* d_obs,
                                                uint32_t n_obs, uint32_t n_landmarks, const rs_triangulate_params* prm, const void* d_best,
                                                const void* d_decision, const void* d_merge_ok, uint32_t n_frames, uint32_t n_world,
                                                void* d_world, void* d_reason, void* stream_to_wait)
{
    return akz_guard([&]() -> int32_t {
        akz_tri_settings st;
        if (!c || !d_kps || !d_poses || !cam || !d_obs_start || (n_obs != 0 && !d_obs) || !d_world || !d_best || !d_decision || !d_merge_ok)
            return AKZ_E_INVALID;
        if (cap_per_img == 0 || n_blocks == 0 || cam->reserved != 0 || n_frames > 65535u) return AKZ_E_INVALID;
        AKZ_TRY(tri_settings(prm, &st));
        if (n_frames == 0) return AKZ_OK;
        const RsHandles h = rs_internal_handles(c);
        AKZ_TRY(akz_enqueue_behind(h, stream_to_wait));
        hipLaunchKernelGGL(k_tri_merged, dim3((cap_per_img + kTriBlock - 1) / kTriBlock, n_frames), dim3(kTriBlock), 0, h.stream,
                           (const akz_keypoint*)d_kps, cap_per_img, n_blocks, (const double*)d_poses, *cam, (const uint32_t*)d_obs_start,
                           (const uint32_t*)d_obs, n_obs, n_landmarks, st, (const uint2*)d_best, (const uint32_t*)d_decision,
                           (const unsigned char*)d_merge_ok, n_world, (double*)d_world, (unsigned char*)d_reason);
        AKZ_LAUNCH_CHECK();
        return AKZ_OK;
    });
}

extern "C" int32_t rs_triangulate_pairs_batch_device(rs_ctx* c, const void* d_kps_a, const void* d_kps_b, uint32_t cap_per_img,
                                                     const uint32_t* ia, const uint32_t* ib, const void* d_pairs, const void* d_npairs,
                                                     uint32_t n_scenes, const rs_camera* cam_a, const rs_camera* cam_b, const void* d_pose,
                                                     const void* d_best_id, const void* d_inliers, const void* d_n_inliers,
                                                     const rs_triangulate_params* prm, void* d_points, void* d_reason, void* stream_to_wait)
{
    return akz_guard([&]() -> int32_t {
        akz_tri_settings st;
        if (!c || !d_kps_a || !d_kps_b || !ia || !ib || !d_pairs || !d_npairs || !cam_a || !cam_b || !d_pose || !d_best_id || !d_inliers ||
            !d_n_inliers || !d_points)
            return AKZ_E_INVALID;
        if (cap_per_img == 0 || cam_a->reserved != 0 || cam_b->reserved != 0 || n_scenes > 65535u) return AKZ_E_INVALID;
        AKZ_TRY(tri_settings(prm, &st));
        if (n_scenes == 0) return AKZ_OK;
        const RsHandles h = rs_internal_handles(c);
        if (h.max_scenes == 0) return AKZ_E_INVALID;              // a context without its batch arena (rs_batch_reserve failed)
        if (n_scenes > h.max_scenes) return AKZ_E_TOO_LARGE;
        AKZ_TRY(akz_enqueue_behind(h, stream_to_wait));
        // the frame lists go where the consensus keeps its own: stream order puts the copy behind that call's last reader
        AKZ_HIP(hipMemcpyAsync(h.d_frames, ia, sizeof(uint32_t) * n_scenes, hipMemcpyHostToDevice, h.stream));
        AKZ_HIP(hipMemcpyAsync(h.d_frames + h.max_scenes, ib, sizeof(uint32_t) * n_scenes, hipMemcpyHostToDevice, h.stream));
        hipLaunchKernelGGL(k_tri_pairs, dim3((cap_per_img + kTriBlock - 1) / kTriBlock, n_scenes), dim3(kTriBlock), 0, h.stream,
                           (const akz_keypoint*)d_kps_a, (const akz_keypoint*)d_kps_b, cap_per_img, (const uint32_t*)h.d_frames,
                           (const uint32_t*)(h.d_frames + h.max_scenes), (const uint32_t*)d_pairs, (const uint32_t*)d_npairs, *cam_a, *cam_b,
                           (const double*)d_pose, (const uint32_t*)d_best_id, (const uint32_t*)d_inliers, (const uint32_t*)d_n_inliers, st,
                           (double*)d_points, (unsigned char*)d_reason);
        AKZ_LAUNCH_CHECK();
        return AKZ_OK;
    });
}
