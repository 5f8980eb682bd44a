// rs_three_view_constraint.hip — the three-view constraints of cv-sfm's pose graph on gfx950: what optimize_three_view does
// behind its shuffle and sort (cv-sfm/src/lib.rs:1939-2062) for n_constraints view triples side by side, each with
// constraint_patience iterations of three_view_adaptive_optimize_l2 (cv-optimize/src/three_view_optimizer.rs:203-272).
// ONE WAVEFRONT PER CONSTRAINT:
//   landmarks        lane l calibrates landmark l's three bearings and keeps the 9 doubles in registers over all iterations;
//                    a copy goes to the wave's own slice of LDS ([9][stride] doubles, component-major), which the
//                    bearing-pair count reads, and from which a lane takes its further landmarks l + 64, l + 128, ... when
//                    more than 64 are used (stride 256 then, 64 otherwise);
//   bearing pairs    all i < j of the used landmarks, the i split over the lanes, an integer count summed by shuffles;
//   optimiser        per iteration a lane adds the 12 gradient components and four norms of its landmark(s), the 16 values
//                    go through the xor butterfly, every lane then holds the same bits and moves the two poses redundantly:
//                    no broadcast, no barrier, no atomic, and for up to 64 landmarks no LDS access either.
// The adaptive optimiser has no early exit, so every accepted constraint of a batch runs the same number of iterations.  A
// refused constraint's wave returns at once.  Every loop is bounded by a parameter (iterations <= RS_TVC_MAX_ITERATIONS,
// landmarks <= RS_TVC_MAX_LANDMARKS); nothing waits on another wave.  The waves of a block share nothing but the block.
//
// The arithmetic is include/akz_three_view_constraint_math.h, the text the CPU checker
// (tests/cpp/three_view_constraint_host.c) compiles too — parity: host build == HIP, bit for bit, the order of the sum over
// landmarks included (fixed in that header).
#include "akz_common.h"
#include "../../include/akz_three_view_constraint_math.h"

#ifndef RS_TVC_BLOCK_WAVES
#define RS_TVC_BLOCK_WAVES 1   // waves (constraints) per block; 4 measured the same (docs/EXPERIMENTS.md #64)
#endif

namespace {

constexpr int kTvcWave = AKZ_TVC_WAVE;
static_assert(AKZ_TVC_WAVE == 64, "akz_wave_sum adds over 64 lanes");
constexpr int kTvcBlock = AKZ_TVC_WAVE * RS_TVC_BLOCK_WAVES;
static_assert(RS_TVC_OK == AKZ_TVC_OK && RS_TVC_FEW_LANDMARKS == AKZ_TVC_FEW_LANDMARKS && RS_TVC_FEW_BEARING_PAIRS == AKZ_TVC_FEW_BEARING_PAIRS &&
              RS_TVC_BAD_INDEX == AKZ_TVC_BAD_INDEX, "verdict values");
static_assert(RS_TVC_STATS == AKZ_TVC_STATS && RS_TVC_S_LANDMARKS == AKZ_TVC_S_LANDMARKS && RS_TVC_S_USED == AKZ_TVC_S_USED &&
              RS_TVC_S_PAIRS == AKZ_TVC_S_PAIRS && RS_TVC_S_ORIGINAL_SCALE == AKZ_TVC_S_ORIGINAL_SCALE &&
              RS_TVC_S_FINAL_SCALE == AKZ_TVC_S_FINAL_SCALE && RS_TVC_S_STAGE == AKZ_TVC_S_STAGE, "stats words");
static_assert(RS_TVC_MAX_LANDMARKS == AKZ_TVC_MAX_LANDMARKS && RS_TVC_MAX_ITERATIONS == AKZ_TVC_MAX_ITERATIONS, "limits");

// all of a constraint's stats words and its verdict, by one lane at the point the verdict falls
__device__ __forceinline__ void tvc_finish(uint32_t* stats, uint32_t* verdict, uint32_t v, uint32_t stage, uint32_t n_list, uint32_t used,
                                           uint32_t pairs, double original_scale, double final_scale)
{
    unsigned long long o, f;
    original_scale = akz_tvc_canonical(original_scale);
    final_scale = akz_tvc_canonical(final_scale);
    __builtin_memcpy(&o, &original_scale, sizeof o);
    __builtin_memcpy(&f, &final_scale, sizeof f);
    stats[AKZ_TVC_S_LANDMARKS] = n_list;
    stats[AKZ_TVC_S_USED] = used;
    stats[AKZ_TVC_S_PAIRS] = pairs;
    stats[AKZ_TVC_S_ORIGINAL_SCALE] = (uint32_t)(o & 0xFFFFFFFFull);
    stats[AKZ_TVC_S_ORIGINAL_SCALE + 1] = (uint32_t)(o >> 32);
    stats[AKZ_TVC_S_FINAL_SCALE] = (uint32_t)(f & 0xFFFFFFFFull);
    stats[AKZ_TVC_S_FINAL_SCALE + 1] = (uint32_t)(f >> 32);
    stats[AKZ_TVC_S_STAGE] = stage;
    *verdict = v;
}

// stride: landmarks a wave's LDS slice has room for per component (64 or RS_TVC_MAX_LANDMARKS; >= the landmarks used).
// Two waves per SIMD: without the bound the compiler takes 262 registers (32 of them AGPRs as spill room) and one wave fits;
// with it 230 VGPRs, still no scratch.  Three waves (168) would spill 130 registers to scratch.
__global__ __launch_bounds__(kTvcBlock, 2) void k_tv_constraints(const akz_keypoint* __restrict__ kps, uint32_t cap, uint32_t n_blocks,
                                                              const double* __restrict__ poses, rs_camera cam,
                                                              const uint32_t* __restrict__ views, const uint32_t* __restrict__ lm_start,
                                                              const uint32_t* __restrict__ lm, uint32_t n_lm, uint32_t n_constraints,
                                                              akz_tvc_settings st, uint32_t stride, double* __restrict__ pose_out,
                                                              uint32_t* __restrict__ verdict, uint32_t* __restrict__ stats_all)
{
    extern __shared__ double tvc_lds[];
    const uint32_t lane = threadIdx.x & (kTvcWave - 1), w = threadIdx.x / kTvcWave;
    const uint32_t s = blockIdx.x * RS_TVC_BLOCK_WAVES + w;
    if (s >= n_constraints) return;
    double* sh = tvc_lds + (size_t)w * 9 * stride;
    uint32_t* stats = stats_all + (size_t)s * AKZ_TVC_STATS;

    // ---- nothing is read through an index before every index of the constraint has been looked at ----
    const uint32_t v0 = views[3 * (size_t)s], v1 = views[3 * (size_t)s + 1], v2 = views[3 * (size_t)s + 2];
    const uint32_t begin = lm_start[s], end = lm_start[s + 1];
    int bad = v0 >= n_blocks || v1 >= n_blocks || v2 >= n_blocks || begin > end || end > n_lm;
    const uint32_t n_list = bad ? 0u : end - begin;
    const uint32_t* list = lm + 3 * (size_t)(bad ? 0u : begin);
    for (size_t i = lane; i < 3 * (size_t)n_list; i += kTvcWave) bad |= list[i] >= cap;
    if (__any(bad)) {
        if (lane == 0) tvc_finish(stats, verdict + s, AKZ_TVC_BAD_INDEX, AKZ_TVC_STAGE_INDEX, 0u, 0u, 0u, 0.0, 0.0);
        return;
    }
    if (n_list < st.optimization_minimum_landmarks) {
        if (lane == 0) tvc_finish(stats, verdict + s, AKZ_TVC_FEW_LANDMARKS, AKZ_TVC_STAGE_LANDMARKS, n_list, 0u, 0u, 0.0, 0.0);
        return;
    }

    // ---- the relative poses (lib.rs:1956-1966) ----
    double rel[24];
    {
        double wp[36];
#pragma unroll
        for (int k = 0; k < 12; ++k) {
            wp[k] = poses[(size_t)12 * v0 + k];
            wp[12 + k] = poses[(size_t)12 * v1 + k];
            wp[24 + k] = poses[(size_t)12 * v2 + k];
        }
        akz_tvc_relative_poses(wp, wp + 12, wp + 24, rel);
    }
    const double original_scale = akz_tvc_scale_of(rel);

    // ---- take(optimization_maximum_landmarks) (lib.rs:1980-1990): the bearings, mine in registers, all in LDS ----
    const uint32_t used = n_list < st.optimization_maximum_landmarks ? n_list : st.optimization_maximum_landmarks;   // <= stride
    double b0[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) b0[k] = 0.0;
    for (uint32_t i = lane; i < used; i += kTvcWave) {
        double b[9];
        const uint32_t blk[3] = {v0, v1, v2};
#pragma unroll
        for (int v = 0; v < 3; ++v) {
            const akz_keypoint& kp = kps[(size_t)blk[v] * cap + list[3 * (size_t)i + v]];
            akz_tri_calibrate(&cam.fx, cam.use_k1, cam.k1, kp.x, kp.y, b + 3 * v);
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            sh[k * stride + i] = b[k];
            if (i == lane) b0[k] = b[k];
        }
    }
    // (a wave's LDS accesses complete in order: what lane a wrote above, lane b reads below without a barrier)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

    // ---- the robust bearing pairs (lib.rs:2011-2032) ----
    uint32_t mine = 0;
    for (uint32_t i = lane; i < used; i += kTvcWave) {
        double a[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) a[k] = sh[k * stride + i];
        for (uint32_t j = i + 1; j < used; ++j) {
            double b[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) b[k] = sh[k * stride + j];
            mine += akz_tv_bearing_pair_robust(a, a + 3, a + 6, b, b + 3, b + 6, st.robust_view_bearing_pair_minimum_cosine_distance) ? 1u : 0u;
        }
    }
    const uint32_t pairs = akz_wave_sum(mine);
    if (pairs < st.robust_view_num_robust_bearing_pair) {
        if (lane == 0) tvc_finish(stats, verdict + s, AKZ_TVC_FEW_BEARING_PAIRS, AKZ_TVC_STAGE_PAIRS, n_list, used, pairs, original_scale, 0.0);
        return;
    }

    // ---- three_view_adaptive_optimize_l2 (three_view_optimizer.rs:203-272) ----
    if (used != 0) {
        double inv[24];
        const double inv_len = 1.0 / (double)used;
        akz_tv_pose_inverse(rel, inv);
        akz_tv_pose_inverse(rel + 12, inv + 12);
        for (uint32_t it = 0; it < st.constraint_patience; ++it) {
            double part[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) part[k] = 0.0;
            if (lane < used) akz_tvc_accumulate(inv, b0, b0 + 3, b0 + 6, part);
            for (uint32_t i = lane + kTvcWave; i < used; i += kTvcWave) {
                double b[9];
#pragma unroll
                for (int k = 0; k < 9; ++k) b[k] = sh[k * stride + i];
                akz_tvc_accumulate(inv, b, b + 3, b + 6, part);
            }
            akz_wave_sum(part);
            akz_tvc_adaptive_step(part, inv_len, inv);
        }
        akz_tv_pose_inverse(inv, rel);
        akz_tv_pose_inverse(inv + 12, rel + 12);
    }

    // ---- back to the original scale (lib.rs:2045-2052) ----
    const double final_scale = akz_tvc_scale_of(rel);
    const double relative_scale = original_scale / final_scale;
    akz_tv_pose_scale(rel, relative_scale);
    akz_tv_pose_scale(rel + 12, relative_scale);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 24; ++k) pose_out[(size_t)24 * s + k] = akz_tvc_canonical(rel[k]);
        tvc_finish(stats, verdict + s, AKZ_TVC_OK, AKZ_TVC_STAGE_FINAL, n_list, used, pairs, original_scale, final_scale);
    }
}

int32_t tvc_settings(const rs_three_view_constraint_params* prm, akz_tvc_settings* st)
{
    if (!prm || prm->struct_size != sizeof(rs_three_view_constraint_params)) return AKZ_E_INVALID;
    if (prm->robust_view_bearing_pair_minimum_cosine_distance != prm->robust_view_bearing_pair_minimum_cosine_distance) return AKZ_E_INVALID;
    if (prm->optimization_maximum_landmarks > (uint32_t)RS_TVC_MAX_LANDMARKS) return AKZ_E_TOO_LARGE;
    st->robust_view_bearing_pair_minimum_cosine_distance = prm->robust_view_bearing_pair_minimum_cosine_distance;
    st->optimization_minimum_landmarks = prm->optimization_minimum_landmarks;
    st->optimization_maximum_landmarks = prm->optimization_maximum_landmarks;
    // the bound that makes the running time finite: more iterations than RS_TVC_MAX_ITERATIONS count as that
    st->constraint_patience = prm->constraint_patience < (uint32_t)RS_TVC_MAX_ITERATIONS ? prm->constraint_patience : (uint32_t)RS_TVC_MAX_ITERATIONS;
    st->robust_view_num_robust_bearing_pair = prm->robust_view_num_robust_bearing_pair;
    return AKZ_OK;
}

}   // namespace

extern "C" int32_t rs_three_view_constraint_params_default(rs_three_view_constraint_params* prm)
{
    if (!prm) return AKZ_E_INVALID;
    prm->struct_size = sizeof(rs_three_view_constraint_params);
    prm->optimization_minimum_landmarks = 24;                              // cv-sfm/src/settings.rs:465-483
    prm->optimization_maximum_landmarks = 64;
    prm->constraint_patience = 1u << 12;
    prm->robust_view_num_robust_bearing_pair = 3;                          // settings.rs:332-338
    prm->robust_view_bearing_pair_minimum_cosine_distance = 1e-2;
    return AKZ_OK;
}

extern "C" int32_t rs_three_view_constraint_batch_device(rs_ctx* c, const void* d_kps, uint32_t cap_per_img, uint32_t n_blocks,
                                                         const void* d_poses, const rs_camera* cam, const void* d_views,
                                                         const void* d_lm_start, const void* d_lm, uint32_t n_lm, uint32_t n_constraints,
                                                         const rs_three_view_constraint_params* prm, void* d_pose_out, void* d_verdict,
                                                         void* d_stats, void* stream_to_wait)
{
    return akz_guard([&]() -> int32_t {
        akz_tvc_settings st;
        AKZ_TRY(tvc_settings(prm, &st));
        if (!c || !d_kps || !d_poses || !cam || !d_views || !d_lm_start || (n_lm != 0 && !d_lm) || !d_pose_out || !d_verdict || !d_stats)
            return AKZ_E_INVALID;
        if (cap_per_img == 0 || n_blocks == 0 || cam->reserved != 0) return AKZ_E_INVALID;
        if (n_constraints == 0) return AKZ_OK;
        const RsHandles h = rs_internal_handles(c);
        AKZ_TRY(akz_enqueue_behind(h, stream_to_wait));
        const uint32_t stride = st.optimization_maximum_landmarks <= (uint32_t)kTvcWave ? (uint32_t)kTvcWave : (uint32_t)RS_TVC_MAX_LANDMARKS;
        const size_t lds = sizeof(double) * 9 * stride * RS_TVC_BLOCK_WAVES;
        const uint32_t grid = (n_constraints + RS_TVC_BLOCK_WAVES - 1) / RS_TVC_BLOCK_WAVES;
#if RS_TVC_BLOCK_WAVES > 3
        if (lds > 65536) AKZ_HIP(hipFuncSetAttribute((const void*)k_tv_constraints, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
#endif
        hipLaunchKernelGGL(k_tv_constraints, dim3(grid), dim3(kTvcBlock), lds, h.stream, (const akz_keypoint*)d_kps, cap_per_img, n_blocks,
                           (const double*)d_poses, *cam, (const uint32_t*)d_views, (const uint32_t*)d_lm_start, (const uint32_t*)d_lm, n_lm,
                           n_constraints, st, stride, (double*)d_pose_out, (uint32_t*)d_verdict, (uint32_t*)d_stats);
        AKZ_LAUNCH_CHECK();
        return AKZ_OK;
    });
}
