// rs_three_view.hip — the three-view bootstrap of a reconstruction on gfx950: everything cv-sfm's init_reconstruction does
// between the poses of its two consensuses and the three frames it returns (cv-sfm/src/lib.rs:1002-1300), for n_scenes
// triples side by side.  One persistent workgroup of 256 threads per triple, one launch, no host step between the stages:
//   classification   one lane per common match (a 4 x 4 eigen-problem for the three-observation point, two more for the
//                    depth ratios in the first pass), 256 matches at a time in list order;
//   take(n)          ordered compaction of each 256: ballot, popcount prefix inside the wave, the waves' counts through
//                    LDS — no atomic decides an order;
//   median           rank counting over the FloatOrd keys in LDS (any exact selection gives the same element);
//   bearing pairs    all i < j of the chosen landmarks, an integer count;
//   optimiser        the chosen landmarks ([9][1024] doubles, 72 KB of LDS, component-major so that a wave reads consecutive
//                    doubles) stay put over all iterations of all runs; per iteration every thread sums its landmarks'
//                    gradients, the wave butterflies, lane 0 of each wave leaves 12 doubles in LDS, ONE barrier, and every
//                    thread adds the four in wave order and moves the poses redundantly (same bits in, same bits out: no
//                    broadcast, no second barrier; the 2 x 4 x 12 buffer alternates by iteration parity).
// Every loop is bounded by a parameter (iterations <= RS_TV_MAX_ITERATIONS); nothing waits on another workgroup.
//
// The arithmetic is include/akz_three_view_math.h, the text the CPU checker (tests/cpp/three_view_host.c) compiles too —
// parity: host build == HIP, bit for bit, the order of the sum over landmarks included (fixed in that header).
#include "akz_common.h"
#include "../../include/akz_three_view_math.h"

namespace {

constexpr int kTvBlock = AKZ_TV_THREADS;
constexpr int kTvWaves = AKZ_TV_THREADS / AKZ_TV_WAVE;
static_assert(AKZ_TV_WAVE == 64, "akz_wave_sum adds over 64 lanes");
static_assert(RS_TV_STATS == AKZ_TV_STATS && RS_TV_MAX_COMMON * sizeof(unsigned long long) <= 9 * AKZ_TV_MAX_LANDMARKS * sizeof(double),
              "the ratio keys of the first pass live where the landmarks go afterwards");
static_assert(RS_TV_OK == AKZ_TV_OK && RS_TV_FEW_SCALES == AKZ_TV_FEW_SCALES && RS_TV_FEW_BEARING_PAIRS == AKZ_TV_FEW_BEARING_PAIRS &&
              RS_TV_FEW_MATCHES == AKZ_TV_FEW_MATCHES && RS_TV_LOST_HALF == AKZ_TV_LOST_HALF && RS_TV_FEW_ROBUST == AKZ_TV_FEW_ROBUST &&
              RS_TV_BAD_INDEX == AKZ_TV_BAD_INDEX, "verdict values");

struct TvShared {
    double lm[9 * AKZ_TV_MAX_LANDMARKS];   // landmarks, component-major; the first pass keeps its u64 ratio keys here
    double red[2][kTvWaves][12];           // the waves' gradient sums, by iteration parity
    uint32_t cnt[2][kTvWaves];             // the waves' counts of a compaction step, by step parity
    double median;
};

struct TvScene {
    const akz_keypoint *kc, *kf, *ks;   // the three keypoint blocks
    const uint32_t *triples, *first_only, *second_only;
    uint32_t n, n_first, n_second;
    const rs_camera* cam;
};
__device__ __forceinline__ void tv_bearing(const TvScene& sc, const akz_keypoint* blk, uint32_t feat, double* b)
{
    akz_tri_calibrate(&sc.cam->fx, sc.cam->use_k1, sc.cam->k1, blk[feat].x, blk[feat].y, b);
}
__device__ __forceinline__ void tv_match(const TvScene& sc, uint32_t i, double* c, double* f, double* s)
{
    tv_bearing(sc, sc.kc, sc.triples[3 * (size_t)i], c);
    tv_bearing(sc, sc.kf, sc.triples[3 * (size_t)i + 1], f);
    tv_bearing(sc, sc.ks, sc.triples[3 * (size_t)i + 2], s);
}

// The first `limit` passing matches in list order into sh.lm (lib.rs:1064-1083, 1140-1159).  Matches behind the last one
// taken are not looked at, as the reference's lazy iterator does not.
__device__ uint32_t tv_take(TvShared& sh, uint32_t& tick, const TvScene& sc, const double* poses, double max_cos, const akz_tv_settings& st)
{
    const uint32_t limit = st.three_view_optimization_landmarks;
    uint32_t m = 0;
    for (uint32_t base = 0; base < sc.n && m < limit; base += kTvBlock) {
        const uint32_t i = base + threadIdx.x;
        double c[3], f[3], s[3];
        bool ok = false;
        if (i < sc.n) {
            tv_match(sc, i, c, f, s);
            ok = akz_tv_tri_landmark_robust(poses, poses + 12, c, f, s, max_cos, st.robust_observation_incidence_minimum_cosine_distance, &st.tri);
        }
        uint32_t total;
        const uint32_t slot = m + akz_block_scan(sh.cnt, tick, ok, &total);
        if (ok && slot < limit) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                sh.lm[k * AKZ_TV_MAX_LANDMARKS + slot] = c[k];
                sh.lm[(3 + k) * AKZ_TV_MAX_LANDMARKS + slot] = f[k];
                sh.lm[(6 + k) * AKZ_TV_MAX_LANDMARKS + slot] = s[k];
            }
        }
        m += total;
    }
    __syncthreads();
    return m < limit ? m : limit;
}

// three_view_simple_optimize_l2 (three_view_optimizer.rs:126-200) on the n landmarks of sh.lm; poses [2][12] in and out.
__device__ uint32_t tv_optimize(TvShared& sh, double* poses, double rate, uint32_t iterations, uint32_t n)
{
    double inv[24];
    akz_tv_opt_state os;
    uint32_t it = 0;
    if (n == 0) return 0;
    const double scale = (1.0 / (double)n) * rate;
    akz_tv_pose_inverse(poses, inv);
    akz_tv_pose_inverse(poses + 12, inv + 12);
    akz_tv_opt_begin(&os);
    for (; it < iterations; ++it) {
        double part[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) part[k] = 0.0;
        for (uint32_t i = threadIdx.x; i < n; i += kTvBlock) {
            double c[3], f[3], s[3], g[12];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                c[k] = sh.lm[k * AKZ_TV_MAX_LANDMARKS + i];
                f[k] = sh.lm[(3 + k) * AKZ_TV_MAX_LANDMARKS + i];
                s[k] = sh.lm[(6 + k) * AKZ_TV_MAX_LANDMARKS + i];
            }
            akz_tv_landmark_gradients(inv, c, f, s, g);
#pragma unroll
            for (int k = 0; k < 12; ++k) part[k] = part[k] + g[k];
        }
        double nets[12];
        akz_block_sum(sh.red, it, part, nets);
        if (akz_tv_opt_step(&os, nets, scale, inv, it, iterations)) break;
    }
    akz_tv_pose_inverse(inv, poses);
    akz_tv_pose_inverse(inv + 12, poses + 12);
    return it;
}

__global__ __launch_bounds__(kTvBlock) void k_three_view(const akz_keypoint* __restrict__ kps, uint32_t cap, uint32_t n_blocks,
                                                         const uint32_t* __restrict__ frames, uint32_t frames_stride, rs_camera cam,
                                                         const double* __restrict__ pose_first, const double* __restrict__ pose_second,
                                                         const uint32_t* __restrict__ triples, const uint32_t* __restrict__ ntriples,
                                                         const uint32_t* __restrict__ first_only, const uint32_t* __restrict__ nfirst,
                                                         const uint32_t* __restrict__ second_only, const uint32_t* __restrict__ nsecond,
                                                         akz_tv_settings st, double* __restrict__ pose_out, uint32_t* __restrict__ verdict,
                                                         unsigned char* __restrict__ combined, unsigned char* __restrict__ first_ok,
                                                         unsigned char* __restrict__ second_ok, uint32_t* __restrict__ stats_all)
{
    __shared__ TvShared sh;
    const uint32_t s = blockIdx.x, tid = threadIdx.x;
    uint32_t* stats = stats_all + (size_t)s * AKZ_TV_STATS;
    uint32_t tick = 0;
    if (tid < (uint32_t)AKZ_TV_STATS) stats[tid] = (tid >= (uint32_t)AKZ_TV_S_RUN_MATCHES && tid < (uint32_t)AKZ_TV_S_ROBUST) ? 0xFFFFFFFFu : 0u;
    if (tid == 0) sh.median = 0.0;

    const uint32_t bc = frames[s], bf = frames[frames_stride + s], bs = frames[2 * (size_t)frames_stride + s];
    TvScene sc;
    sc.cam = &cam;
    sc.n = ntriples[s] < cap ? ntriples[s] : cap;
    sc.n_first = nfirst[s] < cap ? nfirst[s] : cap;
    sc.n_second = nsecond[s] < cap ? nsecond[s] : cap;
    sc.triples = triples + (size_t)s * cap * 3;
    sc.first_only = first_only + (size_t)s * cap * 2;
    sc.second_only = second_only + (size_t)s * cap * 2;

    // ---- nothing is read through an index before every index of the scene has been looked at ----
    int bad = bc >= n_blocks || bf >= n_blocks || bs >= n_blocks;
    for (uint32_t i = tid; i < 3 * sc.n; i += kTvBlock) bad |= sc.triples[i] >= cap;
    for (uint32_t i = tid; i < 2 * sc.n_first; i += kTvBlock) bad |= sc.first_only[i] >= cap;
    for (uint32_t i = tid; i < 2 * sc.n_second; i += kTvBlock) bad |= sc.second_only[i] >= cap;
    if (__syncthreads_or(bad)) {
        if (tid == 0) verdict[s] = AKZ_TV_BAD_INDEX;
        return;
    }
    sc.kc = kps + (size_t)bc * cap;
    sc.kf = kps + (size_t)bf * cap;
    sc.ks = kps + (size_t)bs * cap;

    double poses[24];
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        poses[k] = pose_first[(size_t)12 * s + k];
        poses[12 + k] = pose_second[(size_t)12 * s + k];
    }

    // ---- the depth ratios (lib.rs:1002-1038) ----
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(sh.lm);
    uint32_t n_scales = 0;
    for (uint32_t base = 0; base < sc.n; base += kTvBlock) {
        const uint32_t i = base + tid;
        double ratio = 0.0;
        bool ok = false;
        if (i < sc.n) {
            double c[3], f[3], b[3];
            tv_match(sc, i, c, f, b);
            ok = akz_tv_relative_scale(poses, poses + 12, c, f, b, &st, &ratio);
        }
        uint32_t total;
        const uint32_t slot = n_scales + akz_block_scan(sh.cnt, tick, ok, &total);
        if (ok) keys[slot] = akz_tri_float_ord(ratio);
        n_scales += total;
    }
    __syncthreads();
    if (tid == 0) {
        stats[AKZ_TV_S_SCALES] = n_scales;
        stats[AKZ_TV_S_STAGE] = AKZ_TV_STAGE_SCALES;
    }
    if (n_scales < st.three_view_minimum_relative_scales) {
        if (tid == 0) verdict[s] = AKZ_TV_FEW_SCALES;
        return;
    }
    // ---- the median (lib.rs:1050-1059): exactly one key has rank len / 2 ----
    for (uint32_t i = tid; i < n_scales; i += kTvBlock)
        if (akz_tv_rank(keys, n_scales, i) == n_scales / 2u) sh.median = AKZ_RM_SQRT(akz_tv_key_value(keys[i]));
    __syncthreads();
    const double median = sh.median;
    if (tid == 0) {
        unsigned long long u;
        __builtin_memcpy(&u, &median, sizeof u);
        stats[AKZ_TV_S_MEDIAN_LO] = (uint32_t)(u & 0xFFFFFFFFull);
        stats[AKZ_TV_S_MEDIAN_HI] = (uint32_t)(u >> 32);
    }
    akz_tv_pose_scale(poses + 12, median);

    // ---- the optimisation matches and their robust bearing pairs (lib.rs:1064-1106) ----
    uint32_t n_opt = tv_take(sh, tick, sc, poses, 1.0, st);
    uint32_t mine = 0;
    for (uint32_t i = tid; i < n_opt; i += kTvBlock) {
        double a[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) a[k] = sh.lm[k * AKZ_TV_MAX_LANDMARKS + i];
        for (uint32_t j = i + 1; j < n_opt; ++j) {
            double b[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) b[k] = sh.lm[k * AKZ_TV_MAX_LANDMARKS + j];
            mine += akz_tv_bearing_pair_robust(a, a + 3, a + 6, b, b + 3, b + 6, st.robust_view_bearing_pair_minimum_cosine_distance) ? 1u : 0u;
        }
    }
    const uint32_t pairs = akz_block_sum(sh.cnt, tick, mine);
    if (tid == 0) {
        stats[AKZ_TV_S_PAIRS] = pairs;
        stats[AKZ_TV_S_STAGE] = AKZ_TV_STAGE_PAIRS;
    }
    if (pairs < st.robust_view_num_robust_bearing_pair) {
        if (tid == 0) verdict[s] = AKZ_TV_FEW_BEARING_PAIRS;
        return;
    }

    // ---- optimise, filter again, ... (lib.rs:1108-1187): a fixed trip count, a rejected triple simply stops ----
    const uint32_t robust_minimum_matches = n_opt / 2u;
    for (uint32_t run = 0; run <= st.three_view_filter_loop_iterations; ++run) {
        if (tid == 0) {
            stats[AKZ_TV_S_STAGE] = AKZ_TV_STAGE_RUN0 + run;
            stats[AKZ_TV_S_RUN_MATCHES + run] = n_opt;
        }
        if (n_opt < st.hard_minimum_matches || n_opt <= robust_minimum_matches) {
            if (tid == 0) verdict[s] = n_opt < st.hard_minimum_matches ? AKZ_TV_FEW_MATCHES : AKZ_TV_LOST_HALF;
            return;
        }
        const uint32_t stop = tv_optimize(sh, poses, st.optimization_rate, st.three_view_patience, n_opt);
        if (tid == 0) stats[AKZ_TV_S_RUN_STOP + run] = stop;
        if (run < st.three_view_filter_loop_iterations) n_opt = tv_take(sh, tick, sc, poses, st.maximum_cosine_distance, st);
    }

    // ---- the final counts and masks (lib.rs:1193-1292) ----
    uint32_t robust = 0;
    for (uint32_t base = 0; base < sc.n; base += kTvBlock) {
        const uint32_t i = base + tid;
        bool ok = false;
        if (i < sc.n) {
            double c[3], f[3], b[3];
            tv_match(sc, i, c, f, b);
            ok = akz_tv_tri_landmark_robust(poses, poses + 12, c, f, b, st.maximum_cosine_distance,
                                            st.robust_observation_incidence_minimum_cosine_distance, &st.tri);
        }
        uint32_t total;
        akz_block_scan(sh.cnt, tick, ok, &total);
        robust += total;
    }
    if (tid == 0) {
        stats[AKZ_TV_S_ROBUST] = robust;
        stats[AKZ_TV_S_STAGE] = AKZ_TV_STAGE_FINAL;
    }
    if (robust <= robust_minimum_matches || robust < st.three_view_minimum_robust_matches) {
        if (tid == 0) verdict[s] = robust <= robust_minimum_matches ? AKZ_TV_LOST_HALF : AKZ_TV_FEW_ROBUST;
        return;
    }
    for (uint32_t i = tid; i < sc.n; i += kTvBlock) {
        double c[3], f[3], b[3];
        tv_match(sc, i, c, f, b);
        combined[(size_t)s * cap + i] = (unsigned char)akz_tv_tri_landmark_robust(poses, poses + 12, c, f, b, st.maximum_cosine_distance, 0.0, &st.tri);
    }
    for (uint32_t i = tid; i < sc.n_first; i += kTvBlock) {
        double a[3], b[3];
        tv_bearing(sc, sc.kc, sc.first_only[2 * (size_t)i], a);
        tv_bearing(sc, sc.kf, sc.first_only[2 * (size_t)i + 1], b);
        first_ok[(size_t)s * cap + i] = (unsigned char)akz_tv_bi_landmark_robust(poses, a, b, st.maximum_sine_distance);
    }
    for (uint32_t i = tid; i < sc.n_second; i += kTvBlock) {
        double a[3], b[3];
        tv_bearing(sc, sc.kc, sc.second_only[2 * (size_t)i], a);
        tv_bearing(sc, sc.ks, sc.second_only[2 * (size_t)i + 1], b);
        second_ok[(size_t)s * cap + i] = (unsigned char)akz_tv_bi_landmark_robust(poses + 12, a, b, st.maximum_sine_distance);
    }
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < 24; ++k) pose_out[(size_t)24 * s + k] = poses[k];
        verdict[s] = AKZ_TV_OK;
    }
}

int32_t tv_settings(const rs_three_view_params* prm, akz_tv_settings* st)
{
    if (!prm || prm->struct_size != sizeof(rs_three_view_params)) return AKZ_E_INVALID;
    AKZ_TRY(akz_tri_settings_from(prm->triangulate, &st->tri));
    const double d[5] = {prm->maximum_cosine_distance, prm->maximum_sine_distance, prm->robust_observation_incidence_minimum_cosine_distance,
                         prm->robust_view_bearing_pair_minimum_cosine_distance, prm->optimization_rate};
    for (double x : d)
        if (!AKZ_TRI_FINITE(x)) return AKZ_E_INVALID;
    if (prm->three_view_filter_loop_iterations >= (uint32_t)RS_TV_MAX_RUNS) return AKZ_E_INVALID;
    if (prm->three_view_optimization_landmarks > (uint32_t)RS_TV_MAX_LANDMARKS) return AKZ_E_TOO_LARGE;
    st->maximum_cosine_distance = prm->maximum_cosine_distance;
    st->maximum_sine_distance = prm->maximum_sine_distance;
    st->robust_observation_incidence_minimum_cosine_distance = prm->robust_observation_incidence_minimum_cosine_distance;
    st->robust_view_bearing_pair_minimum_cosine_distance = prm->robust_view_bearing_pair_minimum_cosine_distance;
    st->optimization_rate = prm->optimization_rate;
    st->robust_view_num_robust_bearing_pair = prm->robust_view_num_robust_bearing_pair;
    st->three_view_minimum_relative_scales = prm->three_view_minimum_relative_scales;
    st->three_view_filter_loop_iterations = prm->three_view_filter_loop_iterations;
    st->three_view_optimization_landmarks = prm->three_view_optimization_landmarks;
    // the bound that makes the running time finite: more iterations than RS_TV_MAX_ITERATIONS count as that
    st->three_view_patience = prm->three_view_patience < (uint32_t)RS_TV_MAX_ITERATIONS ? prm->three_view_patience : (uint32_t)RS_TV_MAX_ITERATIONS;
    st->three_view_minimum_robust_matches = prm->three_view_minimum_robust_matches;
    st->hard_minimum_matches = prm->hard_minimum_matches;
    return AKZ_OK;
}

}   // namespace

extern "C" int32_t rs_three_view_params_default(rs_three_view_params* prm)
{
    if (!prm) return AKZ_E_INVALID;
    prm->struct_size = sizeof(rs_three_view_params);
    prm->robust_view_num_robust_bearing_pair = 3;                          // cv-sfm/src/settings.rs:320-427
    prm->maximum_cosine_distance = 1e-5;
    prm->maximum_sine_distance = 1e-1;
    prm->robust_observation_incidence_minimum_cosine_distance = 1e-3;
    prm->robust_view_bearing_pair_minimum_cosine_distance = 1e-2;
    prm->optimization_rate = 0.001;                                        // the literal of lib.rs:1133, 1182
    prm->three_view_minimum_relative_scales = 16;
    prm->three_view_filter_loop_iterations = 8;
    prm->three_view_optimization_landmarks = 1024;
    prm->three_view_patience = 65536;
    prm->three_view_minimum_robust_matches = 32;
    prm->hard_minimum_matches = 32;                                        // the literal of lib.rs:1118, 1167
    return rs_triangulate_params_default(&prm->triangulate);
}

extern "C" int32_t rs_three_view_init_batch_device(rs_ctx* c, const void* d_kps, uint32_t cap_per_img, uint32_t n_blocks, const uint32_t* ic,
                                                   const uint32_t* i_first, const uint32_t* i_second, const rs_camera* cam,
                                                   const void* d_pose_first, const void* d_pose_second, const void* d_triples,
                                                   const void* d_ntriples, const void* d_first_only, const void* d_nfirst,
                                                   const void* d_second_only, const void* d_nsecond, uint32_t n_scenes,
                                                   const rs_three_view_params* prm, void* d_pose_out, void* d_verdict, void* d_combined,
                                                   void* d_first_ok, void* d_second_ok, void* d_stats, void* stream_to_wait)
{
    return akz_guard([&]() -> int32_t {
        akz_tv_settings st;
        AKZ_TRY(tv_settings(prm, &st));
        if (!c || !d_kps || !ic || !i_first || !i_second || !cam || !d_pose_first || !d_pose_second || !d_triples || !d_ntriples ||
            !d_first_only || !d_nfirst || !d_second_only || !d_nsecond || !d_pose_out || !d_verdict || !d_combined || !d_first_ok ||
            !d_second_ok || !d_stats)
            return AKZ_E_INVALID;
        if (cap_per_img == 0 || n_blocks == 0 || cam->reserved != 0 || n_scenes > 65535u) return AKZ_E_INVALID;
        if (cap_per_img > (uint32_t)RS_TV_MAX_COMMON) return AKZ_E_TOO_LARGE;
        if (n_scenes == 0) return AKZ_OK;
        const RsHandles h = rs_internal_handles(c);
        if (h.max_scenes == 0) return AKZ_E_INVALID;              // a context without its batch arena (rs_batch_reserve failed)
        if (n_scenes > h.max_scenes) return AKZ_E_TOO_LARGE;
        AKZ_TRY(akz_enqueue_behind(h, stream_to_wait));
        // the frame lists go where the consensus keeps its own: stream order puts the copies behind that call's last reader
        AKZ_HIP(hipMemcpyAsync(h.d_frames, ic, sizeof(uint32_t) * n_scenes, hipMemcpyHostToDevice, h.stream));
        AKZ_HIP(hipMemcpyAsync(h.d_frames + h.max_scenes, i_first, sizeof(uint32_t) * n_scenes, hipMemcpyHostToDevice, h.stream));
        AKZ_HIP(hipMemcpyAsync(h.d_frames + 2 * (size_t)h.max_scenes, i_second, sizeof(uint32_t) * n_scenes, hipMemcpyHostToDevice, h.stream));
        hipLaunchKernelGGL(k_three_view, dim3(n_scenes), dim3(kTvBlock), 0, h.stream, (const akz_keypoint*)d_kps, cap_per_img, n_blocks,
                           (const uint32_t*)h.d_frames, h.max_scenes, *cam, (const double*)d_pose_first, (const double*)d_pose_second,
                           (const uint32_t*)d_triples, (const uint32_t*)d_ntriples, (const uint32_t*)d_first_only, (const uint32_t*)d_nfirst,
                           (const uint32_t*)d_second_only, (const uint32_t*)d_nsecond, st, (double*)d_pose_out, (uint32_t*)d_verdict,
                           (unsigned char*)d_combined, (unsigned char*)d_first_ok, (unsigned char*)d_second_ok, (uint32_t*)d_stats);
        AKZ_LAUNCH_CHECK();
        return AKZ_OK;
    });
}
