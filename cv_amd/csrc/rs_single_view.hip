// rs_single_view.hip — the refinement of registered poses on gfx950: everything cv-sfm's register_frame_subset does between
// its consensus and the pose and match map it returns (cv-sfm/src/lib.rs:1625-1775), for the new frames of a micro-batch side
// by side.  One persistent workgroup of 256 threads per scene, one launch, no host step between the stages:
//   indices          every match, landmark, observation range and observation of the scene is looked at before anything is
//                    read through one; a scene that names something outside the caller's arrays is refused alone;
//   inliers          the consensus counts its matches without the "None" rows: an ordered compaction of the original list
//                    (ballot, popcount prefix inside the wave, the waves' counts through LDS) gives every robust match its
//                    place, and the first num_matches inliers are gathered through it;
//   consistency      one lane per original match, 256 at a time in list order: the design matrix and the eigenvectors of
//                    the 4 x 4 problem stay in registers, observations are fetched again rather than held;
//   take(n)          the same ordered compaction; matches behind the last one taken are not looked at;
//   optimiser        the chosen matches ([6][2048] doubles, 96 KB of LDS, component-major so that a wave reads consecutive
//                    doubles) stay put over all iterations of a run; per iteration every thread sums its matches' gradients,
//                    the wave butterflies, lane 0 of each wave leaves 6 doubles in LDS, ONE barrier, and every thread adds the
//                    four in wave order and moves the pose redundantly (same bits in, same bits out: no broadcast, no second
//                    barrier; the 2 x 4 x 6 buffer alternates by iteration parity).
// Every loop is bounded by a parameter (iterations <= RS_SV_MAX_ITERATIONS); nothing waits on another workgroup.
//
// The arithmetic is include/akz_single_view_math.h, the text the CPU checker (tests/cpp/single_view_host.c) compiles too —
// parity: host build == HIP, bit for bit, the order of the sum over matches included (fixed in that header).
#include "akz_common.h"
#include "../../include/akz_single_view_math.h"

namespace {

constexpr int kSvBlock = AKZ_SV_THREADS;
constexpr int kSvWaves = AKZ_SV_THREADS / AKZ_SV_WAVE;
static_assert(AKZ_SV_WAVE == 64, "akz_wave_sum adds over 64 lanes");
static_assert(RS_SV_STATS == AKZ_SV_STATS && RS_SV_MAX_MATCHES == AKZ_SV_MAX_MATCHES && RS_SV_MAX_RUNS == AKZ_SV_MAX_RUNS, "limits");
static_assert(RS_SV_OK == AKZ_SV_OK && RS_SV_NO_MODEL == AKZ_SV_NO_MODEL && RS_SV_FEW_LANDMARKS == AKZ_SV_FEW_LANDMARKS &&
              RS_SV_LOST_HALF == AKZ_SV_LOST_HALF && RS_SV_FEW_ROBUST == AKZ_SV_FEW_ROBUST && RS_SV_BAD_INDEX == AKZ_SV_BAD_INDEX,
              "verdict values");
static_assert(RS_SV_S_INLIERS == AKZ_SV_S_INLIERS && RS_SV_S_RUN_MATCHES == AKZ_SV_S_RUN_MATCHES && RS_SV_S_RUN_STOP == AKZ_SV_S_RUN_STOP &&
              RS_SV_S_ROBUST == AKZ_SV_S_ROBUST && RS_SV_S_NO_OTHER == AKZ_SV_S_NO_OTHER && RS_SV_S_STAGE == AKZ_SV_S_STAGE, "stats words");

struct SvShared {
    double lm[6 * AKZ_SV_MAX_MATCHES];   // chosen matches, component-major: bearing xyz, point xyz
    double red[2][kSvWaves][6];          // the waves' gradient sums, by iteration parity
    uint32_t cnt[2][kSvWaves];           // the waves' counts of a compaction step, by step parity
};

// everything the kernel takes, by value
struct SvCall {
    const akz_keypoint* kps;
    const double* poses;          // [n_blocks][12]
    const uint32_t* obs_start;    // [n_landmarks + 1]
    const uint32_t* obs;          // [n_obs][2]
    const double* world;          // [n_rows][4]
    const uint32_t* frames;       // [n_scenes] the new frames' blocks
    const uint32_t* matches;      // [n_scenes][cap][2]
    const uint32_t* nmatches;
    const uint32_t* best;         // [n_scenes][cap][3][2] or null
    const double* pose;
    const uint32_t* best_id;
    const uint32_t* inliers;
    const uint32_t* n_inliers;
    double* pose_out;
    uint32_t* verdict;
    unsigned char* final_mask;
    uint32_t* n_final;
    uint32_t* stats;
    uint32_t* place;              // scratch [n_scenes][cap]: the original index of the k-th match with a world point
    uint32_t cap, n_blocks, n_obs, n_landmarks, n_world, n_rows;
};

// An original match: its feature, its world row and the observation ranges of its one or two landmarks.
struct SvMatch {
    uint32_t feat, row, s0, n0, s1, n1;
};
// false: the match names a feature, a world row, a landmark or an observation range outside the caller's arrays
__device__ __forceinline__ bool sv_resolve(const SvCall& a, const uint32_t* m, uint32_t i, SvMatch* o)
{
    o->feat = m[2 * (size_t)i];
    o->row = m[2 * (size_t)i + 1];
    o->s0 = 0; o->n0 = 0; o->s1 = 0; o->n1 = 0;
    if (o->feat >= a.cap || o->row >= a.n_rows) return false;
    uint32_t l0 = o->row;
    if (o->row >= a.n_world) {                       // a merged match (n_rows > n_world only with a.best)
        const size_t e = (size_t)(o->row - a.n_world) * 3;
        l0 = a.best[2 * e];
        const uint32_t l1 = a.best[2 * (e + 1)];
        if (l1 >= a.n_landmarks) return false;
        const uint32_t s = a.obs_start[l1], t = a.obs_start[l1 + 1];
        if (s > t || t > a.n_obs) return false;
        o->s1 = s; o->n1 = t - s;
    }
    if (l0 >= a.n_landmarks) return false;
    const uint32_t s = a.obs_start[l0], t = a.obs_start[l0 + 1];
    if (s > t || t > a.n_obs) return false;
    o->s0 = s; o->n0 = t - s;
    return true;
}

// the observations of a match as akz_single_view_math.h wants them: the others, then (pose, bearing) itself
struct SvSrc {
    const uint32_t* obs;
    const akz_keypoint* kps;
    const double* poses;
    const rs_camera* cam;
    uint32_t s0, n0, s1, k, cap, n_blocks;
    double pose[12], bearing[3];  // by value: a pointer to the caller's registers would put them in scratch
};
__device__ __forceinline__ int sv_fetch(const SvSrc* s, unsigned i, double* pose, double* b)
{
    if (i >= s->k) {
#pragma unroll
        for (int k = 0; k < 12; ++k) pose[k] = s->pose[k];
        b[0] = s->bearing[0]; b[1] = s->bearing[1]; b[2] = s->bearing[2];
        return 1;
    }
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
AKZ_TRI_DEFINE_TRIANGULATE(sv_triangulate, SvSrc, sv_fetch)
AKZ_SV_DEFINE_CONSISTENT(sv_consistent_src, SvSrc, sv_fetch, sv_triangulate)

struct SvScene {
    const akz_keypoint* kn;       // the new frame's keypoints
    const uint32_t* m;            // its original matches
    uint32_t n;
};
__device__ __forceinline__ void sv_bearing(const SvScene& sc, const rs_camera& cam, uint32_t feat, double* b)
{
    akz_tri_calibrate(&cam.fx, cam.use_k1, cam.k1, sc.kn[feat].x, sc.kn[feat].y, b);
}
__device__ __forceinline__ bool sv_consistent(const SvCall& a, const rs_camera& cam, const SvMatch& mt, const double* pose, const double* b,
                                              const akz_sv_settings& st)
{
    SvSrc src;
    src.obs = a.obs; src.kps = a.kps; src.poses = a.poses; src.cam = &cam;
    src.s0 = mt.s0; src.n0 = mt.n0; src.s1 = mt.s1; src.k = mt.n0 + mt.n1; src.cap = a.cap; src.n_blocks = a.n_blocks;
#pragma unroll
    for (int k = 0; k < 12; ++k) src.pose[k] = pose[k];
    src.bearing[0] = b[0]; src.bearing[1] = b[1]; src.bearing[2] = b[2];
    return sv_consistent_src(&src, src.k, pose, b, &st) != 0;
}
__device__ __forceinline__ void sv_put(SvShared& sh, uint32_t slot, const double* b, const double* world)
{
    double x[3];
    akz_sv_point(world, x);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        sh.lm[k * AKZ_SV_MAX_MATCHES + slot] = b[k];
        sh.lm[(3 + k) * AKZ_SV_MAX_MATCHES + slot] = x[k];
    }
}

// The first `limit` original matches in list order that are consistent under `pose` and have a world point, into sh.lm
// (lib.rs:1664-1693).  Matches behind the last one taken are not looked at, as the reference's lazy iterator does not.
__device__ uint32_t sv_take(SvShared& sh, uint32_t& tick, const SvCall& a, const rs_camera& cam, const SvScene& sc, const double* pose,
                            const akz_sv_settings& st)
{
    const uint32_t limit = st.single_view_optimization_num_matches;
    uint32_t m = 0;
    for (uint32_t base = 0; base < sc.n && m < limit; base += kSvBlock) {
        const uint32_t i = base + threadIdx.x;
        double b[3] = {0.0, 0.0, 0.0};
        const double* w = a.world;
        bool ok = false;
        if (i < sc.n) {
            SvMatch mt;
            sv_resolve(a, sc.m, i, &mt);                 // the prologue saw every match: it resolves
            w = a.world + 4 * (size_t)mt.row;
            if (akz_sv_some(w)) {
                sv_bearing(sc, cam, mt.feat, b);
                ok = sv_consistent(a, cam, mt, pose, b, st);
            }
        }
        uint32_t total;
        const uint32_t slot = m + akz_block_scan(sh.cnt, tick, ok, &total);
        if (ok && slot < limit) sv_put(sh, slot, b, w);
        m += total;
    }
    __syncthreads();
    return m < limit ? m : limit;
}

// single_view_simple_optimize_l2 (single_view_optimizer.rs:80-135) on the n matches of sh.lm; pose [12] in and out.
__device__ uint32_t sv_optimize(SvShared& sh, double* pose, double rate, uint32_t iterations, uint32_t n)
{
    akz_sv_opt_state os;
    uint32_t it = 0;
    if (n == 0) return 0;
    const double inv_landmark_len = 1.0 / (double)n;
    akz_sv_opt_begin(&os);
    for (; it < iterations; ++it) {
        double part[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) part[k] = 0.0;
        for (uint32_t i = threadIdx.x; i < n; i += kSvBlock) {
            double b[3], x[3], g[6];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                b[k] = sh.lm[k * AKZ_SV_MAX_MATCHES + i];
                x[k] = sh.lm[(3 + k) * AKZ_SV_MAX_MATCHES + i];
            }
            if (akz_sv_landmark_delta(pose, b, x, g)) {
#pragma unroll
                for (int k = 0; k < 6; ++k) part[k] = part[k] + g[k];
            }
        }
        double net[6];
        akz_block_sum(sh.red, it, part, net);
        if (akz_sv_opt_step(&os, net, inv_landmark_len, rate, pose, it, iterations)) break;
    }
    return it;
}

__global__ __launch_bounds__(kSvBlock) void k_single_view(SvCall a, rs_camera cam, akz_sv_settings st)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char sv_lds[];
    SvShared& sh = *reinterpret_cast<SvShared*>(sv_lds);
    const uint32_t s = blockIdx.x, tid = threadIdx.x;
    uint32_t* stats = a.stats + (size_t)s * AKZ_SV_STATS;
    uint32_t tick = 0;
    if (tid < (uint32_t)AKZ_SV_STATS) stats[tid] = (tid >= (uint32_t)AKZ_SV_S_RUN_MATCHES && tid < (uint32_t)AKZ_SV_S_ROBUST) ? 0xFFFFFFFFu : 0u;
    if (tid == 0) a.n_final[s] = 0u;

    SvScene sc;
    const uint32_t bn = a.frames[s];
    sc.n = a.nmatches[s] < a.cap ? a.nmatches[s] : a.cap;
    sc.m = a.matches + (size_t)s * a.cap * 2;
    sc.kn = a.kps;

    // ---- nothing is read through an index before every index of the scene has been looked at ----
    int bad = bn >= a.n_blocks;
    uint32_t mine = 0;
    for (uint32_t i = tid; i < sc.n; i += kSvBlock) {
        SvMatch mt;
        if (!sv_resolve(a, sc.m, i, &mt)) {
            bad = 1;
            continue;
        }
        mine += mt.n0 + mt.n1 == 0u ? 1u : 0u;
        for (uint32_t k = 0; k < mt.n0 + mt.n1; ++k) {
            const size_t at = k < mt.n0 ? (size_t)mt.s0 + k : (size_t)mt.s1 + (k - mt.n0);
            bad |= a.obs[2 * at] >= a.n_blocks || a.obs[2 * at + 1] >= a.cap;
        }
    }
    if (__syncthreads_or(bad)) {
        if (tid == 0) a.verdict[s] = AKZ_SV_BAD_INDEX;
        return;
    }
    sc.kn = a.kps + (size_t)bn * a.cap;
    const uint32_t no_other = akz_block_sum(sh.cnt, tick, mine);

    // ---- the list the consensus saw: the matches with a world point, in order ----
    uint32_t* place = a.place + (size_t)s * a.cap;
    uint32_t n_rob = 0;
    for (uint32_t base = 0; base < sc.n; base += kSvBlock) {
        const uint32_t i = base + tid;
        const bool some = i < sc.n && akz_sv_some(a.world + 4 * (size_t)sc.m[2 * (size_t)i + 1]);
        uint32_t total;
        const uint32_t slot = n_rob + akz_block_scan(sh.cnt, tick, some, &total);
        if (some) place[slot] = i;
        n_rob += total;
    }
    __syncthreads();                                  // the places are written before any is read
    if (tid == 0) {
        stats[AKZ_SV_S_NO_OTHER] = no_other;
        stats[AKZ_SV_S_STAGE] = AKZ_SV_STAGE_LANDMARKS;
    }
    if (n_rob < st.single_view_minimum_landmarks) {
        if (tid == 0) a.verdict[s] = AKZ_SV_FEW_LANDMARKS;
        return;
    }
    double pose[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) pose[k] = a.pose[(size_t)12 * s + k];
    if (a.best_id[s] == 0xFFFFFFFFu) {
        if (tid == 0) {
#pragma unroll
            for (int k = 0; k < 12; ++k) a.pose_out[(size_t)12 * s + k] = pose[k];
            stats[AKZ_SV_S_STAGE] = AKZ_SV_STAGE_MODEL;
            a.verdict[s] = AKZ_SV_NO_MODEL;
        }
        return;
    }

    // ---- take(num_matches) of the inliers (lib.rs:1626-1630) ----
    const uint32_t* inl = a.inliers + (size_t)s * a.cap;
    uint32_t n_opt = a.n_inliers[s] < a.cap ? a.n_inliers[s] : a.cap;
    n_opt = n_opt < st.single_view_optimization_num_matches ? n_opt : st.single_view_optimization_num_matches;
    for (uint32_t k = tid; k < n_opt; k += kSvBlock) bad |= inl[k] >= n_rob;
    if (__syncthreads_or(bad)) {
        if (tid == 0) {
            stats[AKZ_SV_S_STAGE] = AKZ_SV_STAGE_INDEX;
            a.verdict[s] = AKZ_SV_BAD_INDEX;
        }
        return;
    }
    for (uint32_t k = tid; k < n_opt; k += kSvBlock) {
        const uint32_t i = place[inl[k]];
        double b[3];
        sv_bearing(sc, cam, sc.m[2 * (size_t)i], b);
        sv_put(sh, k, b, a.world + 4 * (size_t)sc.m[2 * (size_t)i + 1]);
    }
    __syncthreads();
    if (tid == 0) stats[AKZ_SV_S_INLIERS] = n_opt;

    // ---- optimise, select again, ... and the last optimisation (lib.rs:1636-1710): a rejected scene simply stops ----
    const uint32_t robust_minimum_matches = n_opt / 2u;
    for (uint32_t run = 0; run <= st.single_view_filter_loop_iterations; ++run) {
        if (tid == 0) {
            stats[AKZ_SV_S_STAGE] = AKZ_SV_STAGE_RUN0 + run;
            stats[AKZ_SV_S_RUN_MATCHES + run] = n_opt;
        }
        if (n_opt <= robust_minimum_matches) {
            if (tid == 0) a.verdict[s] = AKZ_SV_LOST_HALF;
            return;
        }
        const uint32_t stop = sv_optimize(sh, pose, st.single_view_optimization_rate, st.single_view_patience, n_opt);
        if (tid == 0) stats[AKZ_SV_S_RUN_STOP + run] = stop;
        if (run < st.single_view_filter_loop_iterations) n_opt = sv_take(sh, tick, a, cam, sc, pose, st);
    }

    // ---- the final pass (lib.rs:1712-1772): the consistent flag once, both counts from it ----
    uint32_t robust = 0, n_final = 0;
    for (uint32_t i = tid; i < sc.n; i += kSvBlock) {
        SvMatch mt;
        double b[3];
        sv_resolve(a, sc.m, i, &mt);
        sv_bearing(sc, cam, mt.feat, b);
        const bool ok = sv_consistent(a, cam, mt, pose, b, st);
        a.final_mask[(size_t)s * a.cap + i] = ok ? 1 : 0;
        n_final += ok ? 1u : 0u;
        robust += ok && akz_sv_some(a.world + 4 * (size_t)mt.row) ? 1u : 0u;
    }
    robust = akz_block_sum(sh.cnt, tick, robust);
    n_final = akz_block_sum(sh.cnt, tick, n_final);
    if (tid == 0) {
        unsigned stage;
        const int v = akz_sv_final_verdict(robust, n_final, robust_minimum_matches, st.single_view_minimum_robust_landmarks, &stage);
        a.n_final[s] = n_final;
        stats[AKZ_SV_S_ROBUST] = robust;
        stats[AKZ_SV_S_STAGE] = stage;
        if (v == AKZ_SV_OK) {
#pragma unroll
            for (int k = 0; k < 12; ++k) a.pose_out[(size_t)12 * s + k] = pose[k];
        }
        a.verdict[s] = (uint32_t)v;
    }
}

int32_t sv_settings(const rs_single_view_params* prm, akz_sv_settings* st)
{
    if (!prm || prm->struct_size != sizeof(rs_single_view_params)) return AKZ_E_INVALID;
    // (robust_minimum_observations is copied and not read: the consistency test has no robustness test)
    AKZ_TRY(akz_tri_settings_from(prm->triangulate, &st->tri));
    if (prm->maximum_cosine_distance != prm->maximum_cosine_distance || prm->maximum_sine_distance != prm->maximum_sine_distance ||
        !AKZ_TRI_FINITE(prm->single_view_optimization_rate))
        return AKZ_E_INVALID;
    if (prm->single_view_optimization_num_matches > (uint32_t)RS_SV_MAX_MATCHES) return AKZ_E_TOO_LARGE;
    if (prm->single_view_filter_loop_iterations >= (uint32_t)RS_SV_MAX_RUNS) return AKZ_E_TOO_LARGE;
    st->maximum_cosine_distance = prm->maximum_cosine_distance;
    st->maximum_sine_distance = prm->maximum_sine_distance;
    st->single_view_optimization_rate = prm->single_view_optimization_rate;
    st->single_view_optimization_num_matches = prm->single_view_optimization_num_matches;
    st->single_view_filter_loop_iterations = prm->single_view_filter_loop_iterations;
    // the bound that makes the running time finite: more iterations than RS_SV_MAX_ITERATIONS count as that
    st->single_view_patience = prm->single_view_patience < (uint32_t)RS_SV_MAX_ITERATIONS ? prm->single_view_patience : (uint32_t)RS_SV_MAX_ITERATIONS;
    st->single_view_minimum_landmarks = prm->single_view_minimum_landmarks;
    st->single_view_minimum_robust_landmarks = prm->single_view_minimum_robust_landmarks;
    return AKZ_OK;
}

}   // namespace

extern "C" int32_t rs_single_view_params_default(rs_single_view_params* prm)
{
    if (!prm) return AKZ_E_INVALID;
    prm->struct_size = sizeof(rs_single_view_params);
    prm->single_view_optimization_num_matches = 2048;              // cv-sfm/src/settings.rs:357-359
    prm->single_view_filter_loop_iterations = 5;                   // settings.rs:361-363
    prm->single_view_patience = 100000;                            // settings.rs:365-367
    prm->single_view_optimization_rate = 1e-3;                     // settings.rs:373-375
    prm->single_view_minimum_landmarks = 32;                       // settings.rs:377-379
    prm->single_view_minimum_robust_landmarks = 64;                // settings.rs:381-383
    prm->maximum_cosine_distance = 1e-5;                           // settings.rs:324-326
    prm->maximum_sine_distance = 1e-1;                             // settings.rs:328-330
    return rs_triangulate_params_default(&prm->triangulate);
}

extern "C" int32_t rs_refine_poses_batch_device(rs_ctx* c, const void* d_kps, uint32_t cap_per_img, uint32_t n_blocks, const void* d_poses,
                                                const rs_camera* cam, const void* d_obs_start, const void* d_obs, uint32_t n_obs,
                                                uint32_t n_landmarks, const void* d_world, uint32_t n_world, const uint32_t* ik,
                                                const void* d_matches, const void* d_nmatches, const void* d_best, const void* d_pose,
                                                const void* d_best_id, const void* d_inliers, const void* d_n_inliers, uint32_t n_scenes,
                                                const rs_single_view_params* prm, void* d_pose_out, void* d_verdict, void* d_final,
                                                void* d_n_final, void* d_stats, void* stream_to_wait)
{
    return akz_guard([&]() -> int32_t {
        akz_sv_settings st;
        AKZ_TRY(sv_settings(prm, &st));
        if (!c || !d_kps || !d_poses || !cam || !d_obs_start || (n_obs != 0 && !d_obs) || !d_world || !ik || !d_matches || !d_nmatches ||
            !d_pose || !d_best_id || !d_inliers || !d_n_inliers || !d_pose_out || !d_verdict || !d_final || !d_n_final || !d_stats)
            return AKZ_E_INVALID;
        if (cap_per_img == 0 || n_blocks == 0 || cam->reserved != 0 || n_scenes > 65535u || n_landmarks == 0xFFFFFFFFu) return AKZ_E_INVALID;
        const uint64_t n_rows = (uint64_t)n_world + (d_best ? (uint64_t)n_scenes * cap_per_img : 0u);
        if (n_rows > 0xFFFFFFFFull) return AKZ_E_TOO_LARGE;
        if (n_scenes == 0) return AKZ_OK;
        const RsHandles h = rs_internal_handles(c);
        if (h.max_scenes == 0) return AKZ_E_INVALID;              // a context without its batch arena (rs_batch_reserve failed)
        if (n_scenes > h.max_scenes) return AKZ_E_TOO_LARGE;
        AKZ_TRY(akz_enqueue_behind(h, stream_to_wait));
        RsSingleViewState* sv = rs_internal_single_view(c);
        AKZ_TRY(akz_grow_scratch(h.stream, &sv->d_scratch, &sv->bytes, sizeof(uint32_t) * (size_t)n_scenes * cap_per_img));
        // the frame list goes where the consensus keeps its own: stream order puts the copy behind that call's last reader
        AKZ_HIP(hipMemcpyAsync(h.d_frames, ik, sizeof(uint32_t) * n_scenes, hipMemcpyHostToDevice, h.stream));
        SvCall a;
        a.kps = (const akz_keypoint*)d_kps; a.poses = (const double*)d_poses; a.obs_start = (const uint32_t*)d_obs_start;
        a.obs = (const uint32_t*)d_obs; a.world = (const double*)d_world; a.frames = (const uint32_t*)h.d_frames;
        a.matches = (const uint32_t*)d_matches; a.nmatches = (const uint32_t*)d_nmatches; a.best = (const uint32_t*)d_best;
        a.pose = (const double*)d_pose; a.best_id = (const uint32_t*)d_best_id; a.inliers = (const uint32_t*)d_inliers;
        a.n_inliers = (const uint32_t*)d_n_inliers; a.pose_out = (double*)d_pose_out; a.verdict = (uint32_t*)d_verdict;
        a.final_mask = (unsigned char*)d_final; a.n_final = (uint32_t*)d_n_final; a.stats = (uint32_t*)d_stats;
        a.place = (uint32_t*)sv->d_scratch;
        a.cap = cap_per_img; a.n_blocks = n_blocks; a.n_obs = n_obs; a.n_landmarks = n_landmarks; a.n_world = n_world;
        a.n_rows = (uint32_t)n_rows;
        AKZ_HIP(hipFuncSetAttribute((const void*)k_single_view, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(SvShared)));
        hipLaunchKernelGGL(k_single_view, dim3(n_scenes), dim3(kSvBlock), sizeof(SvShared), h.stream, a, *cam, st);
        AKZ_LAUNCH_CHECK();
        return AKZ_OK;
    });
}
