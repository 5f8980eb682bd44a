// rs_observation_filter.hip — cv-sfm's filter of a reconstruction's observations behind a relaxation of its pose graph
// (VSlam::filter_non_robust_observations, cv-sfm/src/lib.rs:2657-2757) and, with rs_pose_graph.hip in front of it,
// VSlam::optimize_reconstruction as a whole (lib.rs:2343-2355) on gfx950.  The kernels of one pass, in stream order:
//   k_of_prepare     one workgroup per reconstruction: every start it owns is looked at before a landmark is read through one;
//                    its verdict (refused, skipped, running), its view count, its rows of the landmark -> reconstruction map.
//   k_of_decide      one lane per landmark, as k_tri_landmarks: the design matrix and the eigenvectors stay in registers, the
//                    keep flags go to memory and observations are fetched again rather than held (a list may be longer than
//                    any register file).  A chain of FP64 latency per lane.  The counts of a reconstruction are integer sums:
//                    a wave adds its lanes' with akz_wave_sum and one lane adds the sum to the reconstruction's words (a
//                    wave that straddles two reconstructions adds lane by lane); integer sums do not depend on their order.
//   k_of_tile_sums   the exclusive scan of the keep flags over the observations of the call, first level: one workgroup per
//                    tile of kTblTile flags (kTblItems per thread, as the rows of a table's tile) adds its tile.
//   k_of_scan_sums   second level: ONE workgroup walks the tile sums kTblBlock at a time with a running carry, so there is no
//                    third level however many tiles there are; it also closes the reconstructions' verdicts.
//   k_of_scatter     third pass: a workgroup scans its tile again, adds the tile's offset and writes every observation to its
//                    row of the filtered table or of the split list, and the kept-count in front of it to d_pos.
//   k_of_starts      the filtered table's start array from d_pos.
// Nothing here waits on a value another workgroup has yet to write: the levels of the scan are separate launches and their
// order is the order of the launches on the stream; every loop is bounded by an argument of the call.  The compaction is
// bandwidth over small words (1 B read twice, 8 B read and written once, 4 B written once per observation); LDS holds a
// workgroup's four wave totals and nothing else.
//
// The arithmetic is include/akz_observation_filter_math.h, the text the CPU checker
// (tests/cpp/observation_filter_host.c) compiles too — parity: host build == HIP, bit for bit.
#include "rs_table.h"
#include "../../include/akz_observation_filter_math.h"

namespace {

constexpr uint32_t kOfNone = 0xFFFFFFFFu;

static_assert(RS_OF_KEPT == AKZ_OF_KEPT && RS_OF_SINGLE == AKZ_OF_SINGLE && RS_OF_PAIR_SPLIT == AKZ_OF_PAIR_SPLIT &&
              RS_OF_NO_POINT == AKZ_OF_NO_POINT && RS_OF_KICKED == AKZ_OF_KICKED && RS_OF_BAD_INDEX == AKZ_OF_BAD_INDEX &&
              RS_OF_SKIPPED == AKZ_OF_SKIPPED, "landmark states");
static_assert(RS_OF_OK == AKZ_OF_OK && RS_OF_FEW_LANDMARKS == AKZ_OF_FEW_LANDMARKS && RS_OF_BAD_RANGE == AKZ_OF_BAD_RANGE &&
              RS_OF_RECON_SKIPPED == AKZ_OF_RECON_SKIPPED, "verdicts");
static_assert(RS_OF_STATS == AKZ_OF_STATS && RS_OF_S_LANDMARKS == AKZ_OF_S_LANDMARKS && RS_OF_S_ROBUST_BEFORE == AKZ_OF_S_ROBUST_BEFORE &&
              RS_OF_S_ROBUST_AFTER == AKZ_OF_S_ROBUST_AFTER && RS_OF_S_OBS_SPLIT == AKZ_OF_S_OBS_SPLIT &&
              RS_OF_S_PAIR_SPLIT == AKZ_OF_S_PAIR_SPLIT && RS_OF_S_NO_POINT == AKZ_OF_S_NO_POINT && RS_OF_S_KICKED == AKZ_OF_S_KICKED,
              "stats words");
static_assert(RS_OF_NO_SOLVE == AKZ_OF_NO_SOLVE && RS_OF_ROBUST_BEFORE == AKZ_OF_ROBUST_BEFORE && RS_OF_ROBUST_AFTER == AKZ_OF_ROBUST_AFTER,
              "bytes of a landmark");

// a landmark's observations: obs[s0 .. s0 + n), {block, feature} -> keypoint -> calibrated bearing, and the block's pose
struct OfSrc {
    const uint32_t* obs;
    const akz_keypoint* kps;
    const double* poses;
    const rs_camera* cam;
    uint32_t s0, cap, n_blocks;
};
__device__ __forceinline__ int of_fetch(const OfSrc* s, unsigned i, double* pose, double* b)
{
    const size_t at = (size_t)s->s0 + i;
    const uint32_t blk = s->obs[2 * at], feat = s->obs[2 * at + 1];
    if (blk >= s->n_blocks || feat >= s->cap) return 0;
    const akz_keypoint* kp = s->kps + (size_t)blk * s->cap + feat;
    akz_tri_calibrate(&s->cam->fx, s->cam->use_k1, s->cam->k1, kp->x, kp->y, b);
    const double* p = s->poses + (size_t)12 * blk;
#pragma unroll
    for (int k = 0; k < 12; ++k) pose[k] = p[k];
    return 1;
}
AKZ_TRI_DEFINE_TRIANGULATE(of_triangulate, OfSrc, of_fetch)
AKZ_OF_DEFINE_FILTER(of_landmark, OfSrc, of_fetch, of_triangulate)

// everything a pass's kernels share, by value
struct OfCall {
    const akz_keypoint* kps;
    const double* poses;
    const uint32_t* obs_start;    // [n_landmarks + 1]
    const uint32_t* obs;          // [n_obs][2]
    const uint32_t* recon_start;  // [n_recons + 1]
    const uint32_t* view_start;   // [n_recons + 1]
    const uint32_t* skip;         // [n_recons] or null
    unsigned char* keep;          // [n_obs]
    unsigned char* lm_state;      // [n_landmarks]
    unsigned char* tri_reason;    // [n_landmarks]
    unsigned char* robust;        // [n_landmarks]
    uint32_t* obs_start_out;      // [n_landmarks + 1]
    uint2* obs_out;               // [n_obs]
    uint2* split_out;             // [n_obs]
    uint32_t* counts;             // [2]
    uint32_t* verdict;            // [n_recons]
    uint32_t* stats;              // [n_recons][AKZ_OF_STATS]
    uint32_t* lm_recon;           // [n_landmarks] scratch: the running reconstruction a landmark belongs to, kOfNone otherwise
    uint32_t* recon_views;        // [n_recons] scratch
    uint32_t* pos;                // [n_obs + 1] scratch: the kept observations in front of observation i
    uint32_t* tile;               // [n_tiles] scratch: a tile's sum, then its offset
    uint32_t cap, n_blocks, n_obs, n_landmarks, n_recons, n_tiles;
};

// the observations that are the table's: the first min(obs_start[n_landmarks], n_obs)
__device__ __forceinline__ uint32_t of_filled(const OfCall& a)
{
    const uint32_t e = a.obs_start[a.n_landmarks];
    return e < a.n_obs ? e : a.n_obs;
}

// One workgroup per reconstruction.  A reconstruction runs when (1) no start of d_recon_start in front of its own lies above
// it and its range ascends inside [0, n_landmarks], (2) its view range ascends inside [0, n_blocks], (3) no start of
// d_obs_start in front of its first landmark lies above that landmark's and the starts it owns ascend up to n_obs at the
// most.  Two reconstructions that pass share no landmark and no observation, so no two lanes of k_of_decide write one flag.
__global__ __launch_bounds__(kTblBlock) void k_of_prepare(OfCall a)
{
    __shared__ uint32_t s_bad;
    const uint32_t r = blockIdx.x;
    if (threadIdx.x == 0) s_bad = 0u;
    __syncthreads();
    const uint32_t rs = a.recon_start[r], re = a.recon_start[r + 1], vs = a.view_start[r], ve = a.view_start[r + 1];
    uint32_t bad = (rs > re || re > a.n_landmarks || vs > ve || ve > a.n_blocks) ? 1u : 0u;
    for (uint32_t k = threadIdx.x; k < r; k += kTblBlock) bad |= a.recon_start[k] > rs ? 1u : 0u;
    if (!bad) {                                   // rs <= re <= n_landmarks: every index below is inside d_obs_start
        const uint32_t first = a.obs_start[rs];
        for (uint32_t l = threadIdx.x; l < rs; l += kTblBlock) bad |= a.obs_start[l] > first ? 1u : 0u;
        for (uint32_t l = rs + threadIdx.x; l < re; l += kTblBlock) bad |= a.obs_start[l] > a.obs_start[l + 1] ? 1u : 0u;
        bad |= a.obs_start[re] > a.n_obs ? 1u : 0u;
    }
    if (bad) atomicOr(&s_bad, 1u);
    __syncthreads();
    const bool refused = s_bad != 0u, skipped = !refused && a.skip && a.skip[r] != 0u;
    if (!refused && !skipped)
        for (uint32_t l = rs + threadIdx.x; l < re; l += kTblBlock) a.lm_recon[l] = r;
    if (threadIdx.x == 0) {
        uint32_t* stats = a.stats + (size_t)AKZ_OF_STATS * r;
#pragma unroll
        for (int k = 0; k < AKZ_OF_STATS; ++k) stats[k] = 0u;
        if (!refused) stats[AKZ_OF_S_LANDMARKS] = re - rs;
        a.recon_views[r] = refused ? 0u : ve - vs;
        a.verdict[r] = refused ? AKZ_OF_BAD_RANGE : skipped ? AKZ_OF_RECON_SKIPPED : AKZ_OF_OK;   // OK: until k_of_scan_sums has counted
    }
}

// One lane per landmark.  d_keep was set to 1 throughout in front of this kernel.
__global__ __launch_bounds__(kTblBlock) void k_of_decide(OfCall a, rs_camera cam, akz_of_settings st)
{
    const uint32_t l = blockIdx.x * kTblBlock + threadIdx.x, lane = threadIdx.x & 63u;
    const bool valid = l < a.n_landmarks;
    const uint32_t r = valid ? a.lm_recon[l] : kOfNone;
    int state = AKZ_OF_SKIPPED;
    akz_of_result res;
    res.tri_reason = AKZ_OF_NO_SOLVE; res.robust = 0u; res.n_split = 0u;
    if (r != kOfNone) {
        // k_of_prepare saw every start of a running reconstruction: s <= e <= n_obs
        const uint32_t s = a.obs_start[l], e = a.obs_start[l + 1];
        OfSrc src;
        src.obs = a.obs; src.kps = a.kps; src.poses = a.poses; src.cam = &cam;
        src.s0 = s; src.cap = a.cap; src.n_blocks = a.n_blocks;
        st.tri.n_views = a.recon_views[r];
        state = of_landmark(&src, e - s, &st, a.keep + s, &res);
    }
    if (valid) {
        a.lm_state[l] = (unsigned char)state;
        a.tri_reason[l] = (unsigned char)res.tri_reason;
        a.robust[l] = (unsigned char)res.robust;
    }
    uint32_t c[6] = {(res.robust & AKZ_OF_ROBUST_BEFORE) ? 1u : 0u, (res.robust & AKZ_OF_ROBUST_AFTER) ? 1u : 0u, res.n_split,
                     state == AKZ_OF_PAIR_SPLIT ? 1u : 0u, state == AKZ_OF_NO_POINT ? 1u : 0u, state == AKZ_OF_KICKED ? 1u : 0u};
    // lane 0 of a wave holds the wave's lowest landmark: where it is past the table, the whole wave is
    const uint32_t r0 = __shfl(r, 0, 64);
    if (__all(!valid || r == r0)) {
#pragma unroll
        for (int k = 0; k < 6; ++k) c[k] = akz_wave_sum(c[k]);
        if (lane == 0 && r0 != kOfNone) {
#pragma unroll
            for (int k = 0; k < 6; ++k)
                if (c[k]) atomicAdd(&a.stats[(size_t)AKZ_OF_STATS * r0 + AKZ_OF_S_ROBUST_BEFORE + k], c[k]);
        }
    } else if (r != kOfNone) {
#pragma unroll
        for (int k = 0; k < 6; ++k)
            if (c[k]) atomicAdd(&a.stats[(size_t)AKZ_OF_STATS * r + AKZ_OF_S_ROBUST_BEFORE + k], c[k]);
    }
}
static_assert(AKZ_OF_S_ROBUST_BEFORE == 1 && AKZ_OF_S_ROBUST_AFTER == 2 && AKZ_OF_S_OBS_SPLIT == 3 && AKZ_OF_S_PAIR_SPLIT == 4 &&
              AKZ_OF_S_NO_POINT == 5 && AKZ_OF_S_KICKED == 6, "the order of k_of_decide's six counts");

// the kTblItems flags of a thread of tile `tile`, as 0 / 1 (one 32-bit load where the array allows it); flags past the table's
// observations count as 0
__device__ __forceinline__ uint32_t of_thread_flags(const OfCall& a, uint32_t tile, uint32_t filled, uint32_t* k)
{
    static_assert(kTblItems == 4, "four flags are one word");
    const size_t i0 = (size_t)tile * kTblTile + (size_t)threadIdx.x * kTblItems;
    uint32_t word = 0u;
    if (((uintptr_t)a.keep & 3u) == 0u && i0 + kTblItems <= (size_t)a.n_obs)
        word = *reinterpret_cast<const uint32_t*>(a.keep + i0);
    else {
#pragma unroll
        for (int j = 0; j < kTblItems; ++j)
            if (i0 + j < (size_t)a.n_obs) word |= (uint32_t)a.keep[i0 + j] << (8 * j);
    }
    uint32_t sum = 0u;
#pragma unroll
    for (int j = 0; j < kTblItems; ++j) {
        k[j] = (i0 + j < filled && ((word >> (8 * j)) & 0xFFu) != 0u) ? 1u : 0u;
        sum += k[j];
    }
    return sum;
}

__global__ __launch_bounds__(kTblBlock) void k_of_tile_sums(OfCall a)
{
    __shared__ uint32_t s_wave[kTblWaves];
    uint32_t k[kTblItems];
    uint32_t sum = akz_wave_sum(of_thread_flags(a, blockIdx.x, of_filled(a), k));
    if ((threadIdx.x & 63u) == 0u) s_wave[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        sum = 0u;
#pragma unroll
        for (int w = 0; w < kTblWaves; ++w) sum += s_wave[w];
        a.tile[blockIdx.x] = sum;
    }
}

// ONE workgroup: tile sums -> tile offsets; the totals; the verdicts.
__global__ __launch_bounds__(kTblBlock) void k_of_scan_sums(OfCall a, uint32_t minimum_robust_landmarks)
{
    __shared__ uint32_t s_wave[kTblWaves];
    const uint32_t carry = tbl_scan_in_place(a.tile, a.n_tiles, s_wave);
    if (threadIdx.x == 0) {
        const uint32_t filled = of_filled(a);
        a.pos[filled] = carry;
        a.counts[0] = carry;
        a.counts[1] = filled - carry;
    }
    for (uint32_t r = threadIdx.x; r < a.n_recons; r += kTblBlock)
        if (a.verdict[r] == (uint32_t)AKZ_OF_OK)
            a.verdict[r] = (uint32_t)akz_of_verdict(a.stats[(size_t)AKZ_OF_STATS * r + AKZ_OF_S_ROBUST_AFTER], minimum_robust_landmarks);
}

__global__ __launch_bounds__(kTblBlock) void k_of_scatter(OfCall a)
{
    __shared__ uint32_t s_wave[kTblWaves];
    const uint32_t filled = of_filled(a);
    uint32_t k[kTblItems], total;
    const uint32_t sum = of_thread_flags(a, blockIdx.x, filled, k);
    uint32_t kept = a.tile[blockIdx.x] + akz_block_exclusive<kTblWaves>(sum, s_wave, &total);
    const size_t i0 = (size_t)blockIdx.x * kTblTile + (size_t)threadIdx.x * kTblItems;
    const uint2* obs = reinterpret_cast<const uint2*>(a.obs);
#pragma unroll
    for (int j = 0; j < kTblItems; ++j) {
        const size_t i = i0 + j;
        if (i >= filled) break;
        a.pos[i] = kept;
        // kept <= i < n_obs and i - kept < n_obs: both rows are inside the callers' arrays
        if (k[j]) a.obs_out[kept] = obs[i];
        else a.split_out[i - kept] = obs[i];
        kept += k[j];
    }
}

__global__ __launch_bounds__(kTblBlock) void k_of_starts(OfCall a)
{
    const uint32_t l = blockIdx.x * kTblBlock + threadIdx.x;
    if (l > a.n_landmarks) return;
    const uint32_t filled = of_filled(a), s = a.obs_start[l];
    a.obs_start_out[l] = a.pos[s < filled ? s : filled];
}

// the chain: a reconstruction that a stage did not pass stops; verdict = where
__global__ void k_or_note(const uint32_t* __restrict__ stage_verdict, uint32_t ok, uint32_t round, uint32_t stage, uint32_t n,
                          uint32_t* __restrict__ stop, uint32_t* __restrict__ verdict)
{
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n || stop[r] != 0u) return;
    const uint32_t v = stage_verdict[r];
    if (v == ok) return;
    stop[r] = 1u;
    verdict[r] = (uint32_t)RS_OR_STOPPED | round << 16 | stage << 8 | (v & 0xFFu);
}

int32_t of_settings(const rs_observation_filter_params* prm, akz_of_settings* st)
{
    if (!prm || prm->struct_size != sizeof(rs_observation_filter_params) || prm->reserved != 0) return AKZ_E_INVALID;
    if (prm->maximum_cosine_distance != prm->maximum_cosine_distance || prm->maximum_sine_distance != prm->maximum_sine_distance)
        return AKZ_E_INVALID;
    AKZ_TRY(akz_tri_settings_from(prm->triangulate, &st->tri));
    if (!AKZ_TRI_FINITE(prm->triangulate.incidence_minimum_cosine_distance)) return AKZ_E_INVALID;
    if (prm->reconstruction_optimization_iterations > (uint32_t)RS_OF_MAX_ITERATIONS) return AKZ_E_TOO_LARGE;
    st->maximum_cosine_distance = prm->maximum_cosine_distance;
    st->maximum_sine_distance = prm->maximum_sine_distance;
    st->minimum_robust_landmarks = prm->minimum_robust_landmarks;
    st->tri.n_views = 0u;                                          // every reconstruction's own, in k_of_decide
    return AKZ_OK;
}

// the tables of one pass and where it writes
struct OfArgs {
    const void *d_kps, *d_poses, *d_obs_start, *d_obs, *d_recon_start, *d_view_start, *d_skip;
    void *d_keep, *d_lm_state, *d_tri_reason, *d_robust, *d_obs_start_out, *d_obs_out, *d_split_out, *d_counts, *d_recon_verdict, *d_stats;
    uint32_t cap, n_blocks, n_obs, n_landmarks, n_recons;
};

int32_t of_check(rs_ctx* c, const OfArgs& g, const rs_camera* cam)
{
    if (!c || !g.d_kps || !g.d_poses || !cam || !g.d_obs_start || (g.n_obs != 0 && !g.d_obs) || !g.d_recon_start || !g.d_view_start) return AKZ_E_INVALID;
    if (!g.d_keep || !g.d_lm_state || !g.d_tri_reason || !g.d_robust || !g.d_obs_start_out || !g.d_obs_out || !g.d_split_out || !g.d_counts ||
        !g.d_recon_verdict || !g.d_stats)
        return AKZ_E_INVALID;
    if (g.cap == 0 || g.n_blocks == 0 || cam->reserved != 0 || g.n_landmarks == 0xFFFFFFFFu || g.n_obs == 0xFFFFFFFFu) return AKZ_E_INVALID;
    // the input table is const: no output table may lie over it
    const size_t start_bytes = sizeof(uint32_t) * ((size_t)g.n_landmarks + 1), obs_bytes = sizeof(uint32_t) * 2 * (size_t)g.n_obs;
    const void* in[2] = {g.d_obs_start, g.d_obs};
    const size_t in_bytes[2] = {start_bytes, obs_bytes};
    const void* out[4] = {g.d_obs_start_out, g.d_obs_out, g.d_split_out, g.d_keep};
    const size_t out_bytes[4] = {start_bytes, obs_bytes, obs_bytes, g.n_obs};
    return akz_outputs_clear_of_inputs(in, in_bytes, 2, out, out_bytes, 4) ? AKZ_OK : AKZ_E_INVALID;
}

// one pass on the stream (the device is current, the stream ordered behind the caller's)
int32_t of_enqueue(rs_ctx* c, const RsHandles& h, const OfArgs& g, const rs_camera* cam, const akz_of_settings& st)
{
    RsObsFilterState* fs = rs_internal_obs_filter(c);
    const uint32_t n_tiles = (uint32_t)(((size_t)g.n_obs + kTblTile - 1) / kTblTile);
    const size_t w = sizeof(uint32_t);
    AkzScratchPlan plan;
    const size_t at_lm = plan.take(w * ((size_t)g.n_landmarks + 1)), at_views = plan.take(w * ((size_t)g.n_recons + 1));
    const size_t at_pos = plan.take(w * ((size_t)g.n_obs + 1)), at_tile = plan.take(w * ((size_t)n_tiles + 1));
    AKZ_TRY(akz_grow_scratch(h.stream, &fs->d_scratch, &fs->bytes, plan.size()));
    char* base = (char*)fs->d_scratch;
    OfCall a;
    a.kps = (const akz_keypoint*)g.d_kps; a.poses = (const double*)g.d_poses;
    a.obs_start = (const uint32_t*)g.d_obs_start; a.obs = (const uint32_t*)g.d_obs;
    a.recon_start = (const uint32_t*)g.d_recon_start; a.view_start = (const uint32_t*)g.d_view_start; a.skip = (const uint32_t*)g.d_skip;
    a.keep = (unsigned char*)g.d_keep; a.lm_state = (unsigned char*)g.d_lm_state; a.tri_reason = (unsigned char*)g.d_tri_reason;
    a.robust = (unsigned char*)g.d_robust; a.obs_start_out = (uint32_t*)g.d_obs_start_out; a.obs_out = (uint2*)g.d_obs_out;
    a.split_out = (uint2*)g.d_split_out; a.counts = (uint32_t*)g.d_counts; a.verdict = (uint32_t*)g.d_recon_verdict;
    a.stats = (uint32_t*)g.d_stats;
    a.lm_recon = (uint32_t*)(base + at_lm); a.recon_views = (uint32_t*)(base + at_views); a.pos = (uint32_t*)(base + at_pos);
    a.tile = (uint32_t*)(base + at_tile);
    a.cap = g.cap; a.n_blocks = g.n_blocks; a.n_obs = g.n_obs; a.n_landmarks = g.n_landmarks; a.n_recons = g.n_recons; a.n_tiles = n_tiles;
    if (g.n_landmarks) AKZ_HIP(hipMemsetAsync(a.lm_recon, 0xFF, sizeof(uint32_t) * (size_t)g.n_landmarks, h.stream));
    if (g.n_obs) AKZ_HIP(hipMemsetAsync(a.keep, 1, g.n_obs, h.stream));
    if (g.n_recons) {
        hipLaunchKernelGGL(k_of_prepare, dim3(g.n_recons), dim3(kTblBlock), 0, h.stream, a);
        AKZ_LAUNCH_CHECK();
    }
    if (g.n_landmarks) {
        hipLaunchKernelGGL(k_of_decide, dim3((g.n_landmarks + kTblBlock - 1) / kTblBlock), dim3(kTblBlock), 0, h.stream, a, *cam, st);
        AKZ_LAUNCH_CHECK();
    }
    if (n_tiles) {
        hipLaunchKernelGGL(k_of_tile_sums, dim3(n_tiles), dim3(kTblBlock), 0, h.stream, a);
        AKZ_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_of_scan_sums, dim3(1), dim3(kTblBlock), 0, h.stream, a, st.minimum_robust_landmarks);
    AKZ_LAUNCH_CHECK();
    if (n_tiles) {
        hipLaunchKernelGGL(k_of_scatter, dim3(n_tiles), dim3(kTblBlock), 0, h.stream, a);
        AKZ_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_of_starts, dim3(g.n_landmarks / kTblBlock + 1), dim3(kTblBlock), 0, h.stream, a);
    AKZ_LAUNCH_CHECK();
    return AKZ_OK;
}

}   // namespace

extern "C" int32_t rs_observation_filter_params_default(rs_observation_filter_params* prm)
{
    if (!prm) return AKZ_E_INVALID;
    prm->struct_size = sizeof(rs_observation_filter_params);
    prm->minimum_robust_landmarks = 32;                           // cv-sfm/src/settings.rs:340-342
    prm->maximum_cosine_distance = 1e-5;                          // settings.rs:324-326
    prm->maximum_sine_distance = 1e-1;                            // settings.rs:328-330
    prm->reconstruction_optimization_iterations = 1;              // settings.rs:429-431
    prm->reserved = 0;
    return rs_triangulate_params_default(&prm->triangulate);      // settings.rs:344-350 and the triangulator's own
}

extern "C" int32_t rs_filter_observations_device(rs_ctx* c, const void* d_kps, uint32_t cap_per_img, uint32_t n_blocks, const void* d_poses,
                                                 const rs_camera* cam, const void* d_obs_start, const void* d_obs, uint32_t n_obs,
                                                 uint32_t n_landmarks, const void* d_recon_start, const void* d_view_start, uint32_t n_recons,
                                                 const void* d_skip, const rs_observation_filter_params* prm, void* d_keep, void* d_lm_state,
                                                 void* d_tri_reason, void* d_robust, void* d_obs_start_out, void* d_obs_out, void* d_split_out,
                                                 void* d_counts, void* d_recon_verdict, void* d_stats, void* stream_to_wait)
{
    return akz_guard([&]() -> int32_t {
        akz_of_settings st;
        AKZ_TRY(of_settings(prm, &st));
        const OfArgs g = {d_kps, d_poses, d_obs_start, d_obs, d_recon_start, d_view_start, d_skip, d_keep, d_lm_state, d_tri_reason, d_robust,
                          d_obs_start_out, d_obs_out, d_split_out, d_counts, d_recon_verdict, d_stats, cap_per_img, n_blocks, n_obs, n_landmarks,
                          n_recons};
        AKZ_TRY(of_check(c, g, cam));
        const RsHandles h = rs_internal_handles(c);
        AKZ_TRY(akz_enqueue_behind(h, stream_to_wait));
        return of_enqueue(c, h, g, cam, st);
    });
}

extern "C" int32_t rs_optimize_reconstruction_batch_device(
    rs_ctx* c, void* d_poses, uint32_t n_views, const void* d_graph_start, uint32_t n_graphs, const void* d_row_start, const void* d_row_edges,
    uint32_t n_rows, const void* d_views, const void* d_constraint_verdict, const void* d_edges, uint32_t n_constraints,
    const rs_pose_graph_params* pg_prm, const void* d_kps, uint32_t cap_per_img, const rs_camera* cam, const void* d_obs_start, const void* d_obs,
    uint32_t n_obs, uint32_t n_landmarks, const void* d_recon_start, const rs_observation_filter_params* prm, void* d_verdict,
    void* d_graph_verdict, void* d_view_state, void* d_pg_stats, void* d_keep, void* d_lm_state, void* d_tri_reason, void* d_robust,
    void* d_obs_start_out, void* d_obs_out, void* d_split_out, void* d_counts, void* d_recon_verdict, void* d_of_stats, void* d_world,
    void* d_world_reason, void* stream_to_wait)
{
    return akz_guard([&]() -> int32_t {
        akz_of_settings st;
        AKZ_TRY(of_settings(prm, &st));
        if (!pg_prm || pg_prm->struct_size != sizeof(rs_pose_graph_params) || !AKZ_TRI_FINITE(pg_prm->graph_optimization_rate)) return AKZ_E_INVALID;
        if (!d_verdict || !d_graph_start || !d_row_start || (n_rows != 0 && !d_row_edges) || !d_graph_verdict || !d_view_state || !d_pg_stats)
            return AKZ_E_INVALID;
        if (n_constraints != 0 && (!d_views || !d_constraint_verdict || !d_edges)) return AKZ_E_INVALID;
        OfArgs g = {d_kps, d_poses, d_obs_start, d_obs, d_recon_start, d_graph_start, nullptr, d_keep, d_lm_state, d_tri_reason, d_robust,
                    d_obs_start_out, d_obs_out, d_split_out, d_counts, d_recon_verdict, d_of_stats, cap_per_img, n_views, n_obs, n_landmarks,
                    n_graphs};
        AKZ_TRY(of_check(c, g, cam));
        const uint32_t rounds = prm->reconstruction_optimization_iterations;
        const RsHandles h = rs_internal_handles(c);
        RsObsFilterState* fs = rs_internal_obs_filter(c);
        AKZ_TRY(akz_enqueue_behind(h, stream_to_wait));
        // the chain's scratch: a word per reconstruction, and the tables between the rounds (none for one round, one for two)
        const size_t stop_bytes = akz_align_up(sizeof(uint32_t) * ((size_t)n_graphs + 1), 256);
        const size_t start_bytes = akz_align_up(sizeof(uint32_t) * ((size_t)n_landmarks + 1), 256);
        const size_t obs_bytes = akz_align_up(sizeof(uint32_t) * 2 * ((size_t)n_obs + 1), 256);
        const size_t n_tables = rounds <= 1 ? 0 : rounds == 2 ? 1 : 2;
        AKZ_TRY(akz_grow_scratch(h.stream, &fs->d_chain, &fs->chain_bytes, stop_bytes + n_tables * (start_bytes + obs_bytes)));
        char* base = (char*)fs->d_chain;
        uint32_t* d_stop = (uint32_t*)base;
        void* tab_start[2] = {base + stop_bytes, base + stop_bytes + start_bytes + obs_bytes};
        void* tab_obs[2] = {base + stop_bytes + start_bytes, base + stop_bytes + 2 * start_bytes + obs_bytes};
        AKZ_HIP(hipMemsetAsync(d_stop, 0, sizeof(uint32_t) * ((size_t)n_graphs + 1), h.stream));
        if (n_graphs) AKZ_HIP(hipMemsetAsync(d_verdict, 0, sizeof(uint32_t) * (size_t)n_graphs, h.stream));
        const uint32_t note_grid = (n_graphs + 255u) / 256u;
        g.d_skip = d_stop;
        for (uint32_t round = 0; round < rounds; ++round) {
            AKZ_TRY(rs_internal_pose_graph_relax(c, d_poses, n_views, d_graph_start, n_graphs, d_row_start, d_row_edges, n_rows, d_views,
                                                 d_constraint_verdict, d_edges, n_constraints, pg_prm, d_graph_verdict, d_view_state, d_pg_stats,
                                                 d_stop, nullptr));
            if (n_graphs) {
                hipLaunchKernelGGL(k_or_note, dim3(note_grid), dim3(256), 0, h.stream, (const uint32_t*)d_graph_verdict, (uint32_t)RS_PG_OK, round,
                                   (uint32_t)RS_OR_STAGE_RELAX, n_graphs, d_stop, (uint32_t*)d_verdict);
                AKZ_LAUNCH_CHECK();
            }
            const bool last = round + 1 == rounds;
            g.d_obs_start_out = last ? d_obs_start_out : tab_start[round & 1u];
            g.d_obs_out = last ? d_obs_out : tab_obs[round & 1u];
            g.d_split_out = (char*)d_split_out + sizeof(uint32_t) * 2 * (size_t)n_obs * round;
            g.d_counts = (uint32_t*)d_counts + 2 * (size_t)round;
            g.d_recon_verdict = (uint32_t*)d_recon_verdict + (size_t)n_graphs * round;
            g.d_stats = (uint32_t*)d_of_stats + (size_t)RS_OF_STATS * n_graphs * round;
            AKZ_TRY(of_enqueue(c, h, g, cam, st));
            if (n_graphs) {
                hipLaunchKernelGGL(k_or_note, dim3(note_grid), dim3(256), 0, h.stream, (const uint32_t*)g.d_recon_verdict, (uint32_t)RS_OF_OK, round,
                                   (uint32_t)RS_OR_STAGE_FILTER, n_graphs, d_stop, (uint32_t*)d_verdict);
                AKZ_LAUNCH_CHECK();
            }
            g.d_obs_start = g.d_obs_start_out;
            g.d_obs = g.d_obs_out;
        }
        if (rounds == 0) {
            AKZ_HIP(hipMemcpyAsync(d_obs_start_out, d_obs_start, sizeof(uint32_t) * ((size_t)n_landmarks + 1), hipMemcpyDeviceToDevice, h.stream));
            if (n_obs) AKZ_HIP(hipMemcpyAsync(d_obs_out, d_obs, sizeof(uint32_t) * 2 * (size_t)n_obs, hipMemcpyDeviceToDevice, h.stream));
        }
        if (d_world)
            AKZ_TRY(rs_triangulate_landmarks_device(c, d_kps, cap_per_img, n_views, d_poses, cam, d_obs_start_out, d_obs_out, n_obs, n_landmarks,
                                                    &prm->triangulate, d_world, d_world_reason, nullptr));
        return AKZ_OK;
    });
}
