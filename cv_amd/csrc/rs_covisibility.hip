// rs_covisibility.hip — the covisibility search in front of cv-sfm's three-view constraints (VSlam::generate_view_constraints,
// cv-sfm/src/lib.rs:2438-2516, with view_covisibilities, lib.rs:2535-2556), the verdict of record_view_constraints
// (lib.rs:2092-2109) and the rows of flatten_constraints (lib.rs:2519-2532) on gfx950.  Integers only.  The kernels of a
// candidates call, in stream order:
//   k_cv_scatter   one lane per landmark: the inverse map {block, feature} -> landmark (the lowest landmark wins a cell that two
//                  name), a byte per landmark that names a block or feature outside the arrays, a word for a broken start array.
//   k_cv_targets   one workgroup per target (a bounded grid that walks the targets): the target's robust features compacted in
//                  feature order, a count per coview, the candidate views (at most RS_CV_MAX_CANDIDATE_VIEWS, by a histogram
//                  over the counts), ONE BIT ROW PER CANDIDATE over the target's robust features, a pair's count as the
//                  popcount of the AND of two rows — the hot loop, up to 8 128 pairs —, the stable sort of the pairs by count
//                  (bitonic_sort_lds_u64 on keys that carry the pair index), and lane 0 alone for the unique walk and the chain
//                  (akz_cv_walk: serial by nature, short).  Writes the slots' views and counts and their offsets inside the
//                  target.
//   k_cv_scan      ONE workgroup: the exclusive scan of the targets' entries, kCvBlock at a time behind a running carry.
//   k_cv_lists     one workgroup per slot: the covisible landmarks of the slot's triple in the target's feature order (an ordered
//                  compaction), sorted by observation count in LDS, cut, written with their three features.
// The rows live in scratch of the context, not in LDS: 128 rows of 8 192 bits are 128 KB, which beside the 64 KB of sort keys
// is more than the 160 KB of a compute unit; in scratch a workgroup's rows (at most 128 KB, typically a tenth of that) stay in L2
// between the pass that sets the bits and the pass that counts the pairs, and LDS is left to the keys alone, two workgroups
// to a compute unit.  No workgroup waits on another: the levels of the scan are separate launches.  Every loop is bounded by an
// argument of the call or an RS_CV_* constant.
//   k_cv_record    one lane per target: akz_cv_record on the constraint stage's verdicts of its slots.
//   k_pgr_*        rs_pose_graph_rows_device: count (an atomic add per row entry), scan (one workgroup), and the ordered fill as a
//                  sort of the keys view << 32 | edge id over the whole call — n log^2 n whatever the rows' lengths (the unused
//                  slots of a candidates call all sit in view 0's row).
//
// The decisions are include/akz_covisibility_math.h, the text the CPU checker (tests/cpp/covisibility_host.c) compiles too —
// parity: host build == HIP in every output word.
#include "rs_table.h"
#include "../../include/akz_covisibility_math.h"

namespace {

constexpr int kCvBlock = 256;
constexpr int kCvWaves = kCvBlock / 64;
constexpr uint32_t kCvGroups = 1024;                                    // workgroups of k_cv_targets at the most (each owns scratch)
constexpr size_t kCvKeyBytes = sizeof(uint64_t) * 8192;                 // the pair keys: AKZ_CV_MAX_PAIRS rounded up to a power of two

static_assert(RS_CV_MAX_CANDIDATE_VIEWS == AKZ_CV_MAX_CANDIDATE_VIEWS && RS_CV_MAX_SLOTS == AKZ_CV_MAX_SLOTS &&
              RS_CV_MAX_FEATURES == AKZ_CV_MAX_FEATURES && RS_TVC_MAX_LANDMARKS == AKZ_CV_MAX_LANDMARKS, "capacities");
static_assert(AKZ_CV_MAX_PAIRS == AKZ_CV_MAX_CANDIDATE_VIEWS * (AKZ_CV_MAX_CANDIDATE_VIEWS - 1) / 2 && AKZ_CV_MAX_PAIRS <= 8192, "pairs");
static_assert(RS_CV_OK == AKZ_CV_OK && RS_CV_FEW_CONSTRAINTS == AKZ_CV_FEW_CONSTRAINTS && RS_CV_BAD_INDEX == AKZ_CV_BAD_INDEX &&
              RS_CV_NO_GRAPH == AKZ_CV_NO_GRAPH && RS_CV_NOT_RECORDED == AKZ_CV_NOT_RECORDED, "verdicts");
static_assert(RS_CV_S_ROBUST == AKZ_CV_S_ROBUST && RS_CV_S_CANDIDATES == AKZ_CV_S_CANDIDATES && RS_CV_S_PAIRS == AKZ_CV_S_PAIRS &&
              RS_CV_S_UNIQUE == AKZ_CV_S_UNIQUE && RS_CV_S_EMITTED == AKZ_CV_S_EMITTED && RS_CV_S_FLAGS == AKZ_CV_S_FLAGS &&
              RS_CV_S_RECORDED == AKZ_CV_S_RECORDED && RS_CV_STATS == AKZ_CV_STATS && RS_CV_F_CANDIDATES_CAPPED == AKZ_CV_F_CANDIDATES_CAPPED &&
              RS_CV_F_LIMIT_REACHED == AKZ_CV_F_LIMIT_REACHED, "stats words");
static_assert(RS_TRI_OK == AKZ_CV_TRI_OK && RS_TVC_OK == 0 && RS_CV_NOT_RECORDED > RS_TVC_BAD_INDEX, "the words of the stages around");

// everything a candidates call's kernels share, by value
struct CvCall {
    const uint32_t* obs_start;     // [n_landmarks + 1]
    const uint32_t* obs;           // [n_obs][2]
    const unsigned char* reason;   // [n_landmarks]
    const uint32_t* targets;       // [n_targets]
    uint32_t* views;               // [n_slots][3]
    uint32_t* lm_start;            // [n_slots + 1]
    uint32_t* lm;                  // [n_slots * maximum_landmarks][3]
    uint32_t* slot_count;          // [n_slots]
    uint32_t* verdict;             // [n_targets]
    uint32_t* stats;               // [n_targets][AKZ_CV_STATS]
    uint32_t* inv;                 // scratch [n_blocks][cap]: the landmark of a feature, AKZ_CV_NONE
    unsigned char* lm_bad;         // scratch [n_landmarks]
    uint32_t* flags;               // scratch [1]: a start pair that does not ascend within [0, n_obs]
    uint32_t* local;               // scratch [n_slots]: a slot's offset inside its target
    uint32_t* tot;                 // scratch [n_targets]: a target's entries, then its offset
    uint32_t* g_cnt;               // scratch [groups][n_blocks]: a coview's count, then its candidate index
    uint32_t* g_feat;              // scratch [groups][cap]: the landmarks of the target's robust features
    unsigned long long* g_rows;    // scratch [groups][AKZ_CV_MAX_CANDIDATE_VIEWS][wmax]
    uint32_t n_obs, n_landmarks, cap, n_blocks, n_targets, wmax;
    akz_cv_settings st;
};

__global__ __launch_bounds__(kCvBlock) void k_cv_scatter(CvCall a)
{
    const uint32_t l = blockIdx.x * kCvBlock + threadIdx.x;
    if (l >= a.n_landmarks) return;
    const uint32_t s = a.obs_start[l], e = a.obs_start[l + 1];
    if (s > e || e > a.n_obs) {
        atomicOr(a.flags, 1u);
        a.lm_bad[l] = 1;
        return;
    }
    unsigned char bad = 0;
    for (uint32_t i = s; i < e; ++i) {
        const uint32_t blk = a.obs[2 * (size_t)i], feat = a.obs[2 * (size_t)i + 1];
        if (blk >= a.n_blocks || feat >= a.cap) bad = 1;
        else atomicMin(&a.inv[(size_t)blk * a.cap + feat], l);
    }
    a.lm_bad[l] = bad;
}

extern __shared__ __attribute__((aligned(16))) unsigned char cv_lds[];

__global__ __launch_bounds__(kCvBlock) void k_cv_targets(CvCall a)
{
    __shared__ uint32_t s_cnt[2][kCvWaves];
    __shared__ uint32_t s_cand[AKZ_CV_MAX_CANDIDATE_VIEWS];
    __shared__ uint32_t s_unique[(AKZ_CV_MAX_PAIRS + 31) / 32 + 1];
    __shared__ unsigned char s_visited[AKZ_CV_MAX_CANDIDATE_VIEWS + 1];
    __shared__ uint32_t s_thr[3];
    __shared__ uint32_t s_span[2];                                    // the lowest and the highest coview that was counted
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(cv_lds);
    uint32_t* hist = reinterpret_cast<uint32_t*>(cv_lds);             // [nF + 1], before the keys are made
    uint32_t* cnt = a.g_cnt + (size_t)blockIdx.x * a.n_blocks;
    uint32_t* feat = a.g_feat + (size_t)blockIdx.x * a.cap;
    unsigned long long* rows = a.g_rows + (size_t)blockIdx.x * AKZ_CV_MAX_CANDIDATE_VIEWS * a.wmax;
    const uint32_t tid = threadIdx.x, limit = a.st.limit, minc = akz_cv_minimum(&a.st);
    uint32_t tick = 0;
    for (uint32_t t = blockIdx.x; t < a.n_targets; t += gridDim.x) {
        __syncthreads();                                              // the target before is done with LDS and scratch
        const uint32_t v = a.targets[t];
        const size_t slot0 = (size_t)t * limit;
        const bool refuse = v >= a.n_blocks || *a.flags != 0u;
        uint32_t nF = 0;
        int bad = 0;
        // cnt is zero throughout here (the call clears it, every target clears what it touched): a target's passes walk the
        // span of blocks it counted, not the blocks of the whole call
        if (tid == 0) {
            s_span[0] = 0xFFFFFFFFu;
            s_span[1] = 0u;
        }
        if (!refuse) {
            uint32_t lo = 0xFFFFFFFFu, hi = 0u;
            __syncthreads();
            // 1. the robust features in feature order, and every coview's count (lib.rs:2541-2553)
            for (uint32_t j0 = 0; j0 < a.cap; j0 += kCvBlock) {
                const uint32_t j = j0 + tid;
                const uint32_t l = j < a.cap ? a.inv[(size_t)v * a.cap + j] : AKZ_CV_NONE;
                bool flag = false;
                if (l != AKZ_CV_NONE) {
                    if (a.lm_bad[l]) bad = 1;
                    else flag = a.reason[l] == (unsigned char)AKZ_CV_TRI_OK;
                }
                uint32_t total;
                const uint32_t rank = akz_block_scan<kCvWaves>(s_cnt, tick, flag, &total);
                if (flag) {
                    feat[nF + rank] = l;
                    const uint32_t s = a.obs_start[l], e = a.obs_start[l + 1];
                    for (uint32_t i = s; i < e; ++i) {
                        const uint32_t blk = a.obs[2 * (size_t)i];
                        if (blk != v && akz_cv_first_of_block(a.obs, s, i)) {
                            atomicAdd(&cnt[blk], 1u);
                            lo = blk < lo ? blk : lo;
                            hi = blk > hi ? blk : hi;
                        }
                    }
                }
                nF += total;
            }
            if (lo <= hi) {
                atomicMin(&s_span[0], lo);
                atomicMax(&s_span[1], hi);
            }
            bad = __syncthreads_or(bad);
        }
        __syncthreads();
        const uint32_t b_lo = s_span[0] <= s_span[1] ? s_span[0] : 0u, b_n = s_span[0] <= s_span[1] ? s_span[1] - s_span[0] + 1u : 0u;
        uint32_t* stats = a.stats + (size_t)AKZ_CV_STATS * t;
        if (refuse || bad) {
            for (uint32_t k = tid; k < b_n; k += kCvBlock) cnt[b_lo + k] = 0u;
            for (uint32_t k = tid; k < limit; k += kCvBlock) {
                a.views[3 * (slot0 + k)] = a.views[3 * (slot0 + k) + 1] = a.views[3 * (slot0 + k) + 2] = 0u;
                a.slot_count[slot0 + k] = 0u;
                a.local[slot0 + k] = 0u;
            }
            if (tid == 0) {
#pragma unroll
                for (int k = 0; k < AKZ_CV_STATS; ++k) stats[k] = 0u;
                a.verdict[t] = (uint32_t)AKZ_CV_BAD_INDEX;
                a.tot[t] = 0u;
            }
            continue;
        }
        // 2. the candidate views (lib.rs:2446-2453), at most AKZ_CV_MAX_CANDIDATE_VIEWS of them, ascending by block
        for (uint32_t c = tid; c <= nF; c += kCvBlock) hist[c] = 0u;
        __syncthreads();
        for (uint32_t k = tid; k < b_n; k += kCvBlock) {
            const uint32_t c = cnt[b_lo + k];
            if (c >= minc) atomicAdd(&hist[c], 1u);
        }
        __syncthreads();
        if (tid == 0) s_thr[2] = (uint32_t)akz_cv_candidate_threshold(hist, nF, minc, &s_thr[0], &s_thr[1]);
        __syncthreads();
        const uint32_t thr = s_thr[0], quota = s_thr[1];
        const bool capped = s_thr[2] != 0u;
        uint32_t C = 0, eq_run = 0;
        for (uint32_t k0 = 0; k0 < b_n; k0 += kCvBlock) {
            const uint32_t b = b_lo + k0 + tid;
            const bool in = k0 + tid < b_n;                               // b < n_blocks: it was counted
            const uint32_t c = in ? cnt[b] : 0u;
            bool keep = in && c > thr && c >= minc;
            uint32_t total;
            if (capped) {
                const bool eq = in && c == thr;
                const uint32_t r = akz_block_scan<kCvWaves>(s_cnt, tick, eq, &total);
                keep = keep || (eq && eq_run + r < quota);
                eq_run += total;
            }
            const uint32_t ci = C + akz_block_scan<kCvWaves>(s_cnt, tick, keep, &total);
            keep = keep && ci < (uint32_t)AKZ_CV_MAX_CANDIDATE_VIEWS;
            if (in) cnt[b] = keep ? ci : AKZ_CV_NONE;
            if (keep) s_cand[ci] = b;
            C += total;
        }
        C = C < (uint32_t)AKZ_CV_MAX_CANDIDATE_VIEWS ? C : (uint32_t)AKZ_CV_MAX_CANDIDATE_VIEWS;
        // 3. a bit row per candidate over the target's robust features
        const uint32_t W = (nF + 63u) / 64u;
        for (uint32_t k = tid; k < C * W; k += kCvBlock) rows[(size_t)(k / W) * a.wmax + k % W] = 0ull;
        __syncthreads();
        for (uint32_t p = tid; p < nF; p += kCvBlock) {
            const uint32_t l = feat[p], s = a.obs_start[l], e = a.obs_start[l + 1];
            for (uint32_t i = s; i < e; ++i) {
                const uint32_t blk = a.obs[2 * (size_t)i];
                const uint32_t ci = blk != v ? cnt[blk] : AKZ_CV_NONE;
                if (ci != AKZ_CV_NONE) atomicOr(&rows[(size_t)ci * a.wmax + (p >> 6)], 1ull << (p & 63u));
            }
        }
        __syncthreads();
        for (uint32_t k = tid; k < b_n; k += kCvBlock) cnt[b_lo + k] = 0u;   // the counts (by now candidate indices) are done with
        // 4. the pairs' counts (lib.rs:2463-2481) and their stable sort by count, descending (lib.rs:2484-2486)
        const uint32_t P = C * (C - (C ? 1u : 0u)) / 2u;
        uint32_t np2 = 1;
        while (np2 < P) np2 <<= 1;
        uint32_t mine = 0;
        for (uint32_t q = tid; q < np2; q += kCvBlock) {
            unsigned long long key = ~0ull;
            if (q < P) {
                uint32_t ia, ib, count = 0;
                akz_cv_pair_from_index(q, C, &ia, &ib);
                const unsigned long long *ra = rows + (size_t)ia * a.wmax, *rb = rows + (size_t)ib * a.wmax;
                for (uint32_t w = 0; w < W; ++w) count += (uint32_t)__popcll(ra[w] & rb[w]);
                if (count >= minc) {
                    key = akz_cv_pair_key(count, q);
                    ++mine;
                }
            }
            keys[q] = key;
        }
        const uint32_t n_pairs = akz_block_sum<kCvWaves>(s_cnt, tick, mine);
        __syncthreads();
        if (np2 >= 2u) bitonic_sort_lds_u64<kCvBlock>(keys, np2);
        // 5, 6. the unique walk and the chain: one lane
        if (tid == 0) {
            stats[AKZ_CV_S_ROBUST] = nF;
            stats[AKZ_CV_S_CANDIDATES] = C;
            stats[AKZ_CV_S_FLAGS] = capped ? (uint32_t)AKZ_CV_F_CANDIDATES_CAPPED : 0u;
            stats[AKZ_CV_S_RECORDED] = 0u;
            stats[7] = 0u;
            a.tot[t] = akz_cv_walk((const uint64_t*)keys, n_pairs, s_cand, C, v, &a.st, s_visited, s_unique, a.views + 3 * slot0,
                                   a.slot_count + slot0, a.local + slot0, stats);
            a.verdict[t] = (uint32_t)AKZ_CV_OK;
        }
    }
}

// ONE workgroup: the targets' entries -> their offsets; the end of d_lm_start
__global__ __launch_bounds__(kCvBlock) void k_cv_scan(CvCall a)
{
    __shared__ uint32_t s_wave[kCvWaves];
    const uint32_t carry = tbl_scan_in_place<kCvWaves>(a.tot, a.n_targets, s_wave);
    if (threadIdx.x == 0) a.lm_start[(size_t)a.n_targets * a.st.limit] = carry;
}

// One workgroup per slot.  LDS: np2 keys and np2 16-bit features, np2 the power of two at or above cap_per_img.
__global__ __launch_bounds__(kCvBlock) void k_cv_lists(CvCall a, uint32_t np2_cap)
{
    __shared__ uint32_t s_cnt[2][kCvWaves];
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(cv_lds);
    unsigned short* feat_of = reinterpret_cast<unsigned short*>(cv_lds + sizeof(unsigned long long) * (size_t)np2_cap);
    const size_t slot = blockIdx.x;
    const uint32_t tid = threadIdx.x, t = (uint32_t)(slot / a.st.limit);
    const uint32_t start = a.tot[t] + a.local[slot], count = a.slot_count[slot];
    if (tid == 0) a.lm_start[slot] = start;
    if (count == 0u) return;
    // an emitted slot: its target is inside the table, the landmarks of its features have been looked at
    const uint32_t v = a.targets[t];
    const uint32_t x[3] = {a.views[3 * slot], a.views[3 * slot + 1], a.views[3 * slot + 2]};
    const int vi = x[0] == v ? 0 : x[1] == v ? 1 : 2, ai = vi == 0 ? 1 : 0, bi = vi == 2 ? 1 : 2;
    uint32_t tick = 0, run = 0;
    for (uint32_t j0 = 0; j0 < a.cap; j0 += kCvBlock) {
        const uint32_t j = j0 + tid;
        const uint32_t l = j < a.cap ? a.inv[(size_t)v * a.cap + j] : AKZ_CV_NONE;
        bool flag = false;
        uint32_t s = 0, e = 0, f;
        if (l != AKZ_CV_NONE && a.reason[l] == (unsigned char)AKZ_CV_TRI_OK) {
            s = a.obs_start[l];
            e = a.obs_start[l + 1];
            flag = akz_cv_find_view(a.obs, s, e, x[ai], &f) && akz_cv_find_view(a.obs, s, e, x[bi], &f);
        }
        uint32_t total;
        const uint32_t pos = run + akz_block_scan<kCvWaves>(s_cnt, tick, flag, &total);
        if (flag && pos < np2_cap) {
            keys[pos] = akz_cv_list_key(akz_cv_distinct_views(a.obs, s, e), a.st.seed, l, pos);
            feat_of[pos] = (unsigned short)j;
        }
        run += total;
    }
    run = run < np2_cap ? run : np2_cap;
    uint32_t np2 = 1;
    while (np2 < run) np2 <<= 1;
    for (uint32_t k = run + tid; k < np2; k += kCvBlock) keys[k] = ~0ull;
    __syncthreads();
    if (np2 >= 2u) bitonic_sort_lds_u64<kCvBlock>(keys, np2);
    uint32_t take = count < a.st.maximum_landmarks ? count : a.st.maximum_landmarks;
    take = take < run ? take : run;
    for (uint32_t k = tid; k < take; k += kCvBlock) {
        const uint32_t j = feat_of[akz_cv_list_key_pos(keys[k])];
        const uint32_t l = a.inv[(size_t)v * a.cap + j], s = a.obs_start[l], e = a.obs_start[l + 1];
        uint32_t fa = 0, fb = 0;
        akz_cv_find_view(a.obs, s, e, x[ai], &fa);
        akz_cv_find_view(a.obs, s, e, x[bi], &fb);
        uint32_t* row = a.lm + 3 * ((size_t)start + k);
        row[vi] = j;
        row[ai] = fa;
        row[bi] = fb;
    }
}

__global__ __launch_bounds__(kCvBlock) void k_cv_record(const uint32_t* __restrict__ constraint_verdict, const uint32_t* __restrict__ targets,
                                                        uint32_t n_targets, const uint32_t* __restrict__ graph_start, uint32_t n_graphs,
                                                        akz_cv_settings st, uint32_t* __restrict__ recorded, uint32_t* __restrict__ verdict,
                                                        uint32_t* __restrict__ stats)
{
    const uint32_t t = blockIdx.x * kCvBlock + threadIdx.x;
    if (t >= n_targets) return;
    const size_t slot0 = (size_t)t * st.limit;
    uint32_t n = 0u;
    int out = (int)verdict[t];
    if (out == AKZ_CV_OK || out == AKZ_CV_FEW_CONSTRAINTS || out == AKZ_CV_NO_GRAPH) {
        const uint32_t views = akz_cv_graph_views(graph_start, n_graphs, targets[t]);
        out = views == AKZ_CV_NONE ? AKZ_CV_NO_GRAPH : AKZ_CV_OK;
        if (views != AKZ_CV_NONE) out = akz_cv_record(constraint_verdict + slot0, &st, views, recorded + slot0, &n);
    }
    if (out != AKZ_CV_OK && out != AKZ_CV_FEW_CONSTRAINTS)
        for (uint32_t k = 0; k < st.limit; ++k)
            recorded[slot0 + k] = constraint_verdict[slot0 + k] != 0u ? constraint_verdict[slot0 + k] : (uint32_t)AKZ_CV_NOT_RECORDED;
    verdict[t] = (uint32_t)out;
    stats[(size_t)AKZ_CV_STATS * t + AKZ_CV_S_RECORDED] = n;
}

// ---- rs_pose_graph_rows_device ----
__global__ __launch_bounds__(kCvBlock) void k_pgr_count(const uint32_t* __restrict__ views, uint32_t n, uint32_t n_views, uint32_t* cnt, uint32_t* flags)
{
    const uint32_t c = blockIdx.x * kCvBlock + threadIdx.x;
    if (c >= n) return;
    const uint32_t x0 = views[3 * (size_t)c], x1 = views[3 * (size_t)c + 1], x2 = views[3 * (size_t)c + 2];
    if (x0 >= n_views || x1 >= n_views || x2 >= n_views) {
        atomicOr(flags, 1u);
        return;
    }
    atomicAdd(&cnt[x0], 2u);
    atomicAdd(&cnt[x1], 2u);
    atomicAdd(&cnt[x2], 2u);
}
// ONE workgroup: counts -> row_start
__global__ __launch_bounds__(kCvBlock) void k_pgr_scan(const uint32_t* __restrict__ cnt, uint32_t n_views, uint32_t* row_start)
{
    __shared__ uint32_t s_wave[kCvWaves];
    const uint32_t carry = tbl_scan<kCvWaves>(cnt, row_start, n_views, s_wave);
    if (threadIdx.x == 0) row_start[n_views] = carry;
}
// The ordered fill: the key of row entry e = 6 c + s is view << 32 | e (all ones for an entry of a triple outside the table and
// for the padding up to a power of two), and the ascending sort of the keys IS the rows one after another, each ascending —
// a bitonic network over global memory, n log^2 n compare-exchanges whatever the rows' lengths: strides of kPgrChunk keys and
// more are one launch each (k_pgr_merge_global), the strides below it run chunk by chunk in LDS (k_pgr_sort_local).  The order of the launches on the stream is the order of the stages.
constexpr uint32_t kPgrChunk = 2048;                                   // keys a workgroup holds in LDS (16 KB)
__global__ __launch_bounds__(kCvBlock) void k_pgr_keys(const uint32_t* __restrict__ views, uint32_t n, uint32_t n_views, uint32_t np2,
                                                       unsigned long long* __restrict__ keys)
{
    const uint32_t e = blockIdx.x * kCvBlock + threadIdx.x;
    if (e >= np2) return;
    unsigned long long key = ~0ull;
    if (e / 6u < n) {
        const uint32_t c = e / 6u, s = e % 6u;
        const uint32_t x0 = views[3 * (size_t)c], x1 = views[3 * (size_t)c + 1], x2 = views[3 * (size_t)c + 2];
        if (x0 < n_views && x1 < n_views && x2 < n_views) key = (unsigned long long)(AKZ_CV_SLOT_TARGET(s) == 0 ? x0 : AKZ_CV_SLOT_TARGET(s) == 1 ? x1 : x2) << 32 | e;
    }
    keys[e] = key;
}
// strides jstart, jstart / 2, ..., 1 of merge level k2 on the chunk in LDS whose first key is key gbase of the array
__device__ __forceinline__ void pgr_local_passes(unsigned long long* lds, uint32_t gbase, uint32_t k2, uint32_t jstart)
{
    for (uint32_t j = jstart; j > 0; j >>= 1) {
        for (uint32_t t = threadIdx.x; t < kPgrChunk / 2; t += kCvBlock) {
            const uint32_t i = ((t & ~(j - 1u)) << 1) | (t & (j - 1u)), ixj = i | j;
            const unsigned long long a = lds[i], b = lds[ixj];
            const bool up = ((gbase + i) & k2) == 0;
            if ((a > b) == up) {
                lds[i] = b;
                lds[ixj] = a;
            }
        }
        __syncthreads();
    }
}
// every merge level up to kPgrChunk inside a chunk (first = true), or the strides below kPgrChunk of level k2
__global__ __launch_bounds__(kCvBlock) void k_pgr_sort_local(unsigned long long* keys, uint32_t k2, bool first)
{
    __shared__ unsigned long long s_keys[kPgrChunk];
    const uint32_t base = blockIdx.x * kPgrChunk;                      // the array is a multiple of kPgrChunk long
    for (uint32_t i = threadIdx.x; i < kPgrChunk; i += kCvBlock) s_keys[i] = keys[base + i];
    __syncthreads();
    if (first)
        for (uint32_t k = 2; k <= kPgrChunk; k <<= 1) pgr_local_passes(s_keys, base, k, k >> 1);
    else
        pgr_local_passes(s_keys, base, k2, kPgrChunk >> 1);
    for (uint32_t i = threadIdx.x; i < kPgrChunk; i += kCvBlock) keys[base + i] = s_keys[i];
}
__global__ __launch_bounds__(kCvBlock) void k_pgr_merge_global(unsigned long long* keys, uint32_t np2, uint32_t k2, uint32_t j)
{
    const uint32_t t = blockIdx.x * kCvBlock + threadIdx.x;
    if (t >= np2 / 2) return;
    const uint32_t i = ((t & ~(j - 1u)) << 1) | (t & (j - 1u)), ixj = i | j;                  // below np2
    const unsigned long long a = keys[i], b = keys[ixj];
    const bool up = (i & k2) == 0;
    if ((a > b) == up) {
        keys[i] = b;
        keys[ixj] = a;
    }
}
__global__ __launch_bounds__(kCvBlock) void k_pgr_emit(const unsigned long long* __restrict__ keys, uint32_t n_entries, uint32_t* __restrict__ row_edges)
{
    const uint32_t i = blockIdx.x * kCvBlock + threadIdx.x;
    if (i >= n_entries) return;
    const unsigned long long key = keys[i];
    row_edges[i] = key == ~0ull ? 0u : (uint32_t)key;
}

int32_t cv_settings(const rs_covisibility_params* prm, akz_cv_settings* st)
{
    if (!prm || prm->struct_size != sizeof(rs_covisibility_params)) return AKZ_E_INVALID;
    if (prm->optimization_maximum_landmarks > (uint32_t)RS_TVC_MAX_LANDMARKS) return AKZ_E_TOO_LARGE;
    if (prm->optimization_minimum_landmarks > prm->optimization_maximum_landmarks) return AKZ_E_INVALID;
    if (prm->candidate_limit > (uint32_t)RS_CV_MAX_SLOTS) return AKZ_E_TOO_LARGE;
    const uint32_t limit = prm->candidate_limit ? prm->candidate_limit : prm->optimization_maximum_three_view_constraints;
    if (limit > (uint32_t)RS_CV_MAX_SLOTS) return AKZ_E_TOO_LARGE;
    if (limit == 0) return AKZ_E_INVALID;
    st->covisibility_minimum = prm->optimization_robust_covisibility_minimum_landmarks;
    st->maximum_constraints = prm->optimization_maximum_three_view_constraints;
    st->minimum_new = prm->optimization_minimum_new_constraints;
    st->minimum_landmarks = prm->optimization_minimum_landmarks;
    st->maximum_landmarks = prm->optimization_maximum_landmarks;
    st->limit = limit;
    st->seed = prm->shuffle_seed;
    return AKZ_OK;
}

uint32_t cv_np2(uint32_t n)
{
    uint32_t p = 1;
    while (p < n) p <<= 1;
    return p;
}

}   // namespace

extern "C" int32_t rs_covisibility_params_default(rs_covisibility_params* prm)
{
    if (!prm) return AKZ_E_INVALID;
    prm->struct_size = sizeof(rs_covisibility_params);
    prm->optimization_robust_covisibility_minimum_landmarks = 16;   // cv-sfm/src/settings.rs:453-475
    prm->optimization_maximum_three_view_constraints = 64;
    prm->optimization_minimum_new_constraints = 4;
    prm->optimization_minimum_landmarks = 24;
    prm->optimization_maximum_landmarks = 64;
    prm->candidate_limit = 0;
    prm->shuffle_seed = 0;
    return AKZ_OK;
}

extern "C" int32_t rs_covisibility_candidates_device(rs_ctx* c, const void* d_obs_start, const void* d_obs, uint32_t n_obs, uint32_t n_landmarks,
                                                     uint32_t cap_per_img, uint32_t n_blocks, const void* d_reason, const void* d_targets,
                                                     uint32_t n_targets, const rs_covisibility_params* prm, void* d_views, void* d_lm_start,
                                                     void* d_lm, void* d_slot_count, void* d_target_verdict, void* d_stats, void* stream_to_wait)
{
    return akz_guard([&]() -> int32_t {
        akz_cv_settings st;
        AKZ_TRY(cv_settings(prm, &st));
        if (!c || !d_obs_start || (n_obs != 0 && !d_obs) || (n_landmarks != 0 && !d_reason) || !d_lm_start) return AKZ_E_INVALID;
        if (n_targets != 0 && (!d_targets || !d_views || !d_slot_count || !d_target_verdict || !d_stats)) return AKZ_E_INVALID;
        if (cap_per_img == 0 || n_blocks == 0 || n_landmarks == 0xFFFFFFFFu || n_obs == 0xFFFFFFFFu) return AKZ_E_INVALID;
        if (cap_per_img > (uint32_t)RS_CV_MAX_FEATURES) return AKZ_E_TOO_LARGE;
        const size_t n_slots = (size_t)n_targets * st.limit, n_lm = n_slots * st.maximum_landmarks;
        if (n_lm >= 0xFFFFFFFFull || n_slots >= 0xFFFFFFFFull) return AKZ_E_TOO_LARGE;
        if (n_lm != 0 && !d_lm) return AKZ_E_INVALID;
        const RsHandles h = rs_internal_handles(c);
        AKZ_TRY(akz_enqueue_behind(h, stream_to_wait));
        RsCovisibilityState* cs = rs_internal_covisibility(c);
        const uint32_t groups = n_targets < kCvGroups ? n_targets : kCvGroups;
        const uint32_t wmax = (cap_per_img + 63u) / 64u;
        const size_t inv_bytes = akz_align_up(sizeof(uint32_t) * (size_t)n_blocks * cap_per_img, 256);
        const size_t bad_bytes = akz_align_up((size_t)n_landmarks + 1, 256);
        const size_t flag_bytes = 256;
        const size_t local_bytes = akz_align_up(sizeof(uint32_t) * (n_slots + 1), 256);
        const size_t tot_bytes = akz_align_up(sizeof(uint32_t) * ((size_t)n_targets + 1), 256);
        const size_t cnt_bytes = akz_align_up(sizeof(uint32_t) * (size_t)groups * n_blocks, 256);
        const size_t feat_bytes = akz_align_up(sizeof(uint32_t) * (size_t)groups * cap_per_img, 256);
        const size_t rows_bytes = akz_align_up(sizeof(uint64_t) * (size_t)groups * AKZ_CV_MAX_CANDIDATE_VIEWS * wmax, 256);
        AKZ_TRY(akz_grow_scratch(h.stream, &cs->d_scratch, &cs->bytes,
                                 inv_bytes + bad_bytes + flag_bytes + local_bytes + tot_bytes + cnt_bytes + feat_bytes + rows_bytes));
        char* base = (char*)cs->d_scratch;
        CvCall a;
        a.obs_start = (const uint32_t*)d_obs_start; a.obs = (const uint32_t*)d_obs; a.reason = (const unsigned char*)d_reason;
        a.targets = (const uint32_t*)d_targets; a.views = (uint32_t*)d_views; a.lm_start = (uint32_t*)d_lm_start; a.lm = (uint32_t*)d_lm;
        a.slot_count = (uint32_t*)d_slot_count; a.verdict = (uint32_t*)d_target_verdict; a.stats = (uint32_t*)d_stats;
        a.inv = (uint32_t*)base; base += inv_bytes;
        a.lm_bad = (unsigned char*)base; base += bad_bytes;
        a.flags = (uint32_t*)base; base += flag_bytes;
        a.local = (uint32_t*)base; base += local_bytes;
        a.tot = (uint32_t*)base; base += tot_bytes;
        a.g_cnt = (uint32_t*)base; base += cnt_bytes;
        a.g_feat = (uint32_t*)base; base += feat_bytes;
        a.g_rows = (unsigned long long*)base;
        a.n_obs = n_obs; a.n_landmarks = n_landmarks; a.cap = cap_per_img; a.n_blocks = n_blocks; a.n_targets = n_targets; a.wmax = wmax;
        a.st = st;
        AKZ_HIP(hipMemsetAsync(a.inv, 0xFF, sizeof(uint32_t) * (size_t)n_blocks * cap_per_img, h.stream));
        AKZ_HIP(hipMemsetAsync(a.flags, 0, sizeof(uint32_t), h.stream));
        if (n_targets) AKZ_HIP(hipMemsetAsync(a.g_cnt, 0, sizeof(uint32_t) * (size_t)groups * n_blocks, h.stream));
        if (n_lm) AKZ_HIP(hipMemsetAsync(d_lm, 0, sizeof(uint32_t) * 3 * n_lm, h.stream));
        if (n_landmarks) {
            hipLaunchKernelGGL(k_cv_scatter, dim3((n_landmarks + kCvBlock - 1) / kCvBlock), dim3(kCvBlock), 0, h.stream, a);
            AKZ_LAUNCH_CHECK();
        }
        if (n_targets) {
            AKZ_HIP(hipFuncSetAttribute((const void*)k_cv_targets, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kCvKeyBytes));
            hipLaunchKernelGGL(k_cv_targets, dim3(groups), dim3(kCvBlock), kCvKeyBytes, h.stream, a);
            AKZ_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(k_cv_scan, dim3(1), dim3(kCvBlock), 0, h.stream, a);
        AKZ_LAUNCH_CHECK();
        if (n_slots) {
            const uint32_t np2_cap = cv_np2(cap_per_img);
            const size_t lds = (sizeof(uint64_t) + sizeof(uint16_t)) * (size_t)np2_cap;
            if (lds > 65536) AKZ_HIP(hipFuncSetAttribute((const void*)k_cv_lists, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL(k_cv_lists, dim3((uint32_t)n_slots), dim3(kCvBlock), lds, h.stream, a, np2_cap);
            AKZ_LAUNCH_CHECK();
        }
        return AKZ_OK;
    });
}

extern "C" int32_t rs_covisibility_record_device(rs_ctx* c, const void* d_constraint_verdict, const void* d_targets, uint32_t n_targets,
                                                 const void* d_graph_start, uint32_t n_graphs, const rs_covisibility_params* prm, void* d_recorded,
                                                 void* d_target_verdict, void* d_stats, void* stream_to_wait)
{
    return akz_guard([&]() -> int32_t {
        akz_cv_settings st;
        AKZ_TRY(cv_settings(prm, &st));
        if (!c || !d_graph_start) return AKZ_E_INVALID;
        if (n_targets != 0 && (!d_constraint_verdict || !d_targets || !d_recorded || !d_target_verdict || !d_stats)) return AKZ_E_INVALID;
        if ((size_t)n_targets * st.limit >= 0xFFFFFFFFull) return AKZ_E_TOO_LARGE;
        const RsHandles h = rs_internal_handles(c);
        AKZ_TRY(akz_enqueue_behind(h, stream_to_wait));
        if (n_targets == 0) return AKZ_OK;
        hipLaunchKernelGGL(k_cv_record, dim3((n_targets + kCvBlock - 1) / kCvBlock), dim3(kCvBlock), 0, h.stream,
                           (const uint32_t*)d_constraint_verdict, (const uint32_t*)d_targets, n_targets, (const uint32_t*)d_graph_start, n_graphs,
                           st, (uint32_t*)d_recorded, (uint32_t*)d_target_verdict, (uint32_t*)d_stats);
        AKZ_LAUNCH_CHECK();
        return AKZ_OK;
    });
}

extern "C" int32_t rs_pose_graph_rows_device(rs_ctx* c, const void* d_views, uint32_t n_constraints, uint32_t n_views, void* d_row_start,
                                             void* d_row_edges, void* d_flags, void* stream_to_wait)
{
    return akz_guard([&]() -> int32_t {
        if (!c || !d_row_start || !d_flags || (n_constraints != 0 && (!d_views || !d_row_edges))) return AKZ_E_INVALID;
        if (n_views == 0xFFFFFFFFu) return AKZ_E_INVALID;
        if ((size_t)n_constraints * 6 > 0x80000000ull) return AKZ_E_TOO_LARGE;   // the keys are padded to a power of two
        const RsHandles h = rs_internal_handles(c);
        AKZ_TRY(akz_enqueue_behind(h, stream_to_wait));
        RsCovisibilityState* cs = rs_internal_covisibility(c);
        const uint32_t n_entries = 6u * n_constraints;
        uint32_t np2 = kPgrChunk;
        while (np2 < n_entries) np2 <<= 1;
        const size_t cur_bytes = akz_align_up(sizeof(uint32_t) * ((size_t)n_views + 1), 256);
        const size_t key_bytes = sizeof(unsigned long long) * (size_t)np2;
        AKZ_TRY(akz_grow_scratch(h.stream, &cs->d_scratch, &cs->bytes, cur_bytes + key_bytes));
        uint32_t* cnt = (uint32_t*)cs->d_scratch;
        unsigned long long* keys = (unsigned long long*)((char*)cs->d_scratch + cur_bytes);
        AKZ_HIP(hipMemsetAsync(cnt, 0, cur_bytes, h.stream));
        AKZ_HIP(hipMemsetAsync(d_flags, 0, sizeof(uint32_t), h.stream));
        if (n_constraints) {
            hipLaunchKernelGGL(k_pgr_count, dim3((n_constraints + kCvBlock - 1) / kCvBlock), dim3(kCvBlock), 0, h.stream, (const uint32_t*)d_views,
                               n_constraints, n_views, cnt, (uint32_t*)d_flags);
            AKZ_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(k_pgr_scan, dim3(1), dim3(kCvBlock), 0, h.stream, cnt, n_views, (uint32_t*)d_row_start);
        AKZ_LAUNCH_CHECK();
        if (n_constraints) {
            hipLaunchKernelGGL(k_pgr_keys, dim3(np2 / kCvBlock), dim3(kCvBlock), 0, h.stream, (const uint32_t*)d_views, n_constraints, n_views, np2, keys);
            AKZ_LAUNCH_CHECK();
            hipLaunchKernelGGL(k_pgr_sort_local, dim3(np2 / kPgrChunk), dim3(kCvBlock), 0, h.stream, keys, 0u, true);
            AKZ_LAUNCH_CHECK();
            for (uint32_t k2 = 2 * kPgrChunk; k2 <= np2 && k2 != 0; k2 <<= 1) {
                for (uint32_t j = k2 >> 1; j >= kPgrChunk; j >>= 1) {
                    hipLaunchKernelGGL(k_pgr_merge_global, dim3(np2 / 2 / kCvBlock), dim3(kCvBlock), 0, h.stream, keys, np2, k2, j);
                    AKZ_LAUNCH_CHECK();
                }
                hipLaunchKernelGGL(k_pgr_sort_local, dim3(np2 / kPgrChunk), dim3(kCvBlock), 0, h.stream, keys, k2, false);
                AKZ_LAUNCH_CHECK();
            }
            hipLaunchKernelGGL(k_pgr_emit, dim3((n_entries + kCvBlock - 1) / kCvBlock), dim3(kCvBlock), 0, h.stream, keys, n_entries, (uint32_t*)d_row_edges);
            AKZ_LAUNCH_CHECK();
        }
        return AKZ_OK;
    });
}
