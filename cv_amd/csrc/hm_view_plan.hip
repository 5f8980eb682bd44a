// hm_view_plan.hip — from the frames found for a micro-batch to its searches, on the device: hm_view_plan_device,
// hm_knn_planned_batch_device of include/akz.h.
//   try_localize: one reconstruction per turn, most views found first          cv-sfm/src/lib.rs:858-891
//   try_localize_and_incorporate: .remove(&reconstruction)                      cv-sfm/src/lib.rs:926-939
//   register_frame_subset: knn(., 3) against every view of the list it is given cv-sfm/src/lib.rs:1472-1486
// hm_find_frames_batch_device leaves, per new frame, the found views by reconstruction.  Here a frame takes ONE of those groups
// (k_vp_pick, a wave per frame: the lanes look for the group, copy its first n_views keys and test every key against the block
// count before anything is read through it), the distinct target blocks of the whole call are counted and ranked (k_vp_mark: a
// plain store of 1 into a flag word per block, same-value races; k_vp_scan: ONE workgroup, the exclusive scan of the flags
// behind a running carry, so that no workgroup waits for another), and the tables the matcher's kernels read are written where
// the host used to write them (k_vp_tables: an expand job per frame's query block and per distinct target block in ascending
// block order, a problem per (frame, view)).  The grids of the expand and the search come from the rooms alone; a job or a
// problem without work names a zero count, and the matcher's workgroups leave on their own first test.  Nothing is read back.
// Every decision is include/akz_view_plan_math.h's, the text the host build compiles too.  The search kernels are
// hm_match.hip's and are launched there (hm_internal_planned of hm_tables.h).
#include "hm_tables.h"
#include "rs_table.h"
#include "../../include/akz_view_plan_math.h"

static_assert(HM_VP_OK == AKZ_VP_OK && HM_VP_CUT == AKZ_VP_CUT && HM_VP_NO_GROUP == AKZ_VP_NO_GROUP && HM_VP_FIND_REFUSED == AKZ_VP_FIND_REFUSED &&
              HM_VP_BAD_VIEW == AKZ_VP_BAD_VIEW && HM_VP_NO_ROOM == AKZ_VP_NO_ROOM, "verdicts");
static_assert(HM_VP_C_BLOCKS == AKZ_VP_C_BLOCKS && HM_VP_C_LIVE == AKZ_VP_C_LIVE && HM_VP_C_VERDICT == AKZ_VP_C_VERDICT &&
              HM_VP_C_FRAMES == AKZ_VP_C_FRAMES && HM_VP_COUNTS == AKZ_VP_COUNTS, "counts");
static_assert(HM_VP_PICK_RECON == AKZ_VP_PICK_RECON && HM_VP_MAX_VIEWS == AKZ_VP_MAX_VIEWS && AKZ_VP_MAX_VIEWS <= 64, "a wave holds a frame's list");
static_assert(sizeof(HmProb) == sizeof(HmProbX), "one room for either table");

namespace {

constexpr uint32_t kVpCapLimit = 1u << 21;     // rows of a block: what hm_knn_batch_device takes (the packed keys of the search)
constexpr int kVpScanThreads = 1024, kVpScanWaves = kVpScanThreads / 64;

// ---- one frame: its group, its list, its verdict ---------------------------------------------------------------------------------
struct VpPick {
    const uint32_t *views_out, *group_recon, *group_start, *counts, *find_verdict, *pick;
    uint32_t room, flags, n_frames, n_views, n_blocks;
    uint32_t *view_idx, *frame_views, *verdict;
};

__global__ __launch_bounds__(256) void k_vp_pick(const VpPick A)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t f = blockIdx.x * 4u + (threadIdx.x >> 6);          // a wave per frame
    if (f >= A.n_frames) return;
    const size_t row = (size_t)f * A.room;
    uint32_t verdict, taken = 0u, key = AKZ_PL_NONE;
    if (A.find_verdict[f] != (uint32_t)AKZ_PL_OK) {
        verdict = AKZ_VP_FIND_REFUSED;
    } else {
        const uint32_t n_groups = akz_vp_groups(A.counts[(size_t)f * AKZ_PL_COUNTS + AKZ_PL_C_GROUPS], A.room);
        const bool has_pick = A.pick != nullptr;
        const uint32_t pick = has_pick ? A.pick[f] : 0u;
        uint32_t g = AKZ_PL_NONE;
        if (has_pick && (A.flags & (uint32_t)AKZ_VP_PICK_RECON)) {
            for (uint32_t g0 = 0; g0 < n_groups && g == AKZ_PL_NONE; g0 += 64u) {
                const uint32_t k = g0 + lane;
                const unsigned long long hit = __ballot(k < n_groups && akz_vp_group_is(A.group_recon[row + (k < n_groups ? k : 0u)], pick));
                if (hit) g = g0 + (uint32_t)__ffsll((long long)hit) - 1u;
            }
        } else {
            g = akz_vp_group_by_ordinal(has_pick, pick, n_groups);
        }
        if (g == AKZ_PL_NONE) {
            verdict = AKZ_VP_NO_GROUP;
        } else {
            const uint32_t* const gs = A.group_start + (size_t)f * (A.room + 1u);
            uint32_t start;
            const uint32_t length = akz_vp_group_span(gs[g], gs[g + 1u], A.room, &start);
            taken = akz_vp_taken(length, A.n_views);
            if (lane < taken) key = A.views_out[row + start + lane];
            verdict = akz_vp_list_verdict(length, A.n_views);
            if (__ballot(lane < taken && !akz_vp_key_ok(key, A.n_blocks))) {      // the frame is refused alone
                verdict = AKZ_VP_BAD_VIEW;
                taken = 0u;
            }
        }
    }
    if (lane < A.n_views) A.view_idx[(size_t)f * A.n_views + lane] = lane < taken ? key : AKZ_PL_NONE;
    if (lane == 0u) {
        A.frame_views[f] = taken;
        A.verdict[f] = verdict;
    }
}

// ---- the distinct target blocks of the call ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_vp_mark(const uint32_t* __restrict__ view_idx, const uint32_t* __restrict__ frame_views, uint32_t n_frames,
                                                 uint32_t n_views, uint32_t n_blocks, uint32_t* __restrict__ flag)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_frames * n_views) return;
    const uint32_t f = i / n_views, v = i - f * n_views, key = view_idx[i];
    if (akz_vp_live(v, frame_views[f], n_views, key, n_blocks)) flag[key] = 1u;       // (every writer stores the same word)
}

// words of the scratch's head
enum { kVpHeadDistinct = 0, kVpHeadVerdict = 1 };

// ONE workgroup: flag -> rank (the blocks marked below a block), the count and the call's verdict; for hm_view_plan_device
// (plan_counts given) the frames' rows are closed too: a call without room leaves no frame a list.
__global__ __launch_bounds__(kVpScanThreads) void k_vp_scan(const uint32_t* __restrict__ flag, uint32_t n_blocks, uint32_t exp_blocks,
                                                            uint32_t* __restrict__ rank, uint32_t* __restrict__ head, uint32_t n_frames,
                                                            uint32_t n_views, uint32_t* __restrict__ view_idx, uint32_t* __restrict__ frame_views,
                                                            uint32_t* __restrict__ plan_counts)
{
    __shared__ uint32_t s_wave[kVpScanWaves];
    __shared__ uint32_t s_cnt[2][kVpScanWaves];
    const uint32_t carry = tbl_scan<kVpScanWaves>(flag, rank, n_blocks, s_wave);
    const uint32_t call = akz_vp_call_verdict(carry, exp_blocks);
    if (threadIdx.x == 0) {
        head[kVpHeadDistinct] = carry;
        head[kVpHeadVerdict] = call;
    }
    if (!plan_counts) return;
    uint32_t live = 0u, frames = 0u, tick = 0u;
    if (call != (uint32_t)AKZ_VP_OK) {
        for (uint32_t i = threadIdx.x; i < n_frames * n_views; i += kVpScanThreads) view_idx[i] = AKZ_PL_NONE;
        for (uint32_t f = threadIdx.x; f < n_frames; f += kVpScanThreads) frame_views[f] = 0u;
    } else {
        for (uint32_t f = threadIdx.x; f < n_frames; f += kVpScanThreads) {
            live += frame_views[f];
            frames += frame_views[f] != 0u;
        }
    }
    live = akz_block_sum<kVpScanWaves>(s_cnt, tick, live);
    frames = akz_block_sum<kVpScanWaves>(s_cnt, tick, frames);
    if (threadIdx.x == 0) {
        plan_counts[AKZ_VP_C_BLOCKS] = carry;
        plan_counts[AKZ_VP_C_LIVE] = live;
        plan_counts[AKZ_VP_C_VERDICT] = call;
        plan_counts[AKZ_VP_C_FRAMES] = frames;
    }
}

// ---- the tables the expand and the search read ---------------------------------------------------------------------------------------
// Jobs [n_frames + exp_blocks]: job f recodes frame f's query block; job n_frames + r the r-th distinct target block in ascending
// block order; the slots behind the distinct count, and every slot of a call without room, name the zero word.  Problems
// [n_frames][n_views]: a live one finds its queries at job f's place and its targets at the place of its block's rank; a dead
// one names the zero word on both sides.  No entry depends on the order the threads arrive in.
struct VpTables {
    const uint32_t *view_idx, *frame_views, *flag, *rank, *head, *zero, *iq;
    uint32_t n_frames, n_views, n_blocks, exp_blocks, cap, words, k, valu;
    const uint32_t *q, *nq, *t, *nt;
    uint32_t* exp;
    akz_neighbor* out;
    HmExpandJob* jobs;
    void* probs;
};

__global__ __launch_bounds__(256) void k_vp_tables(const VpTables A)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const uint32_t distinct = A.head[kVpHeadDistinct];
    const bool room = A.head[kVpHeadVerdict] == (uint32_t)AKZ_VP_OK;
    const size_t block_words = (size_t)A.cap * A.words;
    if (!A.valu) {
        if (i < A.n_frames) {
            const uint32_t b = A.iq[i];
            A.jobs[i] = room ? HmExpandJob{A.q + (size_t)b * A.cap * 16u, A.nq + b, A.cap, A.exp + (size_t)i * block_words}
                             : HmExpandJob{A.q, A.zero, A.cap, A.exp};
        }
        if (room && i < A.n_blocks && A.flag[i])
            A.jobs[A.n_frames + A.rank[i]] = HmExpandJob{A.t + (size_t)i * A.cap * 16u, A.nt + i, A.cap, A.exp + (size_t)(A.n_frames + A.rank[i]) * block_words};
        if (i < A.exp_blocks && (!room || i >= distinct)) A.jobs[A.n_frames + i] = HmExpandJob{A.t, A.zero, A.cap, A.exp};
    }
    if (i < A.n_frames * A.n_views) {
        const uint32_t f = i / A.n_views, v = i - f * A.n_views, key = A.view_idx[i];
        const bool live = room && akz_vp_live(v, A.frame_views[f], A.n_views, key, A.n_blocks);
        akz_neighbor* const out = A.out + (size_t)i * A.cap * A.k;
        if (A.valu) {
            const uint4* const q = reinterpret_cast<const uint4*>(A.q);
            const uint4* const t = reinterpret_cast<const uint4*>(A.t);
            static_cast<HmProb*>(A.probs)[i] = live ? HmProb{q + (size_t)A.iq[f] * A.cap * 4u, A.nq + A.iq[f], A.cap, t + (size_t)key * A.cap * 4u, A.nt + key, A.cap, out}
                                                    : HmProb{q, A.zero, A.cap, t, A.zero, A.cap, out};
        } else {
            static_cast<HmProbX*>(A.probs)[i] = live ? HmProbX{A.exp + (size_t)f * block_words, A.nq + A.iq[f], A.cap,
                                                               A.exp + (size_t)(A.n_frames + A.rank[key]) * block_words, A.nt + key, A.cap, out}
                                                     : HmProbX{A.exp, A.zero, A.cap, A.exp, A.zero, A.cap, out};
        }
    }
}

// the scratch of a call, byte offsets: [zero words 64 B][head 64 B][flag n_blocks][rank n_blocks][jobs][problems]
struct VpScratch {
    size_t head, flag, rank, jobs, probs, bytes;
};
VpScratch vp_scratch(uint32_t n_blocks, uint32_t n_jobs, uint32_t n_probs)
{
    VpScratch s;
    s.head = 64;
    s.flag = 128;
    s.rank = s.flag + akz_align_up(sizeof(uint32_t) * (size_t)n_blocks, 64);
    s.jobs = s.rank + akz_align_up(sizeof(uint32_t) * (size_t)n_blocks, 64);
    s.probs = s.jobs + akz_align_up(sizeof(HmExpandJob) * (size_t)n_jobs, 64);
    s.bytes = s.probs + akz_align_up(sizeof(HmProbX) * (size_t)n_probs, 64);
    return s;
}

// the refusals both entry points share, from the arguments alone
int32_t vp_check(uint32_t n_frames, uint32_t n_views, uint32_t exp_blocks)
{
    if (n_views == 0u || n_views > (uint32_t)AKZ_VP_MAX_VIEWS || exp_blocks == 0u) return AKZ_E_INVALID;
    if ((uint64_t)n_frames * n_views > 65535u || (uint64_t)n_frames + exp_blocks > 65535u) return AKZ_E_INVALID;
    return AKZ_OK;
}

// clear the zero words, the head and the flags; mark; scan
int32_t vp_count_blocks(hipStream_t stream, unsigned char* d, const VpScratch& S, const uint32_t* view_idx, const uint32_t* frame_views,
                        uint32_t n_frames, uint32_t n_views, uint32_t n_blocks, uint32_t exp_blocks, uint32_t* w_view_idx, uint32_t* w_frame_views,
                        uint32_t* plan_counts)
{
    AKZ_HIP(hipMemsetAsync(d, 0, S.rank, stream));
    hipLaunchKernelGGL(k_vp_mark, dim3((n_frames * n_views + 255u) / 256u), dim3(256), 0, stream, view_idx, frame_views, n_frames, n_views, n_blocks,
                       reinterpret_cast<uint32_t*>(d + S.flag));
    AKZ_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_vp_scan, dim3(1), dim3(kVpScanThreads), 0, stream, reinterpret_cast<const uint32_t*>(d + S.flag), n_blocks, exp_blocks,
                       reinterpret_cast<uint32_t*>(d + S.rank), reinterpret_cast<uint32_t*>(d + S.head), n_frames, n_views, w_view_idx, w_frame_views,
                       plan_counts);
    AKZ_LAUNCH_CHECK();
    return AKZ_OK;
}

}   // namespace

extern "C" int32_t hm_view_plan_device(hm_ctx* c, const void* d_views_out, const void* d_group_recon, const void* d_group_start, const void* d_counts,
                                       const void* d_verdict, uint32_t room, const void* d_pick, uint32_t flags, uint32_t n_frames, uint32_t n_views,
                                       uint32_t n_blocks, uint32_t exp_blocks, void* d_view_idx, void* d_n_views, void* d_plan_verdict,
                                       void* d_plan_counts, void* stream_to_wait)
{
    return akz_guard([&]() -> int32_t {
        if (!d_views_out || !d_group_recon || !d_group_start || !d_counts || !d_verdict || !d_view_idx || !d_n_views || !d_plan_verdict || !d_plan_counts)
            return AKZ_E_INVALID;
        if (flags & ~(uint32_t)HM_VP_PICK_RECON) return AKZ_E_INVALID;
        AKZ_TRY(vp_check(n_frames, n_views, exp_blocks));
        if (!c) return AKZ_E_INVALID;
        if (n_frames == 0u) return AKZ_OK;
        const HmHandles h = hm_internal_handles(c);
        AKZ_TRY(akz_enqueue_behind(h.device, h.stream, h.ev, stream_to_wait));
        HmViewPlanState* vs = hm_internal_view_plan(c);
        const VpScratch S = vp_scratch(n_blocks, 0u, 0u);
        AKZ_TRY(akz_grow_scratch(h.stream, &vs->d_scratch, &vs->bytes, S.bytes));
        VpPick A;
        A.views_out = (const uint32_t*)d_views_out;
        A.group_recon = (const uint32_t*)d_group_recon;
        A.group_start = (const uint32_t*)d_group_start;
        A.counts = (const uint32_t*)d_counts;
        A.find_verdict = (const uint32_t*)d_verdict;
        A.pick = (const uint32_t*)d_pick;
        A.room = room;
        A.flags = flags;
        A.n_frames = n_frames;
        A.n_views = n_views;
        A.n_blocks = n_blocks;
        A.view_idx = (uint32_t*)d_view_idx;
        A.frame_views = (uint32_t*)d_n_views;
        A.verdict = (uint32_t*)d_plan_verdict;
        hipLaunchKernelGGL(k_vp_pick, dim3((n_frames + 3u) / 4u), dim3(256), 0, h.stream, A);
        AKZ_LAUNCH_CHECK();
        return vp_count_blocks(h.stream, (unsigned char*)vs->d_scratch, S, A.view_idx, A.frame_views, n_frames, n_views, n_blocks, exp_blocks,
                               A.view_idx, A.frame_views, (uint32_t*)d_plan_counts);
    });
}

extern "C" int32_t hm_knn_planned_batch_device(hm_ctx* c, const void* d_q, const void* d_nq, const void* d_t, const void* d_nt, uint32_t cap_per_img,
                                               const uint32_t* iq, const void* d_view_idx, const void* d_n_views, uint32_t n_frames, uint32_t n_views,
                                               uint32_t n_blocks, uint32_t exp_blocks, uint32_t k, void* d_out, void* stream_to_wait)
{
    return akz_guard([&]() -> int32_t {
        if (!d_q || !d_nq || !d_t || !d_nt || !iq || !d_view_idx || !d_n_views || !d_out || k < 1u || k > 3u) return AKZ_E_INVALID;
        if (cap_per_img == 0u || cap_per_img >= kVpCapLimit) return AKZ_E_INVALID;
        AKZ_TRY(vp_check(n_frames, n_views, exp_blocks));
        if (!c) return AKZ_E_INVALID;
        if (n_frames == 0u) return AKZ_OK;
        const HmHandles h = hm_internal_handles(c);
        AKZ_TRY(akz_enqueue_behind(h.device, h.stream, h.ev, stream_to_wait));
        HmPlannedSearch s{};
        s.iq = iq;
        s.n_frames = n_frames;
        s.exp_blocks = exp_blocks;
        s.n_probs = n_frames * n_views;
        s.cap = cap_per_img;
        s.k = (int)k;
        AKZ_TRY(hm_internal_planned(c, &s, false));
        HmViewPlanState* vs = hm_internal_view_plan(c);
        const VpScratch S = vp_scratch(n_blocks, n_frames + exp_blocks, s.n_probs);
        AKZ_TRY(akz_grow_scratch(h.stream, &vs->d_scratch, &vs->bytes, S.bytes));
        unsigned char* const d = (unsigned char*)vs->d_scratch;
        AKZ_TRY(vp_count_blocks(h.stream, d, S, (const uint32_t*)d_view_idx, (const uint32_t*)d_n_views, n_frames, n_views, n_blocks, exp_blocks, nullptr,
                                nullptr, nullptr));
        VpTables A;
        A.view_idx = (const uint32_t*)d_view_idx;
        A.frame_views = (const uint32_t*)d_n_views;
        A.flag = reinterpret_cast<const uint32_t*>(d + S.flag);
        A.rank = reinterpret_cast<const uint32_t*>(d + S.rank);
        A.head = reinterpret_cast<const uint32_t*>(d + S.head);
        A.zero = reinterpret_cast<const uint32_t*>(d);
        A.iq = s.d_iq;
        A.n_frames = n_frames;
        A.n_views = n_views;
        A.n_blocks = n_blocks;
        A.exp_blocks = exp_blocks;
        A.cap = cap_per_img;
        A.words = s.words;
        A.k = k;
        A.valu = s.valu ? 1u : 0u;
        A.q = (const uint32_t*)d_q;
        A.nq = (const uint32_t*)d_nq;
        A.t = (const uint32_t*)d_t;
        A.nt = (const uint32_t*)d_nt;
        A.exp = s.exp;
        A.out = (akz_neighbor*)d_out;
        A.jobs = reinterpret_cast<HmExpandJob*>(d + S.jobs);
        A.probs = d + S.probs;
        uint32_t items = s.n_probs > n_blocks ? s.n_probs : n_blocks;
        items = items > n_frames + exp_blocks ? items : n_frames + exp_blocks;
        hipLaunchKernelGGL(k_vp_tables, dim3((items + 255u) / 256u), dim3(256), 0, h.stream, A);
        AKZ_LAUNCH_CHECK();
        s.jobs = A.jobs;
        s.probs = A.probs;
        return hm_internal_planned(c, &s, true);
    });
}
