// rs_landmark_table.hip — the bookkeeping of cv-sfm's landmark table around the registration of a micro-batch on gfx950:
// are_landmarks_sharing_view for the merge candidates (cv-sfm/src/lib.rs:1435-1449) and VSlamData::add_view with
// merge_landmarks and add_landmark (lib.rs:432-500, 699-721) for the accepted frames, out of place.  Integer data movement
// over the CSR table rs_triangulate_landmarks_device reads; every decision is include/akz_landmark_table_math.h, the text the
// CPU checker (tests/cpp/landmark_table_host.c) compiles too — parity: host build == HIP, byte for byte.
//
// rs_landmarks_sharing_view_device is one kernel:
//   k_lt_sharing     one lane per feature of a slot.  A candidate whose two lists hold kLtShortPair entries or fewer together is
//                    walked by its lane; a longer one is handed to the whole wave, which strides over the second list (a list
//                    can be as long as there are views).
// rs_add_views_device, in stream order:
//   k_lt_check_table one lane per start: do the starts ascend inside [0, n_obs]?  (If not, everything behind describes an empty
//                    table.)
//   k_lt_validate    one workgroup per slot: accepted, not accepted or refused; the feature -> match map of the slot (which also
//                    finds a feature named twice); the pose of an accepted slot.
//   k_lt_refs        one lane per match: refs[l] over the final matches of the accepted slots.  A launch of its own behind the
//                    validation, so that a refused slot never counts.
//   k_lt_merges      one lane per match: adds[l], the observations a row gains, and the verdict on every merge from the complete
//                    refs — applied (merged_from[a] = b, merged_into[b] = a; refs == 1 on both sides makes the lane their only
//                    writer) or demoted.
//   k_lt_tile_sums   the exclusive scan of the row lengths over the rows of the input table, first level: one lane per row
//                    gives its length (to d_obs_counts_out), one workgroup per tile of kTblTile rows adds its tile.
//   k_lt_scan_sums   second level: ONE workgroup walks the tile sums kTblBlock at a time behind a running carry, then the new
//                    rows of the slots the same way; the counts and the call's verdict.
//   k_lt_rows        third pass: a workgroup scans its tile again, adds the tile's offset, writes the starts and copies each
//                    row's old list and the list merged into it (8-byte accesses).
//   k_lt_tail        the rows behind the input table: their starts are arithmetic (one observation each), the split list's rows
//                    are written here.
//   k_lt_place       one lane per match: the new observation goes behind its row's old part through a cursor per row.
//   k_lt_new_rows    one workgroup per slot: the features in no final match, compacted in feature order, one row each.
//   k_lt_fixup       one lane per row that gained two or more observations: its tail sorted into slot order, so that the
//                    bytes do not depend on the order the cursor was taken in.
// k_tbl_tail (rs_table.h), the tail of the stages whose rows behind the filled ones are all empty (rs_bootstrap_table.hip,
// rs_reconstruction_merge.hip), is defined here, beside the scratch those stages share.
// The landmark of every observation written goes to d_landmarks_out where the observation is written (atomicMin behind a fill
// of 0xFFFFFFFF: a feature a broken table lists twice gets its lowest key).  Nothing here waits on a value another workgroup
// has yet to write: the levels are separate launches; every loop is bounded by an argument of the call or a checked count.
#include "rs_table.h"
#include "../../include/akz_landmark_table_math.h"

__global__ __launch_bounds__(kTblBlock) void k_tbl_tail(uint32_t* obs_start_out, uint32_t* obs_counts_out, uint32_t first_row, uint32_t lm_room,
                                                        const uint32_t* rows, const uint32_t* total)
{
    const uint32_t k = blockIdx.x * kTblBlock + threadIdx.x;
    if (k > lm_room - first_row) return;
    const uint32_t r = first_row + k;
    if (r < *rows) return;
    obs_start_out[r] = *total;
    if (r < lm_room) obs_counts_out[r] = 0u;
}

namespace {

constexpr uint32_t kLtShortPair = 32;                        // combined length up to which one lane walks a candidate

static_assert(RS_AV_OK == AKZ_AV_OK && RS_AV_NOT_ACCEPTED == AKZ_AV_NOT_ACCEPTED && RS_AV_BAD_INDEX == AKZ_AV_BAD_INDEX &&
              RS_AV_BAD_TABLE == AKZ_AV_BAD_TABLE, "verdicts");
static_assert(RS_AV_S_OBSERVATIONS == AKZ_AV_S_OBSERVATIONS && RS_AV_S_MERGED == AKZ_AV_S_MERGED && RS_AV_S_DEMOTED == AKZ_AV_S_DEMOTED &&
              RS_AV_S_NEW_LANDMARKS == AKZ_AV_S_NEW_LANDMARKS && RS_AV_STATS == AKZ_AV_STATS && RS_AV_COUNTS == AKZ_AV_COUNTS, "stats words");
static_assert(RS_SV_OK == AKZ_LT_SV_OK, "the refinement's verdict that registers a frame");

// words of LtCall::info
enum { kInfoBad = 0, kInfoMerged = 1, kInfoDemoted = 2, kInfoOld = 3, kInfoRows = 4, kInfoSplit = 5, kInfoWords = 8 };

// everything the kernels of one call share, by value
struct LtCall {
    const uint32_t* obs_start;    // [n_landmarks + 1]
    const uint2* obs;             // [n_obs]
    const uint2* split;           // [split_room] or null
    const uint32_t* split_count;  // [1] or null
    const uint32_t* counts;       // [n_blocks]
    const uint32_t* matches;      // [F][cap][2]
    const uint32_t* nmatches;     // [F]
    const unsigned char* final_mask;   // [F][cap]
    const uint32_t* sv_verdict;   // [F]
    const double* pose_out;       // [F][12]
    const uint32_t* best;         // [F][cap][3][2] or null
    const uint32_t* skip;         // [F] or null
    double* poses;                // [n_blocks][12]
    uint32_t* obs_start_out;      // [lm_room + 1]
    uint2* obs_out;               // [obs_room]
    uint32_t* counts_out;         // [4]
    uint32_t* landmarks_out;      // [n_blocks][cap]
    uint32_t* obs_counts_out;     // [lm_room]
    uint32_t* frame_verdict;      // [F]
    uint32_t* stats;              // [F][AKZ_AV_STATS]
    uint32_t* call_verdict;       // [1]
    // scratch
    uint32_t* info;               // [kInfoWords]
    uint32_t* refs;               // [n_landmarks] final matches of accepted slots that name the landmark
    uint32_t* adds;               // [n_landmarks] observations the row gains
    uint32_t* cursor;             // [n_landmarks] how many of them are placed
    uint32_t* merged_into;        // [n_landmarks] a where the row is the b of an applied merge (a tombstone), else none
    uint32_t* merged_from;        // [n_landmarks] b where the row is the a of an applied merge, else none
    uint32_t* block_slot;         // [n_blocks] the slot whose frame is the block, else none
    uint32_t* tile;               // [n_tiles] a tile's sum, then its offset
    uint32_t* frames;             // [F] ik
    uint32_t* accepted;           // [F]
    uint32_t* new_rows;           // [F] rows the slot adds, then the rows of the slots in front of it
    uint32_t* feat;               // [F][cap] the final match that names the feature, else none
    uint32_t cap, n_blocks, n_obs, n_landmarks, n_world, split_room, n_frames, lm_room, n_tiles;
};

__global__ __launch_bounds__(kTblBlock) void k_lt_sharing(const uint32_t* __restrict__ obs_start, const uint32_t* __restrict__ obs,
                                                         uint32_t n_obs, uint32_t n_landmarks, const uint32_t* __restrict__ best,
                                                         const uint32_t* __restrict__ decision, uint32_t cap,
                                                         unsigned char* __restrict__ merge_ok)
{
    const uint32_t j = blockIdx.x * kTblBlock + threadIdx.x, lane = threadIdx.x & 63u;
    const size_t at = (size_t)blockIdx.y * cap + j;
    const bool valid = j < cap;
    const uint32_t fill = akz_lt_fill(obs_start, n_landmarks, n_obs);
    uint32_t sa = 0u, ea = 0u, sb = 0u, eb = 0u;
    const bool cand = valid && akz_lt_candidate(obs_start, n_landmarks, fill, decision[at], best + 6 * at, &sa, &ea, &sb, &eb);
    // a candidate's ranges lie inside [0, fill], fill <= n_obs: every observation read below is the table's
    const bool wide = cand && (ea - sa) + (eb - sb) > kLtShortPair;
    unsigned char ok = 0;
    if (cand && !wide) ok = akz_lt_lists_share(obs, sa, ea, sb, eb) ? 0 : 1;
    tbl_for_wide_rows(wide, [&](int src) {              // wave-uniform: every lane walks the same candidates
        const uint32_t wsa = __shfl(sa, src, 64), wea = __shfl(ea, src, 64), wsb = __shfl(sb, src, 64), web = __shfl(eb, src, 64);
        int share = 0;
        for (uint32_t q = wsb + lane; q < web && !share; q += 64u) share = akz_lt_lists_share(obs, wsa, wea, q, q + 1u);
        const int any = __any(share);
        if ((int)lane == src) ok = any ? 0 : 1;
    });
    if (valid) merge_ok[at] = ok;
}

__global__ __launch_bounds__(kTblBlock) void k_lt_check_table(LtCall a)
{
    const uint32_t l = blockIdx.x * kTblBlock + threadIdx.x;
    const int bad = l <= a.n_landmarks && akz_lt_start_bad(a.obs_start, l, a.n_landmarks, a.n_obs);
    tbl_flag(&a.info[kInfoBad], bad);
}

// what final match i of slot f names; only for i < nmatches[f] <= cap
__device__ __forceinline__ int lt_match(const LtCall& a, uint32_t f, uint32_t i, uint32_t count, uint32_t* feature, uint32_t* la, uint32_t* lb)
{
    const size_t at = (size_t)f * a.cap + i;
    *feature = a.matches[2 * at];
    return akz_lt_match(*feature, a.matches[2 * at + 1], count, f, a.cap, a.n_world, a.n_landmarks, a.best, la, lb);
}

// One workgroup per slot.  info, refs, adds, cursor are zero and merged_into, merged_from, block_slot none in front of it.
__global__ __launch_bounds__(kTblBlock) void k_lt_validate(LtCall a)
{
    __shared__ uint32_t s_bad, s_final;
    const uint32_t f = blockIdx.x, blk = a.frames[f];                     // blk < n_blocks: checked on the host
    const uint32_t count = a.counts[blk], nm = a.nmatches[f];
    const bool off = a.info[kInfoBad] != 0u || a.sv_verdict[f] != (uint32_t)AKZ_LT_SV_OK || (a.skip && a.skip[f] != 0u);
    uint32_t* feat = a.feat + (size_t)f * a.cap;
    for (uint32_t j = threadIdx.x; j < a.cap; j += kTblBlock) feat[j] = AKZ_LT_NONE;
    if (threadIdx.x == 0) {
        s_bad = (count > a.cap || nm > a.cap) ? 1u : 0u;
        s_final = 0u;
        a.block_slot[blk] = f;
    }
    __syncthreads();
    if (!off && s_bad == 0u) {                                           // nm <= cap, count <= cap
        uint32_t mine = 0u, bad = 0u;
        for (uint32_t i = threadIdx.x; i < nm; i += kTblBlock) {
            if (!a.final_mask[(size_t)f * a.cap + i]) continue;
            uint32_t feature, la, lb;
            if (lt_match(a, f, i, count, &feature, &la, &lb) == AKZ_LT_MATCH_BAD) bad = 1u;
            else if (atomicCAS(&feat[feature], AKZ_LT_NONE, i) != AKZ_LT_NONE) bad = 1u;     // feature < count <= cap
            else ++mine;
        }
        __syncthreads();                                                 // every thread has read s_bad
        if (bad) atomicOr(&s_bad, 1u);
        if (mine) atomicAdd(&s_final, mine);
    }
    __syncthreads();
    const bool accepted = !off && s_bad == 0u;
    if (threadIdx.x == 0) {
        const uint32_t n_final = accepted ? s_final : 0u, n_new = accepted ? count - s_final : 0u;   // the features named are distinct
        a.accepted[f] = accepted ? 1u : 0u;
        a.new_rows[f] = n_new;
        a.frame_verdict[f] = off ? AKZ_AV_NOT_ACCEPTED : accepted ? AKZ_AV_OK : AKZ_AV_BAD_INDEX;
        uint32_t* st = a.stats + (size_t)AKZ_AV_STATS * f;
        st[AKZ_AV_S_OBSERVATIONS] = n_final;
        st[AKZ_AV_S_MERGED] = 0u;
        st[AKZ_AV_S_DEMOTED] = 0u;
        st[AKZ_AV_S_NEW_LANDMARKS] = n_new;
    }
    if (accepted && threadIdx.x < 12u) a.poses[(size_t)12 * blk + threadIdx.x] = a.pose_out[(size_t)12 * f + threadIdx.x];
}

// the final match of this lane, in an accepted slot: 0 when there is none
__device__ __forceinline__ int lt_lane_match(const LtCall& a, uint32_t* f, uint32_t* blk, uint32_t* feature, uint32_t* la, uint32_t* lb)
{
    *f = blockIdx.y;
    const uint32_t i = blockIdx.x * kTblBlock + threadIdx.x;
    if (!a.accepted[*f] || i >= a.nmatches[*f] || !a.final_mask[(size_t)*f * a.cap + i]) return 0;   // accepted: nmatches <= cap
    *blk = a.frames[*f];
    return lt_match(a, *f, i, a.counts[*blk], feature, la, lb);          // never AKZ_LT_MATCH_BAD: the slot was accepted
}

__global__ __launch_bounds__(kTblBlock) void k_lt_refs(LtCall a)
{
    uint32_t f, blk, feature, la, lb;
    const int kind = lt_lane_match(a, &f, &blk, &feature, &la, &lb);
    if (!kind) return;
    atomicAdd(&a.refs[la], 1u);                                          // la, lb < n_landmarks: akz_lt_match
    if (kind == AKZ_LT_MATCH_MERGED) atomicAdd(&a.refs[lb], 1u);
}

__global__ __launch_bounds__(kTblBlock) void k_lt_merges(LtCall a)
{
    uint32_t f, blk, feature, la, lb;
    const int kind = lt_lane_match(a, &f, &blk, &feature, &la, &lb);
    if (!kind) return;
    atomicAdd(&a.adds[la], 1u);
    if (kind != AKZ_LT_MATCH_MERGED) return;
    if (akz_lt_merge_applied(a.refs[la], a.refs[lb])) {                  // nothing else names la or lb: this lane alone writes their words
        a.merged_from[la] = lb;
        a.merged_into[lb] = la;
        atomicAdd(&a.stats[(size_t)AKZ_AV_STATS * f + AKZ_AV_S_MERGED], 1u);
        atomicAdd(&a.info[kInfoMerged], 1u);
    } else {
        atomicAdd(&a.stats[(size_t)AKZ_AV_STATS * f + AKZ_AV_S_DEMOTED], 1u);
        atomicAdd(&a.info[kInfoDemoted], 1u);
    }
}

// the length of output row r < n_landmarks (the starts ascend: k_lt_check_table; m < n_landmarks: akz_lt_match)
__device__ __forceinline__ uint32_t lt_row_length(const LtCall& a, uint32_t r)
{
    if (a.info[kInfoBad] != 0u) return 0u;
    const uint32_t m = a.merged_from[r];
    const uint32_t merged = m != AKZ_LT_NONE ? a.obs_start[m + 1] - a.obs_start[m] : 0u;
    return akz_lt_row_length(a.obs_start[r + 1] - a.obs_start[r], merged, a.adds[r], a.merged_into[r] != AKZ_LT_NONE);
}

__global__ __launch_bounds__(kTblBlock) void k_lt_tile_sums(LtCall a)
{
    __shared__ uint32_t s_cnt[2][kTblWaves];
    uint32_t tick = 0u, sum = 0u;
#pragma unroll
    for (int j = 0; j < kTblItems; ++j) {
        const uint32_t r = blockIdx.x * kTblTile + (uint32_t)j * kTblBlock + threadIdx.x;    // n_landmarks + kTblTile < 2^32: rs_add_views_device
        if (r < a.n_landmarks) {
            const uint32_t len = lt_row_length(a, r);
            a.obs_counts_out[r] = len;
            sum += len;
        }
    }
    sum = akz_block_sum<kTblWaves>(s_cnt, tick, sum);
    if (threadIdx.x == 0) a.tile[blockIdx.x] = sum;
}

// ONE workgroup: tile sums -> tile offsets and slot rows -> the rows in front of a slot; the totals.
__global__ __launch_bounds__(kTblBlock) void k_lt_scan_sums(LtCall a)
{
    __shared__ uint32_t s_wave[kTblWaves];
    const uint32_t carry = tbl_scan_in_place(a.tile, a.n_tiles, s_wave), rows = tbl_scan_in_place(a.new_rows, a.n_frames, s_wave);
    if (threadIdx.x == 0) {
        const bool bad = a.info[kInfoBad] != 0u;
        uint32_t n_split = 0u;
        if (!bad && a.split) n_split = *a.split_count < a.split_room ? *a.split_count : a.split_room;
        // bad: no slot was accepted and every length was 0 — carry == rows == 0
        const uint32_t rows_filled = bad ? 0u : a.n_landmarks + n_split + rows;
        a.info[kInfoOld] = carry;
        a.info[kInfoRows] = rows_filled;
        a.info[kInfoSplit] = n_split;
        a.counts_out[AKZ_AV_C_ROWS] = rows_filled;
        a.counts_out[AKZ_AV_C_OBSERVATIONS] = carry + n_split + rows;
        a.counts_out[AKZ_AV_C_MERGED] = a.info[kInfoMerged];
        a.counts_out[AKZ_AV_C_DEMOTED] = a.info[kInfoDemoted];
        *a.call_verdict = bad ? AKZ_AV_BAD_TABLE : AKZ_AV_OK;
    }
}

// observation o is written at obs_out[at] as a member of row `key`
__device__ __forceinline__ void lt_put(const LtCall& a, uint32_t at, uint2 o, uint32_t key)
{
    tbl_put(a.obs_out, a.landmarks_out, a.n_blocks, a.cap, at, o, key);
}

__global__ __launch_bounds__(kTblBlock) void k_lt_rows(LtCall a)
{
    __shared__ uint32_t s_wave[kTblWaves];
    uint32_t run = a.tile[blockIdx.x];
#pragma unroll 1
    for (int j = 0; j < kTblItems; ++j) {
        const uint32_t r = blockIdx.x * kTblTile + (uint32_t)j * kTblBlock + threadIdx.x;
        const uint32_t len = r < a.n_landmarks ? a.obs_counts_out[r] : 0u;
        uint32_t dst = tbl_scan_step(run, len, s_wave);
        if (r >= a.n_landmarks) continue;
        a.obs_start_out[r] = dst;
        if (len == 0u) continue;                          // a tombstone, an empty row, or a refused table
        // dst + len <= the sum of all lengths <= n_obs + n_frames * cap <= obs_room; [s, e) inside [0, n_obs]
        for (uint32_t i = a.obs_start[r], e = a.obs_start[r + 1]; i < e; ++i) lt_put(a, dst++, a.obs[i], r);
        const uint32_t m = a.merged_from[r];
        if (m != AKZ_LT_NONE)
            for (uint32_t i = a.obs_start[m], e = a.obs_start[m + 1]; i < e; ++i) lt_put(a, dst++, a.obs[i], r);
    }
}

__global__ __launch_bounds__(kTblBlock) void k_lt_tail(LtCall a)
{
    const uint32_t k = blockIdx.x * kTblBlock + threadIdx.x;
    if (k > a.lm_room - a.n_landmarks) return;
    const uint32_t r = a.n_landmarks + k;
    if (a.info[kInfoBad] != 0u) {
        a.obs_start_out[r] = 0u;
        if (r < a.lm_room) a.obs_counts_out[r] = 0u;
        return;
    }
    const uint32_t rows_filled = a.info[kInfoRows], at = akz_lt_tail_start(a.info[kInfoOld], rows_filled, a.n_landmarks, r);
    a.obs_start_out[r] = at;
    if (r < a.lm_room) a.obs_counts_out[r] = r < rows_filled ? 1u : 0u;
    if (k < a.info[kInfoSplit]) lt_put(a, at, a.split[k], r);           // k < min(split_count, split_room)
}

__global__ __launch_bounds__(kTblBlock) void k_lt_place(LtCall a)
{
    uint32_t f, blk, feature, la, lb;
    if (!lt_lane_match(a, &f, &blk, &feature, &la, &lb)) return;
    // the row's new observations are its last adds[la]; cursor[la] < adds[la]: the same matches counted both
    const uint32_t at = a.obs_start_out[la + 1] - a.adds[la] + atomicAdd(&a.cursor[la], 1u);
    lt_put(a, at, make_uint2(blk, feature), la);
}

__global__ __launch_bounds__(kTblBlock) void k_lt_new_rows(LtCall a)
{
    __shared__ uint32_t s_cnt[2][kTblWaves];
    const uint32_t f = blockIdx.x;
    if (!a.accepted[f]) return;
    const uint32_t blk = a.frames[f], count = a.counts[blk];             // count <= cap: the slot was accepted
    const uint32_t* feat = a.feat + (size_t)f * a.cap;
    uint32_t row = a.n_landmarks + a.info[kInfoSplit] + a.new_rows[f], tick = 0u;
    for (uint32_t j0 = 0; j0 < count; j0 += kTblBlock) {
        const uint32_t j = j0 + threadIdx.x;
        const bool fresh = j < count && feat[j] == AKZ_LT_NONE;
        uint32_t total;
        const uint32_t rank = akz_block_scan<kTblWaves>(s_cnt, tick, fresh, &total);
        if (fresh) lt_put(a, akz_lt_tail_start(a.info[kInfoOld], a.info[kInfoRows], a.n_landmarks, row + rank), make_uint2(blk, j), row + rank);
        row += total;
    }
}

__global__ __launch_bounds__(kTblBlock) void k_lt_fixup(LtCall a)
{
    const uint32_t r = blockIdx.x * kTblBlock + threadIdx.x;
    if (r >= a.n_landmarks) return;
    const uint32_t n = a.adds[r];
    if (n < 2u) return;
    uint2* tail = a.obs_out + (a.obs_start_out[r + 1] - n);
    for (uint32_t i = 1; i < n; ++i) {                                   // insertion sort: a handful of entries, one per frame
        const uint2 o = tail[i];
        const uint32_t slot = a.block_slot[o.x];                         // o.x is a frame of the call: k_lt_place wrote it
        uint32_t k = i;
        while (k > 0u && akz_lt_tail_less(slot, o.y, a.block_slot[tail[k - 1u].x], tail[k - 1u].y)) {
            tail[k] = tail[k - 1u];
            --k;
        }
        tail[k] = o;
    }
}

}   // namespace

extern "C" int32_t rs_landmarks_sharing_view_device(rs_ctx* c, const void* d_obs_start, const void* d_obs, uint32_t n_obs, uint32_t n_landmarks,
                                                    const void* d_best, const void* d_decision, uint32_t cap_per_img, uint32_t n_frames,
                                                    void* d_merge_ok, void* stream_to_wait)
{
    return akz_guard([&]() -> int32_t {
        if (!d_obs_start || (n_obs != 0 && !d_obs) || !d_best || !d_decision || !d_merge_ok || !c) return AKZ_E_INVALID;
        if (cap_per_img == 0 || n_frames > 65535u || n_landmarks == 0xFFFFFFFFu) return AKZ_E_INVALID;
        const RsHandles h = rs_internal_handles(c);
        AKZ_TRY(akz_enqueue_behind(h, stream_to_wait));
        if (n_frames == 0) return AKZ_OK;
        hipLaunchKernelGGL(k_lt_sharing, dim3((cap_per_img + kTblBlock - 1) / kTblBlock, n_frames), dim3(kTblBlock), 0, h.stream,
                           (const uint32_t*)d_obs_start, (const uint32_t*)d_obs, n_obs, n_landmarks, (const uint32_t*)d_best,
                           (const uint32_t*)d_decision, cap_per_img, (unsigned char*)d_merge_ok);
        AKZ_LAUNCH_CHECK();
        return AKZ_OK;
    });
}

extern "C" int32_t rs_add_views_device(rs_ctx* c, const void* d_obs_start, const void* d_obs, uint32_t n_obs, uint32_t n_landmarks, uint32_t n_world,
                                       const void* d_split, const void* d_split_count, uint32_t split_room, uint32_t cap_per_img,
                                       uint32_t n_blocks, const uint32_t* ik, uint32_t n_frames, const void* d_counts, const void* d_matches,
                                       const void* d_nmatches, const void* d_final, const void* d_verdict, const void* d_pose_out,
                                       const void* d_best, const void* d_skip, uint32_t obs_room, uint32_t lm_room, void* d_poses,
                                       void* d_obs_start_out, void* d_obs_out, void* d_counts_out, void* d_landmarks_out,
                                       void* d_obs_counts_out, void* d_frame_verdict, void* d_stats, void* d_call_verdict, void* stream_to_wait)
{
    return akz_guard([&]() -> int32_t {
        if (!d_obs_start || (n_obs != 0 && !d_obs) || !d_obs_start_out || !d_obs_out || !d_counts_out || !d_landmarks_out || !d_obs_counts_out ||
            !d_call_verdict)
            return AKZ_E_INVALID;
        if (n_frames != 0 && (!ik || !d_counts || !d_matches || !d_nmatches || !d_final || !d_verdict || !d_pose_out || !d_poses ||
                              !d_frame_verdict || !d_stats))
            return AKZ_E_INVALID;
        if ((d_split == nullptr) != (d_split_count == nullptr) || (!d_split && split_room != 0)) return AKZ_E_INVALID;
        if (cap_per_img == 0 || n_blocks == 0 || n_frames > 65535u) return AKZ_E_INVALID;
        if (n_landmarks > 0xFFFFFFFFu - 2u * kTblTile) return AKZ_E_TOO_LARGE;      // row numbers of the last tile stay 32-bit
        // the rooms: no kernel can write past them (every feature of a frame adds one observation and at most one row)
        const uint64_t grow = (uint64_t)split_room + (uint64_t)n_frames * cap_per_img;
        if ((uint64_t)obs_room < (uint64_t)n_obs + grow || (uint64_t)lm_room < (uint64_t)n_landmarks + grow || lm_room == 0xFFFFFFFFu)
            return AKZ_E_INVALID;
        std::vector<unsigned char> seen;
        if (n_frames && !akz_distinct_blocks(ik, n_frames, n_blocks, &seen)) return AKZ_E_INVALID;
        // the input table is const: no output table may lie over it
        const void* in[2] = {d_obs_start, d_obs};
        const size_t in_bytes[2] = {sizeof(uint32_t) * ((size_t)n_landmarks + 1), sizeof(uint32_t) * 2 * (size_t)n_obs};
        const void* out[5] = {d_obs_start_out, d_obs_out, d_obs_counts_out, d_landmarks_out, d_counts_out};
        const size_t out_bytes[5] = {sizeof(uint32_t) * ((size_t)lm_room + 1), sizeof(uint32_t) * 2 * (size_t)obs_room, sizeof(uint32_t) * (size_t)lm_room,
                                     sizeof(uint32_t) * (size_t)n_blocks * cap_per_img, sizeof(uint32_t) * AKZ_AV_COUNTS};
        if (!akz_outputs_clear_of_inputs(in, in_bytes, 2, out, out_bytes, 5)) return AKZ_E_INVALID;
        if (!c) return AKZ_E_INVALID;
        const RsHandles h = rs_internal_handles(c);
        RsLandmarkTableState* ls = rs_internal_landmark_table(c);
        AKZ_TRY(akz_enqueue_behind(h, stream_to_wait));
        const uint32_t n_tiles = (uint32_t)(((size_t)n_landmarks + kTblTile - 1) / kTblTile);
        const size_t w = sizeof(uint32_t), lm_bytes = w * ((size_t)n_landmarks + 1), frame_bytes = w * ((size_t)n_frames + 1);
        AkzScratchPlan plan;                                             // zero: info .. cursor; none: merged_into .. block_slot
        const size_t at_info = plan.take(w * kInfoWords), at_refs = plan.take(lm_bytes), at_adds = plan.take(lm_bytes), at_cursor = plan.take(lm_bytes);
        const size_t at_into = plan.take(lm_bytes), at_from = plan.take(lm_bytes), at_slot = plan.take(w * (size_t)n_blocks);
        const size_t at_tile = plan.take(w * ((size_t)n_tiles + 1)), at_frames = plan.take(frame_bytes), at_accepted = plan.take(frame_bytes);
        const size_t at_new = plan.take(frame_bytes), at_feat = plan.take(w * ((size_t)n_frames * cap_per_img + 1));
        AKZ_TRY(akz_grow_scratch(h.stream, &ls->d_scratch, &ls->bytes, plan.size()));
        char* base = (char*)ls->d_scratch;
        LtCall a;
        a.obs_start = (const uint32_t*)d_obs_start; a.obs = (const uint2*)d_obs; a.split = (const uint2*)d_split;
        a.split_count = (const uint32_t*)d_split_count; a.counts = (const uint32_t*)d_counts; a.matches = (const uint32_t*)d_matches;
        a.nmatches = (const uint32_t*)d_nmatches; a.final_mask = (const unsigned char*)d_final; a.sv_verdict = (const uint32_t*)d_verdict;
        a.pose_out = (const double*)d_pose_out; a.best = (const uint32_t*)d_best; a.skip = (const uint32_t*)d_skip; a.poses = (double*)d_poses;
        a.obs_start_out = (uint32_t*)d_obs_start_out; a.obs_out = (uint2*)d_obs_out; a.counts_out = (uint32_t*)d_counts_out;
        a.landmarks_out = (uint32_t*)d_landmarks_out; a.obs_counts_out = (uint32_t*)d_obs_counts_out; a.frame_verdict = (uint32_t*)d_frame_verdict;
        a.stats = (uint32_t*)d_stats; a.call_verdict = (uint32_t*)d_call_verdict;
        a.info = (uint32_t*)(base + at_info); a.refs = (uint32_t*)(base + at_refs); a.adds = (uint32_t*)(base + at_adds);
        a.cursor = (uint32_t*)(base + at_cursor); a.merged_into = (uint32_t*)(base + at_into); a.merged_from = (uint32_t*)(base + at_from);
        a.block_slot = (uint32_t*)(base + at_slot); a.tile = (uint32_t*)(base + at_tile); a.frames = (uint32_t*)(base + at_frames);
        a.accepted = (uint32_t*)(base + at_accepted); a.new_rows = (uint32_t*)(base + at_new); a.feat = (uint32_t*)(base + at_feat);
        a.cap = cap_per_img; a.n_blocks = n_blocks; a.n_obs = n_obs; a.n_landmarks = n_landmarks; a.n_world = n_world;
        a.split_room = split_room; a.n_frames = n_frames; a.lm_room = lm_room; a.n_tiles = n_tiles;
        AKZ_HIP(hipMemsetAsync(base + at_info, 0, at_into - at_info, h.stream));
        AKZ_HIP(hipMemsetAsync(base + at_into, 0xFF, at_tile - at_into, h.stream));
        AKZ_HIP(hipMemsetAsync(d_landmarks_out, 0xFF, out_bytes[3], h.stream));
        if (n_frames) AKZ_HIP(hipMemcpyAsync(a.frames, ik, w * n_frames, hipMemcpyHostToDevice, h.stream));
        const dim3 block(kTblBlock), per_match((cap_per_img + kTblBlock - 1) / kTblBlock, n_frames ? n_frames : 1u);
        hipLaunchKernelGGL(k_lt_check_table, dim3(n_landmarks / kTblBlock + 1), block, 0, h.stream, a);
        AKZ_LAUNCH_CHECK();
        if (n_frames) {
            hipLaunchKernelGGL(k_lt_validate, dim3(n_frames), block, 0, h.stream, a);
            AKZ_LAUNCH_CHECK();
            hipLaunchKernelGGL(k_lt_refs, per_match, block, 0, h.stream, a);
            AKZ_LAUNCH_CHECK();
            hipLaunchKernelGGL(k_lt_merges, per_match, block, 0, h.stream, a);
            AKZ_LAUNCH_CHECK();
        }
        if (n_tiles) {
            hipLaunchKernelGGL(k_lt_tile_sums, dim3(n_tiles), block, 0, h.stream, a);
            AKZ_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(k_lt_scan_sums, dim3(1), block, 0, h.stream, a);
        AKZ_LAUNCH_CHECK();
        if (n_tiles) {
            hipLaunchKernelGGL(k_lt_rows, dim3(n_tiles), block, 0, h.stream, a);
            AKZ_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(k_lt_tail, dim3((lm_room - n_landmarks) / kTblBlock + 1), block, 0, h.stream, a);
        AKZ_LAUNCH_CHECK();
        if (n_frames) {
            hipLaunchKernelGGL(k_lt_place, per_match, block, 0, h.stream, a);
            AKZ_LAUNCH_CHECK();
            hipLaunchKernelGGL(k_lt_new_rows, dim3(n_frames), block, 0, h.stream, a);
            AKZ_LAUNCH_CHECK();
            if (n_landmarks) {
                hipLaunchKernelGGL(k_lt_fixup, dim3((n_landmarks + kTblBlock - 1) / kTblBlock), block, 0, h.stream, a);
                AKZ_LAUNCH_CHECK();
            }
        }
        return AKZ_OK;
    });
}
