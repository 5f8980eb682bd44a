// hm_place.hip — which frames a frame is compared with, on the device: hm_find_frames_batch_device of include/akz.h.
//   VSlamData::find_visually_similar_and_recent_frames   cv-sfm/src/lib.rs:597-668
//   try_localize: the reconstructions by views found     cv-sfm/src/lib.rs:853-855
// Two kernels per call.  k_place_dist: the Hamming distances of every query's hash to every stored hash, tiled (a workgroup
// owns 64 queries x 64 stored rows, both sides staged through LDS in chunks of 32 words, a 4 x 4 patch of accumulators per
// thread, xor + accumulating population count per word pair), u16 into the context's scratch.  k_place_select: one workgroup
// per query — the window of recent frames, the exact selection of the nearest hashes from a histogram of the row's distances
// (no sort of n_stored keys), the three filters, the chain, its split by reconstruction and the order of the groups.  Every
// decision is include/akz_place_math.h's, the text the host build compiles too.  The LDS atomics count (a histogram, frames per
// window slot): sums, whose arrival order reaches no output byte.
#include "akz_common.h"
#include "../../include/akz_place_math.h"

static_assert(HM_PL_OK == AKZ_PL_OK && HM_PL_BAD_INDEX == AKZ_PL_BAD_INDEX && HM_PL_BAD_TABLE == AKZ_PL_BAD_TABLE, "verdicts");
static_assert(HM_PL_COUNTS == AKZ_PL_COUNTS && HM_PL_C_RECENT == AKZ_PL_C_RECENT && HM_PL_C_SIMILAR == AKZ_PL_C_SIMILAR &&
              HM_PL_C_SEARCHED == AKZ_PL_C_SEARCHED && HM_PL_C_GROUPS == AKZ_PL_C_GROUPS && HM_PL_C_FREE == AKZ_PL_C_FREE, "counts");
static_assert(HM_PL_MAX_HASH_BYTES == AKZ_PL_MAX_HASH_BYTES && HM_PL_MAX_SEARCH == AKZ_PL_MAX_SEARCH && HM_PL_MAX_RECENT == AKZ_PL_MAX_RECENT &&
              HM_PL_NONE == AKZ_PL_NONE, "limits");
static_assert(8 * HM_PL_MAX_HASH_BYTES < 65536, "a distance fits 16 bits");

namespace {

// ---- distances ---------------------------------------------------------------------------------------------------------------
constexpr uint32_t kPlTileQ = 64, kPlTileS = 64;     // queries x stored rows of a workgroup
constexpr uint32_t kPlChunk = 32;                    // words of both sides staged per step
constexpr uint32_t kPlPitch = kPlChunk + 4;          // row pitch in LDS: 16-byte rows, and the 16 rows a b128 read touches start on 16 distinct 4-bank groups

__global__ __launch_bounds__(256) void k_place_dist(const uint32_t* __restrict__ hashes, uint32_t n_stored, uint32_t words,
                                                    const uint32_t* __restrict__ query, uint32_t nq, uint16_t* __restrict__ dist, size_t pitch)
{
    __shared__ __attribute__((aligned(16))) uint32_t sq[kPlTileQ * kPlPitch];
    __shared__ __attribute__((aligned(16))) uint32_t ss[kPlTileS * kPlPitch];
    __shared__ uint32_t s_row[kPlTileQ];
    const uint32_t tid = threadIdx.x, tx = tid & 15u, ty = tid >> 4;
    const uint32_t q0 = blockIdx.y * kPlTileQ;
    const size_t s0 = (size_t)blockIdx.x * kPlTileS;
    if (tid < kPlTileQ) {                                  // a query that names no stored row reads nothing: its side is zeros
        const uint32_t r = q0 + tid < nq ? query[q0 + tid] : AKZ_PL_NONE;
        s_row[tid] = r < n_stored ? r : AKZ_PL_NONE;
    }
    __syncthreads();
    uint32_t acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0u;
    for (uint32_t w0 = 0; w0 < words; w0 += kPlChunk) {
        const uint32_t cw = min(kPlChunk, words - w0);
#pragma unroll
        for (uint32_t e = 0; e < kPlTileQ * kPlChunk / 256u; ++e) {
            const uint32_t idx = tid + 256u * e, r = idx / kPlChunk, c = idx % kPlChunk;
            const uint32_t qrow = s_row[r];
            const size_t srow = s0 + r;
            sq[r * kPlPitch + c] = (qrow != AKZ_PL_NONE && c < cw) ? hashes[(size_t)qrow * words + w0 + c] : 0u;
            ss[r * kPlPitch + c] = (srow < n_stored && c < cw) ? hashes[srow * words + w0 + c] : 0u;
        }
        __syncthreads();
        const uint32_t cend = (cw + 3u) & ~3u;             // (the words past cw are zeros on both sides)
        for (uint32_t c = 0; c < cend; c += 4u) {
            uint4 a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = *reinterpret_cast<const uint4*>(&sq[(ty * 4u + i) * kPlPitch + c]);
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = *reinterpret_cast<const uint4*>(&ss[(tx + 16u * j) * kPlPitch + c]);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    acc[i][j] += (uint32_t)__popc(a[i].x ^ b[j].x);
                    acc[i][j] += (uint32_t)__popc(a[i].y ^ b[j].y);
                    acc[i][j] += (uint32_t)__popc(a[i].z ^ b[j].z);
                    acc[i][j] += (uint32_t)__popc(a[i].w ^ b[j].w);
                }
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t q = q0 + ty * 4u + i;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const size_t s = s0 + tx + 16u * j;
            if (q < nq && s < n_stored) dist[(size_t)q * pitch + s] = (uint16_t)acc[i][j];
        }
    }
}

// ---- one query: window, selection, filters, chain, groups ----------------------------------------------------------------------
constexpr int kPlThreads = 1024, kPlWaves = kPlThreads / 64;

struct PlArgs {
    const uint32_t *feed, *pos, *recon, *view, *query, *visible;
    const uint16_t* dist;                 // [queries of this launch][pitch], null when the search is left out
    size_t pitch;
    uint32_t n_stored, q_first;           // the launch's workgroup b is query q_first + b
    uint32_t num_similar, num_recent, recent_threshold, search_num, bins;
    uint32_t room, need;                  // the row pitch of the outputs; the longest chain of these parameters (<= room)
    uint32_t *found, *views_out, *group_recon, *group_start, *free_out, *counts, *verdict;
    akz_neighbor* search;
    // the workgroup's LDS, byte offsets: {win, wcnt} [slots], found [need], then either keys [np2 of search_num] u64 and hist [bins]
    // or, once the similar frames are known, what the groups need (PlGroupLds below)
    uint32_t off_found, off_keys, off_hist;
    uint32_t np2_need;
};
// the group phase's share of the LDS behind off_keys, for a chain of up to `need` entries
struct PlGroupLds {
    uint32_t mkeys, gkeys, memseg, segstart, segrank, glen, gstart, bytes;
};
__host__ __device__ inline PlGroupLds pl_group_lds(uint32_t need, uint32_t np2_need)
{
    PlGroupLds g;
    g.mkeys = 0u;
    g.gkeys = g.mkeys + 8u * np2_need;
    g.memseg = g.gkeys + 8u * np2_need;
    g.segstart = g.memseg + 4u * need;
    g.segrank = g.segstart + 4u * (need + 1u);
    g.glen = g.segrank + 4u * need;
    g.gstart = g.glen + 4u * need;
    g.bytes = g.gstart + 4u * need;
    return g;
}
inline uint32_t pl_np2(uint32_t n)
{
    uint32_t p = 1u;
    while (p < n) p <<= 1;
    return p;
}

__device__ __forceinline__ uint32_t pl_np2_device(uint32_t n) { return n <= 1u ? 1u : 1u << (32 - __clz((int)(n - 1u))); }

__global__ __launch_bounds__(kPlThreads) void k_place_select(const PlArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    __shared__ uint32_t cnt[2][kPlWaves];
    __shared__ uint32_t s_wave[kPlWaves];
    __shared__ uint32_t s_threshold, s_quota;
    const uint32_t tid = threadIdx.x;
    const uint32_t qi = A.q_first + blockIdx.x;
    uint32_t tick = 0;
    uint32_t* const my_counts = A.counts + (size_t)qi * AKZ_PL_COUNTS;

    // ---- the query
    const uint32_t q = A.query[qi], vis = A.visible ? A.visible[qi] : A.n_stored;
    uint32_t verdict = akz_pl_query_verdict(q, vis, A.n_stored);
    if (verdict != AKZ_PL_OK) {
        if (tid < AKZ_PL_COUNTS) my_counts[tid] = 0u;
        if (tid == 0) A.verdict[qi] = verdict;
        return;
    }
    const uint32_t feed_q = A.feed[q], pos_q = A.pos[q];
    const uint32_t nr = A.num_recent, slots = akz_pl_window_slots(nr);
    const uint32_t wanted = akz_pl_searched(A.search_num, vis);
    const bool searching = A.dist != nullptr && wanted != 0u;
    uint32_t* const win = reinterpret_cast<uint32_t*>(lds);
    uint32_t* const wcnt = win + slots;
    uint32_t* const found = reinterpret_cast<uint32_t*>(lds + A.off_found);
    unsigned long long* const keys = reinterpret_cast<unsigned long long*>(lds + A.off_keys);
    uint32_t* const hist = reinterpret_cast<uint32_t*>(lds + A.off_hist);
    const uint16_t* const drow = searching ? A.dist + (size_t)blockIdx.x * A.pitch : nullptr;

    // ---- one pass over the visible rows: the histogram of the distances, the frames on every slot of the window
    for (uint32_t t = tid; t < slots; t += kPlThreads) {
        win[t] = AKZ_PL_NONE;
        wcnt[t] = 0u;
    }
    if (searching)
        for (uint32_t b = tid; b < A.bins; b += kPlThreads) hist[b] = 0u;
    __syncthreads();
    for (uint32_t i = tid; i < vis; i += kPlThreads) {
        if (searching) atomicAdd(&hist[min((uint32_t)drow[i], A.bins - 1u)], 1u);
        uint32_t slot;
        if (nr && i != q && akz_pl_window_slot(A.feed[i], A.pos[i], feed_q, pos_q, nr, &slot)) {
            atomicAdd(&wcnt[slot], 1u);
            win[slot] = i;                                  // (two frames on a slot: the query is refused, the row is never read)
        }
    }
    __syncthreads();
    const uint32_t bad = akz_block_sum<kPlWaves>(cnt, tick, (tid < slots && akz_pl_slot_bad(tid, wcnt[tid], nr)) ? 1u : 0u);
    if (bad) {
        if (tid < AKZ_PL_COUNTS) my_counts[tid] = 0u;
        if (tid == 0) A.verdict[qi] = AKZ_PL_BAD_TABLE;
        return;
    }

    // ---- recent: the occupied slots in ascending position
    uint32_t n_recent = 0;
    {
        const bool has = tid < slots && wcnt[tid] != 0u;
        const uint32_t place = akz_block_scan<kPlWaves>(cnt, tick, has, &n_recent);
        if (has) found[place] = win[tid];
    }

    // ---- search: the threshold distance from the histogram, the ordered compaction, the sort of at most search_num keys
    uint32_t n_similar = 0;
    if (searching) {
        {
            const uint32_t per = (A.bins + kPlThreads - 1u) / kPlThreads;
            const uint32_t b0 = min(A.bins, tid * per), b1 = min(A.bins, b0 + per);
            uint32_t sum = 0;
            for (uint32_t b = b0; b < b1; ++b) sum += hist[b];
            uint32_t total;
            const uint32_t before = akz_block_exclusive<kPlWaves>(sum, s_wave, &total);
            uint32_t threshold, quota, unused;
            if (before < wanted && wanted - before <= sum && akz_pl_threshold_run(hist, b0, b1, before, wanted, &threshold, &quota, &unused)) {
                s_threshold = threshold;
                s_quota = quota;
            }
            __syncthreads();
        }
        const uint32_t threshold = s_threshold, quota = s_quota;
        const uint32_t np2 = pl_np2_device(wanted);
        for (uint32_t j = wanted + tid; j < np2; j += kPlThreads) keys[j] = ~0ull;
        uint32_t base_at = 0, base_take = 0;
        for (uint32_t i0 = 0; i0 < vis && base_take < wanted; i0 += kPlThreads) {
            const uint32_t i = i0 + tid;
            const bool in = i < vis;
            const uint32_t d = in ? (uint32_t)drow[i] : 0xFFFFFFFFu;
            uint32_t rank_at = quota, total_at = 0;
            if (base_at < quota) rank_at = base_at + akz_block_scan<kPlWaves>(cnt, tick, in && d == threshold, &total_at);
            const bool take = in && akz_pl_takes(d, threshold, rank_at, quota);
            uint32_t total_take;
            const uint32_t place = base_take + akz_block_scan<kPlWaves>(cnt, tick, take, &total_take);
            if (take && place < wanted) keys[place] = akz_pl_key(d, i);
            base_at += total_at;
            base_take += total_take;
        }
        __syncthreads();
        bitonic_sort_lds_u64<kPlThreads>(keys, np2);
        if (A.search) {
            akz_neighbor* const out = A.search + (size_t)qi * A.search_num;
            for (uint32_t j = tid; j < wanted; j += kPlThreads) out[j] = akz_neighbor{akz_pl_key_row(keys[j]), akz_pl_key_distance(keys[j])};
        }
        // ---- similar: the search list through the three filters, the first num_similar
        uint32_t kept = 0;
        for (uint32_t j0 = 0; j0 < wanted && kept < A.num_similar; j0 += kPlThreads) {
            const uint32_t j = j0 + tid;
            const uint32_t r = j < wanted ? akz_pl_key_row(keys[j]) : AKZ_PL_NONE;
            const bool keep = j < wanted && akz_pl_similar_keeps(r, A.feed[r], A.pos[r], q, feed_q, pos_q, nr, A.recent_threshold);
            uint32_t total;
            const uint32_t place = kept + akz_block_scan<kPlWaves>(cnt, tick, keep, &total);
            if (keep && place < A.num_similar) found[n_recent + place] = r;
            kept += total;
        }
        n_similar = min(kept, A.num_similar);
    }
    __syncthreads();                                        // found is complete; keys and hist are free

    // ---- chain: the free frames in chain order, the frames with a view as (reconstruction, chain position) keys
    const uint32_t n_chain = n_recent + n_similar;
    const PlGroupLds G = pl_group_lds(A.need, A.np2_need);
    unsigned char* const gl = lds + A.off_keys;
    unsigned long long* const mkeys = reinterpret_cast<unsigned long long*>(gl + G.mkeys);
    unsigned long long* const gkeys = reinterpret_cast<unsigned long long*>(gl + G.gkeys);
    uint32_t* const memseg = reinterpret_cast<uint32_t*>(gl + G.memseg);
    uint32_t* const segstart = reinterpret_cast<uint32_t*>(gl + G.segstart);
    uint32_t* const segrank = reinterpret_cast<uint32_t*>(gl + G.segrank);
    uint32_t* const glen = reinterpret_cast<uint32_t*>(gl + G.glen);
    uint32_t* const gstart = reinterpret_cast<uint32_t*>(gl + G.gstart);
    const size_t row = (size_t)qi * A.room;
    uint32_t n_free = 0;
    for (uint32_t e0 = 0; e0 < n_chain; e0 += kPlThreads) {
        const uint32_t e = e0 + tid;
        const uint32_t r = e < n_chain ? found[e] : 0u;
        const uint32_t rc = e < n_chain ? A.recon[r] : 0u;
        const bool is_free = e < n_chain && rc == AKZ_PL_NONE;
        uint32_t total;
        const uint32_t place = n_free + akz_block_scan<kPlWaves>(cnt, tick, is_free, &total);
        if (e < n_chain) {
            A.found[row + e] = r;
            if (is_free) A.free_out[row + place] = r;
            else mkeys[e - place] = akz_pl_member_key(rc, e);
        }
        n_free += total;
    }
    const uint32_t n_members = n_chain - n_free;
    const uint32_t np2m = pl_np2_device(n_members);
    __syncthreads();
    for (uint32_t m = n_members + tid; m < np2m; m += kPlThreads) mkeys[m] = ~0ull;
    __syncthreads();
    bitonic_sort_lds_u64<kPlThreads>(mkeys, np2m);

    // ---- groups: the runs of one reconstruction, ordered by (views found descending, reconstruction key)
    uint32_t n_groups = 0;
    for (uint32_t m0 = 0; m0 < n_members; m0 += kPlThreads) {
        const uint32_t m = m0 + tid;
        const bool head = m < n_members && (m == 0u || (uint32_t)(mkeys[m] >> 32) != (uint32_t)(mkeys[m - 1u] >> 32));
        uint32_t total;
        const uint32_t place = n_groups + akz_block_scan<kPlWaves>(cnt, tick, head, &total);   // heads before m
        if (m < n_members) {
            memseg[m] = head ? place : place - 1u;
            if (head) segstart[place] = m;
        }
        n_groups += total;
    }
    if (tid == 0) segstart[n_groups] = n_members;
    const uint32_t np2g = pl_np2_device(n_groups);
    __syncthreads();
    for (uint32_t s = tid; s < np2g; s += kPlThreads)
        gkeys[s] = s < n_groups ? akz_pl_group_key(segstart[s + 1u] - segstart[s], (uint32_t)(mkeys[segstart[s]] >> 32)) : ~0ull;
    __syncthreads();
    bitonic_sort_lds_u64<kPlThreads>(gkeys, np2g);
    for (uint32_t s = tid; s < n_groups; s += kPlThreads) {
        const uint32_t len = segstart[s + 1u] - segstart[s], rc = (uint32_t)(mkeys[segstart[s]] >> 32);
        const unsigned long long key = akz_pl_group_key(len, rc);
        uint32_t lo = 0, hi = n_groups;                    // the keys are distinct: the place of this run's among the sorted ones
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (gkeys[mid] < key) lo = mid + 1u;
            else hi = mid;
        }
        segrank[s] = lo;
        glen[lo] = len;
        A.group_recon[row + lo] = rc;
    }
    __syncthreads();
    uint32_t* const my_start = A.group_start + (size_t)qi * (A.room + 1u);
    uint32_t running = 0;
    for (uint32_t g0 = 0; g0 < n_groups; g0 += kPlThreads) {
        const uint32_t g = g0 + tid;
        uint32_t total;
        const uint32_t before = running + akz_block_exclusive<kPlWaves>(g < n_groups ? glen[g] : 0u, s_wave, &total);
        if (g < n_groups) {
            gstart[g] = before;
            my_start[g] = before;
        }
        running += total;
    }
    if (tid == 0) my_start[n_groups] = n_members;
    __syncthreads();
    for (uint32_t m = tid; m < n_members; m += kPlThreads) {
        const uint32_t s = memseg[m];
        A.views_out[row + gstart[segrank[s]] + (m - segstart[s])] = A.view[found[(uint32_t)mkeys[m]]];
    }
    if (tid == 0) {
        my_counts[AKZ_PL_C_RECENT] = n_recent;
        my_counts[AKZ_PL_C_SIMILAR] = n_similar;
        my_counts[AKZ_PL_C_SEARCHED] = wanted;
        my_counts[AKZ_PL_C_GROUPS] = n_groups;
        my_counts[AKZ_PL_C_FREE] = n_free;
        A.verdict[qi] = AKZ_PL_OK;
    }
}

// the distances of one launch pair stay below this many bytes of scratch: a call of more queries runs in several pairs
constexpr size_t kPlScratchBytes = (size_t)64 << 20;
constexpr uint32_t kPlLdsLimit = 160u * 1024u;

}   // namespace

extern "C" int32_t hm_place_params_default(hm_place_params* p)
{
    if (!p) return AKZ_E_INVALID;
    p->num_similar = 0u;         // cv-sfm/src/settings.rs:437-451
    p->num_recent = 32u;
    p->recent_threshold = 0u;
    p->search_num = 512u;
    return AKZ_OK;
}

extern "C" uint32_t hm_place_room(const hm_place_params* p) { return p ? akz_pl_room(p->num_similar, p->num_recent) : 0u; }

extern "C" int32_t hm_find_frames_batch_device(hm_ctx* c, const void* d_hashes, const void* d_feed, const void* d_pos, const void* d_recon,
                                               const void* d_view, uint32_t n_stored, uint32_t hash_bytes, const void* d_query,
                                               const void* d_visible, uint32_t nq, const hm_place_params* prm, uint32_t room, void* d_found,
                                               void* d_views_out, void* d_group_recon, void* d_group_start, void* d_free, void* d_search,
                                               void* d_counts, void* d_verdict, void* stream_to_wait)
{
    return akz_guard([&]() -> int32_t {
        if (!d_hashes || !d_feed || !d_pos || !d_recon || !d_view || !d_query || !prm || !d_found || !d_views_out || !d_group_recon ||
            !d_group_start || !d_free || !d_counts || !d_verdict)
            return AKZ_E_INVALID;
        if (hash_bytes == 0u || (hash_bytes & 3u) || nq > 65535u) return AKZ_E_INVALID;
        if (hash_bytes > (uint32_t)HM_PL_MAX_HASH_BYTES || prm->search_num > (uint32_t)HM_PL_MAX_SEARCH || prm->num_recent > (uint32_t)HM_PL_MAX_RECENT)
            return AKZ_E_TOO_LARGE;
        if (prm->num_similar > prm->search_num || room < akz_pl_room(prm->num_similar, prm->num_recent)) return AKZ_E_INVALID;
        if (!c) return AKZ_E_INVALID;
        if (nq == 0u) return AKZ_OK;
        const HmHandles h = hm_internal_handles(c);
        AKZ_TRY(akz_enqueue_behind(h.device, h.stream, h.ev, stream_to_wait));
        const bool searching = prm->search_num != 0u && (prm->num_similar != 0u || d_search != nullptr);

        PlArgs A;
        A.feed = (const uint32_t*)d_feed;
        A.pos = (const uint32_t*)d_pos;
        A.recon = (const uint32_t*)d_recon;
        A.view = (const uint32_t*)d_view;
        A.query = (const uint32_t*)d_query;
        A.visible = (const uint32_t*)d_visible;
        A.n_stored = n_stored;
        A.num_similar = prm->num_similar;
        A.num_recent = prm->num_recent;
        A.recent_threshold = prm->recent_threshold;
        A.search_num = prm->search_num;
        A.bins = akz_pl_bins(hash_bytes);
        A.room = room;
        A.found = (uint32_t*)d_found;
        A.views_out = (uint32_t*)d_views_out;
        A.group_recon = (uint32_t*)d_group_recon;
        A.group_start = (uint32_t*)d_group_start;
        A.free_out = (uint32_t*)d_free;
        A.counts = (uint32_t*)d_counts;
        A.verdict = (uint32_t*)d_verdict;
        A.search = (akz_neighbor*)d_search;
        A.need = akz_pl_room(prm->num_similar, prm->num_recent);
        A.np2_need = pl_np2(A.need);
        A.off_found = (uint32_t)akz_align_up(sizeof(uint32_t) * 2 * akz_pl_window_slots(prm->num_recent), 16);
        A.off_keys = (uint32_t)akz_align_up(A.off_found + sizeof(uint32_t) * (size_t)A.need, 16);
        const uint32_t key_bytes = searching ? 8u * pl_np2(prm->search_num) : 0u;
        A.off_hist = A.off_keys + key_bytes;
        const uint32_t select_bytes = key_bytes + (searching ? 4u * A.bins : 0u), group_bytes = pl_group_lds(A.need, A.np2_need).bytes;
        const uint32_t lds = A.off_keys + (select_bytes > group_bytes ? select_bytes : group_bytes);
        if (lds + 1024u > kPlLdsLimit) return AKZ_E_TOO_LARGE;                                   // (not reached inside the limits above)
        if (lds > 32768u) AKZ_HIP(hipFuncSetAttribute((const void*)k_place_select, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));

        // the distances: [queries of a launch pair][pitch] u16 in the context's scratch
        const size_t pitch = akz_align_up(n_stored ? n_stored : 1u, 64);
        uint32_t per_launch = nq;
        if (searching) {
            const size_t fit = kPlScratchBytes / (pitch * sizeof(uint16_t));
            per_launch = (uint32_t)(fit >= nq ? nq : fit < kPlTileQ ? kPlTileQ : fit / kPlTileQ * kPlTileQ);
            HmPlaceState* ps = hm_internal_place(c);
            AKZ_TRY(akz_grow_scratch(h.stream, &ps->d_scratch, &ps->bytes, (size_t)per_launch * pitch * sizeof(uint16_t)));
            A.dist = (const uint16_t*)ps->d_scratch;
        } else {
            A.dist = nullptr;
        }
        A.pitch = pitch;
        for (uint32_t q0 = 0; q0 < nq; q0 += per_launch) {
            const uint32_t n = nq - q0 < per_launch ? nq - q0 : per_launch;
            if (searching && n_stored) {
                hipLaunchKernelGGL(k_place_dist, dim3((uint32_t)(pitch / kPlTileS), (n + kPlTileQ - 1u) / kPlTileQ), dim3(256), 0, h.stream,
                                   (const uint32_t*)d_hashes, n_stored, hash_bytes / 4u, A.query + q0, n, (uint16_t*)A.dist, pitch);
                AKZ_LAUNCH_CHECK();
            }
            A.q_first = q0;
            hipLaunchKernelGGL(k_place_select, dim3(n), dim3(kPlThreads), lds, h.stream, A);
            AKZ_LAUNCH_CHECK();
        }
        return AKZ_OK;
    });
}
