// rs_repack.hip — a reconstruction repacked on gfx950: views removed (VSlamData::remove_view, cv-sfm/src/lib.rs:517-546, for
// every removed view at once), the landmark table compacted (tombstones, rows that lost every observation and the empty tail
// dropped), rows and blocks renumbered, the per-block pools and the constraints moved along, the frame table's views mapped.
// Integer data movement; every decision is include/akz_repack_math.h, the text the CPU checker (tests/cpp/repack_host.c)
// compiles too — parity: host build == HIP, byte for byte.
//
// rs_repack_table_device, in stream order:
//   k_rp_count       one workgroup per tile of kTblTile rows, one lane per row: is the row's range inside the table, are its
//                    indices good, how many of its observations stay.  A row longer than a wave is counted by its wave.  The
//                    same launch checks the map (a reference count per target: a second taker breaks it) and the range starts,
//                    and leaves the tile's sums: rows kept, observations kept.
//   k_rp_scan_sums   ONE workgroup: the tile sums become tile offsets behind a running carry; the verdict and the counts.
//   k_rp_rows        a workgroup scans its tile again (keep flags -> keys, kept lengths -> starts) and scatters the kept
//                    observations with their mapped block; a row longer than a wave is placed by its wave, by ballot rank, so
//                    that the bytes do not depend on arrival order.  atomicMin into d_landmarks_out behind a fill of 0xFFFFFFFF.
//   k_rp_tail        the starts and counts behind the kept rows (all of them on a refusal) and the mapped range starts.
// rs_gather_blocks_device: k_rp_map_check (the map's validity and its inverse), k_rp_gather (every row of dst is a row of src
// or zeros; 16-byte accesses where the row length and both pointers allow).
// rs_repack_constraints_device: k_rp_constraints, ONE workgroup: an ordered compaction behind a running carry, the tail, the
// mapped range starts.  hm_place_remap_views_device: k_rp_frames, elementwise.
// Nothing here waits on a value another workgroup has yet to write: the levels are separate launches; every loop is bounded by
// an argument of the call or a checked range.
#include "rs_table.h"
#include "../../include/akz_repack_math.h"

namespace {

constexpr uint32_t kRpWave = 64;                             // a row with more observations is walked by its wave

static_assert(RS_RP_OK == AKZ_RP_OK && RS_RP_BAD_TABLE == AKZ_RP_BAD_TABLE && RS_RP_BAD_INDEX == AKZ_RP_BAD_INDEX &&
              RS_RP_BAD_MAP == AKZ_RP_BAD_MAP && RS_RP_NO_ROOM == AKZ_RP_NO_ROOM, "verdicts");
static_assert(RS_RP_C_ROWS == AKZ_RP_C_ROWS && RS_RP_C_OBSERVATIONS == AKZ_RP_C_OBSERVATIONS && RS_RP_C_EMPTY_DROPPED == AKZ_RP_C_EMPTY_DROPPED &&
              RS_RP_C_ROWS_DROPPED == AKZ_RP_C_ROWS_DROPPED && RS_RP_C_OBS_DROPPED == AKZ_RP_C_OBS_DROPPED && RS_RP_COUNTS == AKZ_RP_COUNTS,
              "count words");
static_assert(RS_TVC_BAD_INDEX == AKZ_RP_TVC_BAD_INDEX && HM_PL_NONE == AKZ_RP_NONE, "the values the tails are filled with");

// words of RpCall::info
enum { kInfoBadTable = 0, kInfoBadMap = 1, kInfoBadIndex = 2, kInfoEmpty = 3, kInfoVerdict = 4, kInfoRows = 5, kInfoObs = 6, kInfoWords = 8 };

// everything the kernels of one rs_repack_table_device call share, by value
struct RpCall {
    const uint32_t* obs_start;    // [n_landmarks + 1]
    const uint2* obs;             // [n_obs]
    const uint32_t* map;          // [n_blocks] or null (the identity)
    const uint32_t* recon_start;  // [n_recons + 1] or null
    uint32_t* obs_start_out;      // [lm_room + 1]
    uint2* obs_out;               // [obs_room]
    uint32_t* obs_counts_out;     // [lm_room]
    uint32_t* landmarks_out;      // [n_blocks_out][cap]
    uint32_t* key_out;            // [n_landmarks]
    uint32_t* recon_start_out;    // [n_recons + 1] or null
    uint32_t* counts_out;         // [AKZ_RP_COUNTS]
    uint32_t* call_verdict;       // [1]
    // scratch
    uint32_t* info;               // [kInfoWords], zero in front of the call
    uint32_t* refs;               // [n_blocks_out], zero in front of the call: the blocks that take the target
    uint32_t* kept;               // [n_landmarks + 1] the observations a row keeps, then the kept rows below it
    uint32_t* tile_rows;          // [n_tiles] a tile's kept rows, then its offset
    uint32_t* tile_obs;           // [n_tiles] the same for the kept observations
    uint32_t cap, n_blocks, n_blocks_out, n_obs, n_landmarks, n_recons, obs_room, lm_room, n_tiles;
};

// entry b < n_blocks of a map that is not null: 1 when it breaks the map.  inv (or null, zero in front of the call) gets the block
// of every target, plus one.
__device__ __forceinline__ int rp_map_entry(const uint32_t* map, uint32_t b, uint32_t n_blocks_out, uint32_t* refs, uint32_t* inv)
{
    const uint32_t m = map[b];
    if (m == AKZ_RP_NONE) return 0;
    if (akz_rp_entry_bad(m, n_blocks_out)) return 1;
    if (akz_rp_target_shared(atomicAdd(&refs[m], 1u))) return 1;        // m < n_blocks_out
    if (inv) inv[m] = b + 1u;                                             // the only taker of m, or the map is refused; 0: none
    return 0;
}

__global__ __launch_bounds__(kTblBlock) void k_rp_count(RpCall a)
{
    __shared__ uint32_t s_cnt[2][kTblWaves];
    const uint32_t lane = threadIdx.x & 63u, g0 = blockIdx.x * kTblBlock + threadIdx.x, stride = gridDim.x * kTblBlock;
    int bad_table = 0, bad_map = 0, bad_index = 0;
    if (a.map)
        for (uint32_t b = g0; b < a.n_blocks; b += stride) bad_map |= rp_map_entry(a.map, b, a.n_blocks_out, a.refs, nullptr);
    if (a.recon_start)
        for (uint32_t r = g0; r <= a.n_recons; r += stride) bad_table |= akz_rp_range_bad(a.recon_start, r, a.n_recons, a.n_landmarks);
    if (g0 == 0u) bad_table |= akz_lt_start_bad(a.obs_start, a.n_landmarks, a.n_landmarks, a.n_obs);
    uint32_t tick = 0u, n_keep = 0u, n_len = 0u, n_empty = 0u;
#pragma unroll 1
    for (int j = 0; j < kTblItems; ++j) {
        const uint32_t r = blockIdx.x * kTblTile + (uint32_t)j * kTblBlock + threadIdx.x;     // n_landmarks + kTblTile < 2^32: the entry point
        const bool valid = r < a.n_landmarks;
        uint32_t s = 0u, e = 0u;
        const bool ok = valid && akz_rp_row_range(a.obs_start, r, a.n_obs, &s, &e);        // [s, e) inside [0, n_obs]
        if (valid && !ok) bad_table = 1;
        const uint32_t len = ok ? e - s : 0u;
        const bool wide = len > kRpWave;
        uint32_t kept = 0u;
        if (!wide)
            for (uint32_t i = s; i < s + len; ++i) {
                const uint2 o = a.obs[i];
                const int k = akz_rp_observation(a.map, o.x, o.y, a.n_blocks, a.cap);
                if (k < 0) bad_index = 1;
                else kept += (uint32_t)k;
            }
        tbl_for_wide_rows(wide, [&](int src) {              // wave-uniform: every lane walks the same rows
            const uint32_t ws = __shfl(s, src, 64), we = __shfl(e, src, 64);
            uint32_t cnt = 0u;
            for (uint32_t q0 = ws; q0 < we; q0 += 64u) {
                const uint32_t q = q0 + lane;
                int k = 0;
                if (q < we) {
                    const uint2 o = a.obs[q];
                    k = akz_rp_observation(a.map, o.x, o.y, a.n_blocks, a.cap);
                }
                if (k < 0) bad_index = 1;
                cnt += (uint32_t)__popcll(__ballot(k == 1));
            }
            if ((int)lane == src) kept = cnt;
        });
        if (valid) a.kept[r] = kept;
        n_keep += kept != 0u ? 1u : 0u;
        n_len += kept;
        n_empty += (ok && len == 0u) ? 1u : 0u;
    }
    n_keep = akz_block_sum<kTblWaves>(s_cnt, tick, n_keep);
    n_len = akz_block_sum<kTblWaves>(s_cnt, tick, n_len);
    n_empty = akz_block_sum<kTblWaves>(s_cnt, tick, n_empty);
    if (threadIdx.x == 0 && blockIdx.x < a.n_tiles) {
        a.tile_rows[blockIdx.x] = n_keep;
        a.tile_obs[blockIdx.x] = n_len;
        if (n_empty) atomicAdd(&a.info[kInfoEmpty], n_empty);             // an integer sum: the same in any order
    }
    tbl_flag(&a.info[kInfoBadTable], bad_table);
    tbl_flag(&a.info[kInfoBadMap], bad_map);
    tbl_flag(&a.info[kInfoBadIndex], bad_index);
}

// ONE workgroup: tile sums -> tile offsets; the verdict and the counts.
__global__ __launch_bounds__(kTblBlock) void k_rp_scan_sums(RpCall a)
{
    __shared__ uint32_t s_wave[kTblWaves];
    const uint32_t rows = tbl_scan_in_place(a.tile_rows, a.n_tiles, s_wave), observations = tbl_scan_in_place(a.tile_obs, a.n_tiles, s_wave);
    if (threadIdx.x == 0) {
        const uint32_t verdict = akz_rp_verdict(a.info[kInfoBadTable] != 0u, a.info[kInfoBadMap] != 0u, a.info[kInfoBadIndex] != 0u, rows,
                                                observations, a.lm_room, a.obs_room);
        const bool counted = akz_rp_counted(verdict);
        // counted: the starts ascend inside [0, n_obs], every row was counted
        const uint32_t old_obs = counted ? a.obs_start[a.n_landmarks] - a.obs_start[0] : 0u, empty = a.info[kInfoEmpty];
        a.info[kInfoVerdict] = verdict;
        a.info[kInfoRows] = rows;
        a.info[kInfoObs] = observations;
        a.kept[a.n_landmarks] = rows;                                      // the kept rows below n_landmarks: k_rp_tail's range starts
        a.counts_out[AKZ_RP_C_ROWS] = counted ? rows : 0u;
        a.counts_out[AKZ_RP_C_OBSERVATIONS] = counted ? observations : 0u;
        a.counts_out[AKZ_RP_C_EMPTY_DROPPED] = counted ? empty : 0u;
        a.counts_out[AKZ_RP_C_ROWS_DROPPED] = counted ? a.n_landmarks - rows - empty : 0u;
        a.counts_out[AKZ_RP_C_OBS_DROPPED] = counted ? old_obs - observations : 0u;
        *a.call_verdict = verdict;
    }
}

// kept observation {block, feature} of row `key` is written at obs_out[at]; only under AKZ_RP_OK: at < obs_room, block <
// n_blocks_out (the map is valid), feature < cap (k_rp_count) — tbl_put's test never fails
__device__ __forceinline__ void rp_put(const RpCall& a, uint32_t at, uint32_t block, uint32_t feature, uint32_t key)
{
    tbl_put(a.obs_out, a.landmarks_out, a.n_blocks_out, a.cap, at, make_uint2(block, feature), key);
}

__global__ __launch_bounds__(kTblBlock) void k_rp_rows(RpCall a)
{
    __shared__ uint32_t s_wave[kTblWaves];
    const uint32_t lane = threadIdx.x & 63u;
    const bool call_ok = a.info[kInfoVerdict] == (uint32_t)AKZ_RP_OK;
    uint32_t run_rows = a.tile_rows[blockIdx.x], run_obs = a.tile_obs[blockIdx.x];
#pragma unroll 1
    for (int j = 0; j < kTblItems; ++j) {
        const uint32_t r = blockIdx.x * kTblTile + (uint32_t)j * kTblBlock + threadIdx.x;
        const bool valid = r < a.n_landmarks;
        const uint32_t kept = valid ? a.kept[r] : 0u;
        const uint32_t key = tbl_scan_step(run_rows, kept != 0u ? 1u : 0u, s_wave);
        uint32_t dst = tbl_scan_step(run_obs, kept, s_wave);
        const bool live = call_ok && kept != 0u;           // call_ok: key < rows <= lm_room, dst + kept <= observations <= obs_room
        if (valid) {
            a.key_out[r] = live ? key : AKZ_RP_NONE;
            a.kept[r] = key;                                // only this lane reads the word: now the kept rows below r
        }
        uint32_t s = 0u, e = 0u;
        if (live) {
            a.obs_start_out[key] = dst;
            a.obs_counts_out[key] = kept;
            s = a.obs_start[r];                             // call_ok: every row's range lies inside [0, n_obs]
            e = a.obs_start[r + 1];
        }
        const bool wide = e - s > kRpWave;
        if (!wide)
            for (uint32_t i = s; i < e; ++i) {
                const uint2 o = a.obs[i];
                const uint32_t m = akz_rp_map(a.map, o.x);  // call_ok: o.x < n_blocks
                if (m != AKZ_RP_NONE) rp_put(a, dst++, m, o.y, key);
            }
        tbl_for_wide_rows(wide, [&](int src) {              // wave-uniform
            const uint32_t ws = __shfl(s, src, 64), we = __shfl(e, src, 64), wkey = __shfl(key, src, 64);
            uint32_t base = __shfl(dst, src, 64);
            for (uint32_t q0 = ws; q0 < we; q0 += 64u) {
                const uint32_t q = q0 + lane;
                uint2 o = make_uint2(0u, 0u);
                uint32_t m = AKZ_RP_NONE;
                if (q < we) {
                    o = a.obs[q];
                    m = akz_rp_map(a.map, o.x);
                }
                const uint32_t slot = tbl_wave_append(base, m != AKZ_RP_NONE, lane);
                if (m != AKZ_RP_NONE) rp_put(a, slot, m, o.y, wkey);
            }
        });
    }
}

__global__ __launch_bounds__(kTblBlock) void k_rp_tail(RpCall a)
{
    const uint32_t r = blockIdx.x * kTblBlock + threadIdx.x;               // the grid covers lm_room + 1 <= 2^32 - 1 lanes
    const bool call_ok = a.info[kInfoVerdict] == (uint32_t)AKZ_RP_OK;
    if (r <= a.lm_room && (!call_ok || r >= a.info[kInfoRows])) {
        a.obs_start_out[r] = call_ok ? a.info[kInfoObs] : 0u;
        if (r < a.lm_room) a.obs_counts_out[r] = 0u;
    }
    // call_ok: recon_start[r] <= n_landmarks (k_rp_count)
    if (a.recon_start_out && r <= a.n_recons) a.recon_start_out[r] = call_ok ? a.kept[a.recon_start[r]] : 0u;
}

// the blocks' pools: info, refs and inv zero in front of it (one fill)
__global__ __launch_bounds__(kTblBlock) void k_rp_map_check(const uint32_t* __restrict__ map, uint32_t n_blocks, uint32_t n_blocks_out,
                                                           uint32_t* refs, uint32_t* inv, uint32_t* info)
{
    const uint32_t b = blockIdx.x * kTblBlock + threadIdx.x;
    const int bad = b < n_blocks && rp_map_entry(map, b, n_blocks_out, refs, inv);
    tbl_flag(&info[kInfoBadMap], bad);
}

// T = uint4 or uint32_t; a row is `units` of them.  inv null: the identity.
template <typename T>
__global__ __launch_bounds__(kTblBlock) void k_rp_gather(const T* __restrict__ src, T* __restrict__ dst, const uint32_t* __restrict__ inv,
                                                        const uint32_t* __restrict__ info, uint32_t units, uint32_t n_blocks_out,
                                                        uint32_t* verdict)
{
    constexpr int kUnroll = 4;
    const bool bad = info[kInfoBadMap] != 0u;
    if (blockIdx.x == 0u && blockIdx.y == 0u && threadIdx.x == 0u) *verdict = bad ? AKZ_RP_BAD_MAP : AKZ_RP_OK;
    T zero;
    memset(&zero, 0, sizeof(T));
    for (uint32_t t = blockIdx.y; t < n_blocks_out; t += gridDim.y) {
        const uint32_t from = bad ? AKZ_RP_NONE : inv ? inv[t] - 1u : t; // a valid map: inv[t] - 1 < n_blocks, or 0 - 1 == none
        const T* in = src + (size_t)(from != AKZ_RP_NONE ? from : 0u) * units;
        T* out = dst + (size_t)t * units;
        for (uint32_t u0 = blockIdx.x * (kTblBlock * kUnroll) + threadIdx.x; u0 < units; u0 += gridDim.x * (kTblBlock * kUnroll)) {
            T v[kUnroll];
#pragma unroll
            for (int k = 0; k < kUnroll; ++k) {
                const uint32_t u = u0 + (uint32_t)k * kTblBlock;          // units <= 2^30 (row_bytes is a u32): u stays 32-bit
                v[k] = (from != AKZ_RP_NONE && u < units) ? in[u] : zero;
            }
#pragma unroll
            for (int k = 0; k < kUnroll; ++k) {
                const uint32_t u = u0 + (uint32_t)k * kTblBlock;
                if (u < units) out[u] = v[k];
            }
        }
    }
}

// ONE workgroup.  prefix [n + 1]: the kept constraints below every constraint.
__global__ __launch_bounds__(kTblBlock) void k_rp_constraints(const uint32_t* __restrict__ views, const double* __restrict__ poses,
                                                             const uint32_t* __restrict__ cverdict, const uint32_t* __restrict__ map,
                                                             const uint32_t* __restrict__ start, uint32_t n, uint32_t n_blocks,
                                                             uint32_t n_blocks_out, uint32_t n_ranges, uint32_t* __restrict__ views_out,
                                                             double* __restrict__ poses_out, uint32_t* __restrict__ cverdict_out,
                                                             uint32_t* __restrict__ count, uint32_t* __restrict__ start_out, uint32_t* prefix)
{
    __shared__ uint32_t s_cnt[2][kTblWaves];
    uint32_t tick = 0u, carry = 0u;
    for (uint32_t c0 = 0; c0 < n; c0 += kTblBlock) {
        const uint32_t c = c0 + threadIdx.x;
        const bool keep = c < n && akz_rp_constraint_kept(map, views + 3 * (size_t)c, n_blocks, n_blocks_out);
        uint32_t total;
        const uint32_t at = carry + akz_block_scan<kTblWaves>(s_cnt, tick, keep, &total);
        carry += total;
        if (c < n) prefix[c] = at;
        if (keep) {                                          // at <= c < n
            for (int k = 0; k < 3; ++k) views_out[3 * (size_t)at + k] = akz_rp_map(map, views[3 * (size_t)c + k]);
            cverdict_out[at] = cverdict[c];
            for (int k = 0; k < 24; ++k) poses_out[24 * (size_t)at + k] = poses[24 * (size_t)c + k];
        }
    }
    for (uint32_t i = carry + threadIdx.x; i < n; i += kTblBlock) {        // the room behind the count: triples no stage takes
        for (int k = 0; k < 3; ++k) views_out[3 * (size_t)i + k] = AKZ_RP_NONE;
        cverdict_out[i] = AKZ_RP_TVC_BAD_INDEX;
        for (int k = 0; k < 24; ++k) poses_out[24 * (size_t)i + k] = 0.0;
    }
    if (threadIdx.x == 0) {
        *count = carry;
        prefix[n] = carry;
    }
    __syncthreads();                                         // prefix is this workgroup's own
    if (start)
        for (uint32_t r = threadIdx.x; r <= n_ranges; r += kTblBlock) {
            const uint32_t s = start[r];
            start_out[r] = prefix[s < n ? s : n];
        }
}

__global__ __launch_bounds__(kTblBlock) void k_rp_frames(uint32_t* __restrict__ recon, uint32_t* __restrict__ view, uint32_t n_stored,
                                                        uint32_t which, const uint32_t* __restrict__ map, uint32_t n_blocks,
                                                        uint32_t* __restrict__ flags)
{
    const uint32_t i = blockIdx.x * kTblBlock + threadIdx.x;
    uint32_t v = 0u;
    const int k = i < n_stored ? akz_rp_frame(map, recon[i], view[i], which, n_blocks, &v) : 0;
    if (k == 1) view[i] = v;
    if (k == 2) recon[i] = AKZ_RP_NONE;
    tbl_flag(flags, k < 0);
}

}   // namespace

extern "C" int32_t rs_repack_table_device(rs_ctx* c, const void* d_obs_start, const void* d_obs, uint32_t n_obs, uint32_t n_landmarks,
                                          uint32_t cap_per_img, uint32_t n_blocks, const void* d_block_map, uint32_t n_blocks_out,
                                          const void* d_recon_start, uint32_t n_recons, uint32_t obs_room, uint32_t lm_room,
                                          void* d_obs_start_out, void* d_obs_out, void* d_obs_counts_out, void* d_landmarks_out,
                                          void* d_key_out, void* d_recon_start_out, void* d_counts_out, void* d_call_verdict,
                                          void* stream_to_wait)
{
    return akz_guard([&]() -> int32_t {
        if (!d_obs_start || (n_obs != 0 && !d_obs) || !d_obs_start_out || (obs_room != 0 && !d_obs_out) || (lm_room != 0 && !d_obs_counts_out) ||
            !d_counts_out || !d_call_verdict)
            return AKZ_E_INVALID;
        if ((n_landmarks != 0 && !d_key_out) || (n_blocks_out != 0 && !d_landmarks_out)) return AKZ_E_INVALID;
        if ((d_recon_start == nullptr) != (d_recon_start_out == nullptr) || (!d_recon_start && n_recons != 0)) return AKZ_E_INVALID;
        if (cap_per_img == 0 || n_blocks == 0 || lm_room == 0xFFFFFFFFu || n_recons == 0xFFFFFFFFu) return AKZ_E_INVALID;
        if (!d_block_map && n_blocks_out != n_blocks) return AKZ_E_INVALID;
        if (n_landmarks > 0xFFFFFFFFu - 2u * kTblTile) return AKZ_E_TOO_LARGE;      // row numbers of the last tile stay 32-bit
        const size_t w = sizeof(uint32_t);
        const void* in[4] = {d_obs_start, d_obs, d_block_map, d_recon_start};
        const size_t in_bytes[4] = {w * ((size_t)n_landmarks + 1), w * 2 * (size_t)n_obs, w * (size_t)n_blocks, w * ((size_t)n_recons + 1)};
        const void* out[8] = {d_obs_start_out, d_obs_out, d_obs_counts_out, d_landmarks_out, d_key_out, d_recon_start_out, d_counts_out, d_call_verdict};
        const size_t out_bytes[8] = {w * ((size_t)lm_room + 1), w * 2 * (size_t)obs_room, w * (size_t)lm_room, w * (size_t)n_blocks_out * cap_per_img,
                                     w * (size_t)n_landmarks, w * ((size_t)n_recons + 1), w * AKZ_RP_COUNTS, w};
        if (!akz_outputs_clear_of_inputs(in, in_bytes, 4, out, out_bytes, 8)) return AKZ_E_INVALID;
        if (!c) return AKZ_E_INVALID;
        const RsHandles h = rs_internal_handles(c);
        RsLandmarkTableState* ls = rs_internal_landmark_table(c);
        AKZ_TRY(akz_enqueue_behind(h, stream_to_wait));
        const uint32_t n_tiles = (uint32_t)(((size_t)n_landmarks + kTblTile - 1) / kTblTile);
        AkzScratchPlan plan;                                             // zero: info, refs
        const size_t at_info = plan.take(w * kInfoWords), at_refs = plan.take(w * ((size_t)n_blocks_out + 1)), at_kept = plan.take(w * ((size_t)n_landmarks + 1));
        const size_t at_tile_rows = plan.take(w * ((size_t)n_tiles + 1)), at_tile_obs = plan.take(w * ((size_t)n_tiles + 1));
        AKZ_TRY(akz_grow_scratch(h.stream, &ls->d_scratch, &ls->bytes, plan.size()));
        char* base = (char*)ls->d_scratch;
        RpCall a;
        a.obs_start = (const uint32_t*)d_obs_start; a.obs = (const uint2*)d_obs; a.map = (const uint32_t*)d_block_map;
        a.recon_start = (const uint32_t*)d_recon_start; a.obs_start_out = (uint32_t*)d_obs_start_out; a.obs_out = (uint2*)d_obs_out;
        a.obs_counts_out = (uint32_t*)d_obs_counts_out; a.landmarks_out = (uint32_t*)d_landmarks_out; a.key_out = (uint32_t*)d_key_out;
        a.recon_start_out = (uint32_t*)d_recon_start_out; a.counts_out = (uint32_t*)d_counts_out; a.call_verdict = (uint32_t*)d_call_verdict;
        a.info = (uint32_t*)(base + at_info); a.refs = (uint32_t*)(base + at_refs); a.kept = (uint32_t*)(base + at_kept);
        a.tile_rows = (uint32_t*)(base + at_tile_rows); a.tile_obs = (uint32_t*)(base + at_tile_obs);
        a.cap = cap_per_img; a.n_blocks = n_blocks; a.n_blocks_out = n_blocks_out; a.n_obs = n_obs; a.n_landmarks = n_landmarks;
        a.n_recons = n_recons; a.obs_room = obs_room; a.lm_room = lm_room; a.n_tiles = n_tiles;
        AKZ_HIP(hipMemsetAsync(base + at_info, 0, at_kept - at_info, h.stream));
        if (out_bytes[3]) AKZ_HIP(hipMemsetAsync(d_landmarks_out, 0xFF, out_bytes[3], h.stream));
        const dim3 block(kTblBlock);
        hipLaunchKernelGGL(k_rp_count, dim3(n_tiles ? n_tiles : 1u), block, 0, h.stream, a);
        AKZ_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_rp_scan_sums, dim3(1), block, 0, h.stream, a);
        AKZ_LAUNCH_CHECK();
        if (n_tiles) {
            hipLaunchKernelGGL(k_rp_rows, dim3(n_tiles), block, 0, h.stream, a);
            AKZ_LAUNCH_CHECK();
        }
        const uint32_t tail_lanes = lm_room > n_recons ? lm_room : n_recons;       // lanes 0 .. tail_lanes
        hipLaunchKernelGGL(k_rp_tail, dim3(tail_lanes / kTblBlock + 1), block, 0, h.stream, a);
        AKZ_LAUNCH_CHECK();
        return AKZ_OK;
    });
}

extern "C" int32_t rs_gather_blocks_device(rs_ctx* c, const void* d_src, void* d_dst, uint32_t row_bytes, uint32_t n_blocks,
                                           const void* d_block_map, uint32_t n_blocks_out, void* d_verdict, void* stream_to_wait)
{
    return akz_guard([&]() -> int32_t {
        if (!d_src || !d_dst || !d_verdict || row_bytes == 0 || (row_bytes & 3u) != 0 || n_blocks == 0) return AKZ_E_INVALID;
        if ((((uintptr_t)d_src | (uintptr_t)d_dst | (uintptr_t)d_block_map | (uintptr_t)d_verdict) & 3u) != 0) return AKZ_E_INVALID;   // 4-byte words at the least
        if (!d_block_map && n_blocks_out != n_blocks) return AKZ_E_INVALID;
        const size_t w = sizeof(uint32_t), src_bytes = (size_t)n_blocks * row_bytes, dst_bytes = (size_t)n_blocks_out * row_bytes;
        const auto over = akz_ranges_overlap;
        if (over(d_src, src_bytes, d_dst, dst_bytes) || over(d_block_map, w * n_blocks, d_dst, dst_bytes) || over(d_src, src_bytes, d_verdict, w) ||
            over(d_dst, dst_bytes, d_verdict, w) || over(d_block_map, w * n_blocks, d_verdict, w))
            return AKZ_E_INVALID;
        if (!c) return AKZ_E_INVALID;
        const RsHandles h = rs_internal_handles(c);
        RsLandmarkTableState* ls = rs_internal_landmark_table(c);
        AKZ_TRY(akz_enqueue_behind(h, stream_to_wait));
        AkzScratchPlan plan;                                             // zero: info, and refs and inv where there is a map
        const size_t at_info = plan.take(w * kInfoWords), at_refs = plan.take(w * ((size_t)n_blocks_out + 1)), at_inv = plan.take(w * ((size_t)n_blocks_out + 1));
        AKZ_TRY(akz_grow_scratch(h.stream, &ls->d_scratch, &ls->bytes, plan.size()));
        char* base = (char*)ls->d_scratch;
        uint32_t *info = (uint32_t*)(base + at_info), *refs = (uint32_t*)(base + at_refs), *inv = (uint32_t*)(base + at_inv);
        AKZ_HIP(hipMemsetAsync(base + at_info, 0, (d_block_map ? plan.size() : at_refs) - at_info, h.stream));
        if (d_block_map) {
            hipLaunchKernelGGL(k_rp_map_check, dim3((n_blocks + kTblBlock - 1) / kTblBlock), dim3(kTblBlock), 0, h.stream,
                               (const uint32_t*)d_block_map, n_blocks, n_blocks_out, refs, inv, info);
            AKZ_LAUNCH_CHECK();
        }
        const uint32_t* d_inv = d_block_map ? inv : nullptr;
        const bool wide = (row_bytes & 15u) == 0 && ((uintptr_t)d_src & 15u) == 0 && ((uintptr_t)d_dst & 15u) == 0;
        const uint32_t units = row_bytes / (wide ? 16u : 4u), per_block = kTblBlock * 4;
        const uint32_t gx = (units + per_block - 1) / per_block;
        const dim3 grid(gx < 256u ? gx : 256u, n_blocks_out == 0 ? 1u : n_blocks_out < 65535u ? n_blocks_out : 65535u);
        if (wide)
            hipLaunchKernelGGL(k_rp_gather<uint4>, grid, dim3(kTblBlock), 0, h.stream, (const uint4*)d_src, (uint4*)d_dst, d_inv,
                               (const uint32_t*)info, units, n_blocks_out, (uint32_t*)d_verdict);
        else
            hipLaunchKernelGGL(k_rp_gather<uint32_t>, grid, dim3(kTblBlock), 0, h.stream, (const uint32_t*)d_src, (uint32_t*)d_dst, d_inv,
                               (const uint32_t*)info, units, n_blocks_out, (uint32_t*)d_verdict);
        AKZ_LAUNCH_CHECK();
        return AKZ_OK;
    });
}

extern "C" int32_t rs_repack_constraints_device(rs_ctx* c, const void* d_views, const void* d_constraint_poses, const void* d_constraint_verdict,
                                                uint32_t n_constraints, const void* d_block_map, uint32_t n_blocks, uint32_t n_blocks_out,
                                                const void* d_start, uint32_t n_ranges, void* d_views_out, void* d_constraint_poses_out,
                                                void* d_constraint_verdict_out, void* d_count, void* d_start_out, void* stream_to_wait)
{
    return akz_guard([&]() -> int32_t {
        if (!d_count || n_blocks == 0 || n_constraints == 0xFFFFFFFFu || n_ranges == 0xFFFFFFFFu) return AKZ_E_INVALID;
        if (n_constraints != 0 && (!d_views || !d_constraint_poses || !d_constraint_verdict || !d_views_out || !d_constraint_poses_out ||
                                   !d_constraint_verdict_out))
            return AKZ_E_INVALID;
        if ((d_start == nullptr) != (d_start_out == nullptr) || (!d_start && n_ranges != 0)) return AKZ_E_INVALID;
        if (!d_block_map && n_blocks_out != n_blocks) return AKZ_E_INVALID;
        const size_t w = sizeof(uint32_t), n = n_constraints;
        const void* in[5] = {d_views, d_constraint_poses, d_constraint_verdict, d_block_map, d_start};
        const size_t in_bytes[5] = {w * 3 * n, sizeof(double) * 24 * n, w * n, w * (size_t)n_blocks, w * ((size_t)n_ranges + 1)};
        const void* out[5] = {d_views_out, d_constraint_poses_out, d_constraint_verdict_out, d_count, d_start_out};
        const size_t out_bytes[5] = {w * 3 * n, sizeof(double) * 24 * n, w * n, w, w * ((size_t)n_ranges + 1)};
        if (!akz_outputs_clear_of_inputs(in, in_bytes, 5, out, out_bytes, 5)) return AKZ_E_INVALID;
        if (!c) return AKZ_E_INVALID;
        const RsHandles h = rs_internal_handles(c);
        RsLandmarkTableState* ls = rs_internal_landmark_table(c);
        AKZ_TRY(akz_enqueue_behind(h, stream_to_wait));
        AKZ_TRY(akz_grow_scratch(h.stream, &ls->d_scratch, &ls->bytes, akz_align_up(w * (n + 1), 256)));
        hipLaunchKernelGGL(k_rp_constraints, dim3(1), dim3(kTblBlock), 0, h.stream, (const uint32_t*)d_views, (const double*)d_constraint_poses,
                           (const uint32_t*)d_constraint_verdict, (const uint32_t*)d_block_map, (const uint32_t*)d_start, n_constraints, n_blocks,
                           n_blocks_out, n_ranges, (uint32_t*)d_views_out, (double*)d_constraint_poses_out, (uint32_t*)d_constraint_verdict_out,
                           (uint32_t*)d_count, (uint32_t*)d_start_out, (uint32_t*)ls->d_scratch);
        AKZ_LAUNCH_CHECK();
        return AKZ_OK;
    });
}

extern "C" int32_t hm_place_remap_views_device(hm_ctx* c, void* d_recon, void* d_view, uint32_t n_stored, uint32_t recon, const void* d_block_map,
                                               uint32_t n_blocks, void* d_flags, void* stream_to_wait)
{
    return akz_guard([&]() -> int32_t {
        if (!d_flags || (n_stored != 0 && (!d_recon || !d_view)) || n_blocks == 0 || recon == HM_PL_NONE) return AKZ_E_INVALID;
        const size_t w = sizeof(uint32_t);
        const auto over = akz_ranges_overlap;
        if (over(d_block_map, w * n_blocks, d_recon, w * n_stored) || over(d_block_map, w * n_blocks, d_view, w * n_stored) ||
            over(d_recon, w * n_stored, d_view, w * n_stored) || over(d_flags, w, d_recon, w * n_stored) || over(d_flags, w, d_view, w * n_stored) ||
            over(d_flags, w, d_block_map, w * n_blocks))
            return AKZ_E_INVALID;
        if (!c) return AKZ_E_INVALID;
        const HmHandles h = hm_internal_handles(c);
        AKZ_TRY(akz_enqueue_behind(h.device, h.stream, h.ev, stream_to_wait));
        AKZ_HIP(hipMemsetAsync(d_flags, 0, w, h.stream));
        if (n_stored == 0) return AKZ_OK;
        hipLaunchKernelGGL(k_rp_frames, dim3((n_stored + kTblBlock - 1) / kTblBlock), dim3(kTblBlock), 0, h.stream, (uint32_t*)d_recon,
                           (uint32_t*)d_view, n_stored, recon, (const uint32_t*)d_block_map, n_blocks, (uint32_t*)d_flags);
        AKZ_LAUNCH_CHECK();
        return AKZ_OK;
    });
}
